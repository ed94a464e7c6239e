"""Edge-shape parity of the clip-and-step optimizer kernels (csrc/optim.hip) against per-step float64 references, at the shapes
where their code paths change: the second float4 slot of a thread, a second workgroup, a tail beside several workgroups, second
grid-stride trips, 1 .. 4096 partials, narrow / wide / two-pass / plain fold workgroups and plain workgroups that walk two
strides, and the eight instantiations of the late-fold launch with short fold workgroups, tails and 0 .. 4093 earlier partials.

Cases, references and the bar live in tests/optim_edge_cases.py; tests/test_optim_edge_cases_host.py proves on the CPU that the
inputs carry the bar and reach the paths they are named for.  Every parity check holds
  step, s1, s2  max |got - want64| <= 1e-5 * max |want64| (the applied step p_old - p_new, not the parameter); every measured
                error / scale goes to the parity log (tools/parity_summary.py sums it up)
  out_norm      rtol 1e-6 against the float64 norm
  bounds        every buffer has slack behind n, prefilled with NaN: those bits are unchanged after the launch
  param_copy    bit-equal to param
  determinism   two fresh runs of a case are bit-identical
and the folds are bit-exact against the documented summation order."""
import ctypes

import numpy as np
import pytest
import torch

import optim_edge_cases as E
from parity_log import record_parity

pytestmark = pytest.mark.gpu

SLACK = 64
EINVAL = -22
PMAX = 4096


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    from deeprl_amd.support import select_device, Config
    select_device(0)
    return Config.DEVICE


def _ids(cases):
    return [c["name"] for c in cases]


def _nan(n, dev, dtype=torch.float32):
    return torch.full((n,), float("nan"), dtype=dtype, device=dev)


def _buf(n, dev, values=None, offset=0):
    """n floats with NaN slack on both sides of [offset, offset + n); returns (whole buffer, the view)."""
    b = _nan(offset + n + SLACK, dev)
    if values is not None:
        b[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(dev)
    return b, b[offset:offset + n]


def _bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64 if x.dtype == np.float64 else x.dtype)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


def _slack_untouched(whole, offset, n, what):
    w = whole.detach().cpu().numpy()
    out = np.concatenate([w[:offset], w[offset + n:]])
    assert np.all(_bits(out) == _bits(np.float32("nan"))), what + ": written outside [0, n)"


def _close(kernel, case, what, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (kernel, case, what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), "%s[%s] %s: non-finite output" % (kernel, case, what)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s[%s] %s: err/scale %.3g (bar %.1g), scale %.3g" % (kernel, case, what, err / scale, E.BAR, scale))
    record_parity("optim_edges %s.%s[%s]" % (kernel, what, case), err_over_scale=err / scale, scale=scale)
    assert err <= E.BAR * scale, "%s[%s] %s: max abs err %.3e vs scale %.3e (%.2e of it, bar %.0e)" % (
        kernel, case, what, err, scale, err / scale, E.BAR)


def _parity(kernel, case, kind, before, grad, after, sqsum, max_norm, t, norm_got):
    """One step: before / after = dicts of float32 numpy p, s1, s2; norm_got None where the launch writes none."""
    w = E.ref_step(kind, before["p"], grad, before["s1"], before["s2"], sqsum, max_norm, t)
    _close(kernel, case, "step", before["p"].astype(np.float64) - after["p"].astype(np.float64), w["step"])
    _close(kernel, case, "s1", after["s1"], w["s1"])
    if w["s2"] is not None:
        _close(kernel, case, "s2", after["s2"], w["s2"])
    else:
        _same(after["s2"], before["s2"], "%s[%s]: plain RMSprop touched grad_avg" % (kernel, case))
    if norm_got is not None:
        print("%s[%s] norm: got %.9g want %.9g" % (kernel, case, norm_got, w["norm"]))
        record_parity("optim_edges %s.norm[%s]" % (kernel, case), rel=abs(norm_got - w["norm"]) / w["norm"])
        assert abs(norm_got - w["norm"]) <= 1e-6 * w["norm"], "%s[%s]: norm %.9g, float64 %.9g" % (kernel, case, norm_got, w["norm"])
    return w


class _State:
    """Parameter, two states and the parameter mirror of one run, each with NaN slack; s2 of plain RMSprop stays NaN."""

    def __init__(self, c, dev, offset=0):
        n = c["n"]
        self.n, self.offset, self.kind = n, offset, c["kind"]
        uses_s2 = E.KINDS[c["kind"]]["opt"] == "adam" or E.KINDS[c["kind"]]["centered"]
        self.whole, self.v = {}, {}
        for k, init in (("p", c["p0"]), ("s1", np.zeros(n)), ("s2", np.zeros(n) if uses_s2 else None), ("cp", None), ("g", None)):
            self.whole[k], self.v[k] = _buf(n, dev, init, offset)
        self.norm = _nan(1, dev)

    def set_grad(self, g):
        self.v["g"].copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)))

    def snap(self):
        return {k: self.v[k].detach().cpu().numpy().copy() for k in ("p", "s1", "s2", "cp", "g")}

    def check_bounds(self, what):
        for k in self.whole:
            _slack_untouched(self.whole[k], self.offset, self.n, "%s %s" % (what, k))


def _hp(kind):
    return {k: (float(v) if isinstance(v, float) else v) for k, v in E.KINDS[kind].items()}


def _launch_step(st, kind, partials, n_partials, max_norm, t, step_dev=None, copy=True, out_norm=True):
    """The two-launch step kernels of one kind on the state's views (dra_rmsprop_step(_copy) / dra_adam_step_counter)."""
    from deeprl_amd import ops
    h, v = _hp(kind), st.v
    norm = st.norm if out_norm else None
    if h["opt"] == "rmsprop":
        ops.rmsprop_step(v["p"], v["g"], v["s1"], v["s2"], partials, n_partials, max_norm, h["lr"], h["alpha"], h["eps"],
                         h["centered"], norm, param_copy=v["cp"] if copy else None)
    else:
        step_dev.fill_(t)
        ops.adam_step_counter(v["p"], v["g"], v["s1"], v["s2"], partials, n_partials, max_norm, h["lr"], h["beta1"], h["beta2"],
                              h["eps"], step_dev, norm, v["cp"] if copy else None)
    torch.cuda.synchronize()


# ------------------------------------------------------- dra_rmsprop_step(_copy), dra_adam_step_counter: two float4 slots
def _run_step_case(c, dev, copy):
    from deeprl_amd import ops
    st = _State(c, dev)
    partials = torch.zeros(ops.norm_partials(), dtype=torch.float64, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    trace = []
    for k in range(E.STEPS):
        st.set_grad(c["grads"][k])
        ops.grad_sqnorm(st.v["g"], partials)
        before = st.snap()
        _launch_step(st, c["kind"], partials, ops.norm_partials(), c["max_norm"], k + 1, step_dev, copy)
        trace.append(dict(before=before, after=st.snap(), norm=st.norm.item()))
        st.check_bounds("%s step %d" % (c["name"], k))
    return trace


@pytest.mark.parametrize("c", E.step_cases(), ids=_ids(E.step_cases()))
def test_two_slot_step_edges(dev, c):
    kernel = "rmsprop_step_copy" if E.KINDS[c["kind"]]["opt"] == "rmsprop" else "adam_step_counter"
    trace = _run_step_case(c, dev, copy=True)
    for k, tr in enumerate(trace):
        case = "%s step%d" % (c["name"], k)
        _parity(kernel, case, c["kind"], tr["before"], c["grads"][k], tr["after"], E.sqsum64(c["grads"][k]), c["max_norm"],
                k + 1, tr["norm"])
        _same(tr["after"]["cp"], tr["after"]["p"], case + ": param_copy is not the parameters")
        _same(tr["after"]["g"], c["grads"][k], case + ": the gradient was written")
    again = _run_step_case(c, dev, copy=True)
    plain = _run_step_case(c, dev, copy=False)          # dra_rmsprop_step / no mirror: the same bits, and no mirror written
    for k, tr in enumerate(trace):
        for key in ("p", "s1", "s2", "cp"):
            _same(again[k]["after"][key], tr["after"][key], "%s step %d: second run differs in %s" % (c["name"], k, key))
        for key in ("p", "s1", "s2"):
            _same(plain[k]["after"][key], tr["after"][key], "%s step %d: the run without a mirror differs in %s" % (c["name"], k, key))
        assert np.all(np.isnan(plain[k]["after"]["cp"])) and again[k]["norm"] == tr["norm"] == plain[k]["norm"]


@pytest.mark.parametrize("c", [c for c in E.step_cases() if c["kind"] == "adam"], ids=lambda c: c["name"])
def test_adam_step_counter_without_partials(dev, c):
    """partials = None (no clipping requested): clip_coef_from_partials returns before its barriers, so the bias corrections
    thread 0 leaves in LDS need a barrier of their own; every wave of every workgroup must step with them (found by the late-fold
    bit-identity cases: waves 1-3 stepped with whatever an earlier launch had left in LDS)."""
    st = _State(c, dev)
    st.set_grad(c["grads"][0])
    before = st.snap()
    _launch_step(st, "adam", None, 0, 0.0, 2, torch.zeros(1, dtype=torch.int64, device=dev))
    after = st.snap()
    st.check_bounds(c["name"])
    _parity("adam_step_counter", c["name"] + " no partials", "adam", before, c["grads"][0], after, 1.0, 0.0, 2, None)
    _same(after["cp"], after["p"], "param_copy is not the parameters")
    assert np.isnan(st.norm.item()), "out_norm written without partials"


# ------------------------------------------------------------------- dra_adam_step / dra_adam_step_dev: scalar grid-stride
def _run_adam_case(c, dev, form):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib
    st = _State(c, dev, c["offset"])
    h = _hp("adam")
    npart = ops.norm_partials()
    partials = torch.zeros(npart, dtype=torch.float64, device=dev)
    aligned = torch.zeros(c["n"], dtype=torch.float32, device=dev)        # dra_grad_sqnorm wants 16-byte alignment, the step does not
    trace = []
    for k in range(E.STEPS):
        st.set_grad(c["grads"][k])
        aligned.copy_(st.v["g"])
        ops.grad_sqnorm(aligned, partials)
        before, v = st.snap(), st.v
        if form == "host":
            ops.adam_step(v["p"], v["g"], v["s1"], v["s2"], partials, npart, c["max_norm"], h["lr"], h["beta1"], h["beta2"], h["eps"],
                          k + 1, st.norm)
        else:
            out2 = (ctypes.c_float * 2)()
            lib.dra_adam_hyper(h["lr"], h["beta1"], h["beta2"], k + 1, out2)
            hyper_dev = torch.tensor([out2[0], out2[1]], dtype=torch.float32, device=dev)
            ops.adam_step_dev(v["p"], v["g"], v["s1"], v["s2"], partials, npart, c["max_norm"], h["beta1"], h["beta2"], h["eps"],
                              hyper_dev, st.norm)
        torch.cuda.synchronize()
        trace.append(dict(before=before, after=st.snap(), norm=st.norm.item()))
        st.check_bounds("%s step %d" % (c["name"], k))
    return trace


@pytest.mark.parametrize("c", E.adam_cases(), ids=_ids(E.adam_cases()))
def test_adam_step_edges(dev, c):
    host = _run_adam_case(c, dev, "host")
    for k, tr in enumerate(host):
        case = "%s step%d" % (c["name"], k)
        _parity("adam_step", case, "adam", tr["before"], c["grads"][k], tr["after"], E.sqsum64(c["grads"][k]), c["max_norm"], k + 1,
                tr["norm"])
        _same(tr["after"]["g"], c["grads"][k], case + ": the gradient was written")
    devf, again = _run_adam_case(c, dev, "dev"), _run_adam_case(c, dev, "host")
    for k, tr in enumerate(host):
        for key in ("p", "s1", "s2"):
            _same(devf[k]["after"][key], tr["after"][key], "%s step %d: adam_step_dev differs from adam_step in %s" % (c["name"], k, key))
            _same(again[k]["after"][key], tr["after"][key], "%s step %d: second run differs in %s" % (c["name"], k, key))
        assert devf[k]["norm"] == tr["norm"] == again[k]["norm"]


# --------------------------------------------------------------------------------------------------- dra_grad_sqnorm
def _run_sqnorm(c, dev):
    from deeprl_amd import ops
    whole, g = _buf(c["n"], dev, c["grad"])
    npart = ops.norm_partials()
    partials = _nan(npart + 8, dev, torch.float64)
    slabs = None if c["slabs"] is None else torch.from_numpy(c["slabs"]).to(dev)
    ops.grad_sqnorm(g, partials, slabs, c["n_slabs"], c["stride"] if c["n_slabs"] else 0)
    torch.cuda.synchronize()
    _slack_untouched(whole, 0, c["n"], "grad_sqnorm[%s]" % c["name"])
    if slabs is not None:
        _same(slabs, c["slabs"], "grad_sqnorm[%s]: the slabs were written" % c["name"])
    return g.cpu().numpy(), partials.cpu().numpy(), npart


@pytest.mark.parametrize("c", E.sqnorm_cases(), ids=_ids(E.sqnorm_cases()))
def test_grad_sqnorm_edges(dev, c):
    g, partials, npart = _run_sqnorm(c, dev)
    want = E.fold_in_order(c["slabs"][:, :c["n"]]) if c["n_slabs"] else c["grad"]
    _same(g, want, "grad_sqnorm[%s]: the folded gradient is not the in-order float32 sum" % c["name"])
    assert np.all(np.isnan(partials[npart:])), "partials written behind dra_norm_partials()"
    assert np.all(np.isfinite(partials[:npart])) and np.all(partials[:npart] >= 0.0)
    got, sq = partials[:npart].sum(), E.sqsum64(want)
    print("grad_sqnorm[%s] sum of partials: rel err %.3g" % (c["name"], abs(got - sq) / sq))
    record_parity("optim_edges grad_sqnorm.partials[%s]" % c["name"], rel=abs(got - sq) / sq)
    assert abs(got - sq) <= 1e-6 * sq
    g2, partials2, _ = _run_sqnorm(c, dev)
    _same(g2, g, "second run: gradient")
    _same(partials2, partials, "second run: partials")


# ------------------------------------------------------------------------- clip_coef_from_partials through rmsprop_step
def _run_coef(c, dev, max_norm, with_partials=True):
    st = _State(c, dev)
    st.set_grad(c["grad"])
    partials = _nan(PMAX + 8, dev, torch.float64)              # NaN at and beyond n_partials: an entry too many poisons the norm
    partials[:c["n_partials"]] = torch.from_numpy(c["partials"]).to(dev)
    before = st.snap()
    _launch_step(st, c["kind"], partials if with_partials else None, c["n_partials"], max_norm, 1)
    st.check_bounds(c["name"])
    return before, st.snap(), st.norm.item()


@pytest.mark.parametrize("c", E.coef_cases(), ids=_ids(E.coef_cases()))
def test_clip_coef_from_partials_edges(dev, c):
    want32 = np.float32(np.sqrt(np.float64(c["sqsum"])))

    def norm_ok(what, got):
        ulps = abs(np.float64(got) - np.float64(want32)) / np.float64(np.spacing(want32))
        print("clip_coef[%s] %s: out_norm %.9g, float32(sqrt(float64 sum)) %.9g: %.1f ulp" % (c["name"], what, got, want32, ulps))
        record_parity("optim_edges clip_coef.norm_ulps[%s %s]" % (c["name"], what), ulps=ulps)
        assert ulps <= 1.0

    before, clipped, norm = _run_coef(c, dev, c["max_norm"])
    norm_ok("clipped", norm)
    w = _parity("clip_coef", c["name"] + " clipped", c["kind"], before, c["grad"], clipped, c["sqsum"], c["max_norm"], 1, norm)
    assert w["coef"] < 0.3
    _, free, norm0 = _run_coef(c, dev, 0.0)                    # max_norm = 0 does not clip; the norm is still written
    norm_ok("max_norm=0", norm0)
    _parity("clip_coef", c["name"] + " max_norm=0", c["kind"], before, c["grad"], free, c["sqsum"], 0.0, 1, norm0)
    _, clamped, norm1 = _run_coef(c, dev, float(np.float32(4.0 * np.sqrt(c["sqsum"]))))       # a norm below max_norm: coef is exactly 1
    _, none, norm_none = _run_coef(c, dev, c["max_norm"], with_partials=False)                # no partials: no clipping, no norm
    assert norm1 == norm0 == norm and np.isnan(norm_none), "out_norm: %r %r %r, without partials %r" % (norm, norm0, norm1, norm_none)
    for key in ("p", "s1", "s2", "cp"):
        _same(clamped[key], free[key], "a norm below max_norm must give the max_norm = 0 bits: " + key)
        _same(none[key], free[key], "partials = None must give the max_norm = 0 bits: " + key)
    _, again, norm2 = _run_coef(c, dev, c["max_norm"])
    assert norm2 == norm
    for key in ("p", "s1", "s2", "cp"):
        _same(again[key], clipped[key], "second run: " + key)


# ---------------------------------------------------------------------------------------------- dra_grad_sqnorm_segs
def _run_segs(c, dev):
    from deeprl_amd import ops
    st = _State(c, dev)
    st.set_grad(c["grad"])
    slabs = [torch.from_numpy(sl).to(dev) for sl in c["seg_slabs"]]
    segs, off = [], 0
    for cnt, ns, sl in zip(c["counts"], c["slabs"], slabs):
        segs.append((off, cnt, sl, cnt + c["pad"], ns))
        off += cnt
    partials = _nan(PMAX + 8, dev, torch.float64)
    n_ret = ops.grad_sqnorm_segs(st.v["g"], segs, partials)
    torch.cuda.synchronize()
    folded, parts = st.v["g"].cpu().numpy(), partials.cpu().numpy()
    before = st.snap()
    _launch_step(st, c["kind"], partials, n_ret, c["max_norm"], 1)
    st.check_bounds("grad_sqnorm_segs[%s]" % c["name"])
    return dict(n_ret=n_ret, segs=segs, folded=folded, partials=parts, before=before, after=st.snap(), norm=st.norm.item())


@pytest.mark.parametrize("layout", E.SEGS_LAYOUTS, ids=_ids(E.SEGS_LAYOUTS))
def test_grad_sqnorm_segs_edges(dev, layout):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib
    c = E.segs_case(layout)
    r = _run_segs(c, dev)
    b = ctypes.c_int(0)
    lib.dra_grad_sqnorm_segs_blocks(c["n"], ops._fold_seg_array(r["segs"]), len(r["segs"]), ctypes.byref(b))
    assert r["n_ret"] == b.value == c["expect"]["partials"], (r["n_ret"], b.value, c["expect"])
    _same(r["folded"], c["want"], "grad_sqnorm_segs[%s]: segments are not the ordered fold, or the plain part was written" % c["name"])
    parts = r["partials"]
    assert np.all(np.isnan(parts[r["n_ret"]:])), "partials written beyond the returned count"
    assert np.all(np.isfinite(parts[:r["n_ret"]])) and np.all(parts[:r["n_ret"]] >= 0.0)
    got, sq = parts[:r["n_ret"]].sum(), E.sqsum64(c["want"])
    print("grad_sqnorm_segs[%s] %d partials, sum: rel err %.3g" % (c["name"], r["n_ret"], abs(got - sq) / sq))
    record_parity("optim_edges grad_sqnorm_segs.partials[%s]" % c["name"], rel=abs(got - sq) / sq)
    assert abs(got - sq) <= 1e-6 * sq
    w = _parity("grad_sqnorm_segs+rmsprop_step", c["name"], c["kind"], r["before"], c["want"], r["after"], sq, c["max_norm"], 1, r["norm"])
    assert w["coef"] < 1.0
    _same(r["after"]["cp"], r["after"]["p"], "param_copy")
    again = _run_segs(c, dev)
    _same(again["partials"], parts, "second run: partials")
    for key in ("p", "s1", "s2"):
        _same(again["after"][key], r["after"][key], "second run: " + key)


# ------------------------------------------------------------------------------------------------ dra_clip_step_late
_LATE = dict(dead=False)      # a non-zero timeout flag invalidates the device-side hand-over: no further late launches this session


def _late_launch(c, st, slabs, partials, flag, max_norm, t, step_dev):
    """Arms the slots (-1.0, same stream) and launches; fails the test, and retires the late cases, on a timeout flag."""
    from deeprl_amd import ops
    h = _hp(c["kind"])
    fb = c["expect"]["fold_blocks"]
    partials[c["n_prior"]:c["n_prior"] + fb].fill_(-1.0)
    seg = (0, c["count"], slabs, c["stride"], c["n_slabs"])
    v = st.v
    if h["opt"] == "rmsprop":
        ops.clip_step_late(v["p"], v["g"], v["s1"], v["s2"], seg, partials, c["n_prior"], flag, ops.OPT_RMSPROP, max_norm,
                           (h["lr"], h["alpha"], h["eps"]), h["centered"], None, st.norm, v["cp"])
    else:
        step_dev.fill_(t)
        ops.clip_step_late(v["p"], v["g"], v["s1"], v["s2"], seg, partials, c["n_prior"], flag, ops.OPT_ADAM, max_norm,
                           (h["lr"], h["beta1"], h["eps"], h["beta2"]), False, step_dev, st.norm, v["cp"])
    torch.cuda.synchronize()
    if flag.item() != 0:
        _LATE["dead"] = True
        pytest.fail("clip_step_late[%s]: the timeout flag is %d: a fold workgroup's sum never arrived" % (c["name"], flag.item()))


def _run_late(c, dev, max_norm=None, only=None):
    """The case's three steps (or, with `only` = (k, state), step k from that state); max_norm None: the case's."""
    from deeprl_amd import ops
    assert ops.clip_step_late_blocks((0, c["count"], torch.zeros(4, device=dev), c["stride"], c["n_slabs"])) == c["expect"]["fold_blocks"]
    st = _State(c, dev)
    flag = torch.zeros(1, dtype=torch.int32).pin_memory()
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    partials = _nan(PMAX + 8, dev, torch.float64)
    trace = []
    for k in range(E.STEPS) if only is None else [only[0]]:
        if only is not None:
            for key in ("p", "s1", "s2"):
                st.v[key].copy_(torch.from_numpy(only[1][key]))
        x = E.late_step_inputs(c, k)
        g = np.full(c["n"], np.nan, dtype=np.float32)       # the segment's part of grad is written, never read
        g[c["count"]:] = c["rest"][k]
        st.set_grad(g)
        slabs = torch.from_numpy(x["slabs"]).to(dev)
        partials.fill_(float("nan"))
        partials[:c["n_prior"]] = torch.from_numpy(x["prior"]).to(dev)
        before = st.snap()
        _late_launch(c, st, slabs, partials, flag, c["max_norm"] if max_norm is None else max_norm, k + 1, step_dev)
        _same(slabs, x["slabs"], "clip_step_late[%s]: the slabs were written" % c["name"])
        trace.append(dict(before=before, after=st.snap(), norm=st.norm.item(), partials=partials.cpu().numpy().copy(), x=x))
        st.check_bounds("clip_step_late[%s] step %d" % (c["name"], k))
    return trace


@pytest.mark.parametrize("c", E.late_cases(), ids=_ids(E.late_cases()))
def test_clip_step_late_edges(dev, c):
    if _LATE["dead"]:
        pytest.skip("an earlier late-fold launch raised its timeout flag")
    kernel, fb, npr = "clip_step_late", c["expect"]["fold_blocks"], c["n_prior"]
    trace = _run_late(c, dev)
    for k, tr in enumerate(trace):
        case, x = "%s step%d" % (c["name"], k), tr["x"]
        _same(tr["after"]["g"][:c["count"]], x["fold"], case + ": the folded segment is not the NG-ordered float32 sum")
        _same(tr["after"]["g"][c["count"]:], c["rest"][k], case + ": grad behind the segment was written")
        parts = tr["partials"]
        _same(parts[:npr], x["prior"], case + ": the earlier partials were written")
        assert np.all(np.isnan(parts[npr + fb:])), case + ": partials written behind the slots"
        slots = parts[npr:npr + fb]
        assert np.all(slots >= 0.0), case + ": a slot still holds its flag value"
        rel = abs(slots.sum() - x["seg_sq"]) / x["seg_sq"]
        print("%s[%s] slots: rel err of their sum %.3g" % (kernel, case, rel))
        record_parity("optim_edges clip_step_late.slots[%s]" % case, rel=rel)
        assert rel <= 1e-6
        _parity(kernel, case, c["kind"], tr["before"], x["grad"], tr["after"], x["sqsum"], c["max_norm"], k + 1, tr["norm"])
        _same(tr["after"]["cp"], tr["after"]["p"], case + ": param_copy is not the parameters")
    again = _run_late(c, dev)
    for k, tr in enumerate(trace):
        for key in ("p", "s1", "s2", "cp", "g"):
            _same(again[k]["after"][key], tr["after"][key], "%s step %d: second run differs in %s" % (c["name"], k, key))
        _same(again[k]["partials"], tr["partials"], "second run: partials")
        assert again[k]["norm"] == tr["norm"]
    # max_norm = 0 from the state the last step started from: the bits of the two-launch kernel on the pre-folded gradient
    k = E.STEPS - 1
    start = trace[k]["before"]
    free = _run_late(c, dev, max_norm=0.0, only=(k, start))[0]
    ref = _State(c, dev)
    for key in ("p", "s1", "s2"):
        ref.v[key].copy_(torch.from_numpy(start[key]))
    ref.set_grad(trace[k]["x"]["grad"])
    _launch_step(ref, c["kind"], None, 0, 0.0, k + 1, torch.zeros(1, dtype=torch.int64, device=dev), out_norm=False)
    want = ref.snap()
    for key in ("p", "s1", "s2", "cp"):
        _same(free["after"][key], want[key], "%s: max_norm = 0 differs from the two-launch step on the folded gradient in %s" % (c["name"], key))
    assert abs(free["norm"] - np.sqrt(trace[k]["x"]["sqsum"])) <= 1e-6 * np.sqrt(trace[k]["x"]["sqsum"])      # the norm is still written


# ---------------------------------------------------------------------------------------------------- argument limits
def test_argument_limits_are_refused_before_any_launch(dev):
    """Every check the launchers make, through .raw: DRA_EINVAL, and nothing launched (the buffers are real and large enough
    for the launch each call describes, and keep their bits)."""
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, ptr, stream_ptr
    n = 257 * 256 + 8                     # floats: one more fold workgroup than the late launch allows, at 64 float4 each
    rs = np.random.RandomState(1)
    bufs = {k: torch.from_numpy(rs.standard_normal(n + 4).astype(np.float32)).to(dev) for k in ("p", "g", "s1", "s2", "cp")}
    keep = {k: v.clone() for k, v in bufs.items()}
    slabs = torch.zeros(161, 528, dtype=torch.float32, device=dev)
    one_slab = torch.zeros(1, n, dtype=torch.float32, device=dev)
    partials = torch.ones(8 + PMAX + 8, dtype=torch.float64, device=dev)[8:]      # slack on both sides
    partials[PMAX - 3:] = -1.0
    norm = torch.zeros(1, dtype=torch.float32, device=dev)
    step_dev = torch.ones(1, dtype=torch.int64, device=dev)
    hyper_dev = torch.ones(2, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32).pin_memory()
    s = stream_ptr()
    P = lambda k, off=0: ptr(bufs[k][off:])

    def rms(p=P("p"), g=P("g"), s1=P("s1"), s2=P("s2"), cnt=2052, parts=ptr(partials), npart=512, centered=1, cp=P("cp")):
        return lib.dra_rmsprop_step_copy.raw(p, g, s1, s2, cnt, parts, npart, 1.0, 1e-2, 0.95, 0.01, centered, ptr(norm), cp, s)

    def ctr(p=P("p"), cnt=2052, npart=512, sd=ptr(step_dev), cp=P("cp"), off=0):
        return lib.dra_adam_step_counter.raw(p, P("g", off), P("s1", off), P("s2", off), cnt, ptr(partials), npart, 1.0, 1e-2, 0.9, 0.999, 1e-8, sd,
                                             ptr(norm), cp, s)

    def adam(npart=512, step=1):
        return lib.dra_adam_step.raw(P("p"), P("g"), P("s1"), P("s2"), 2052, ptr(partials), npart, 1.0, 1e-2, 0.9, 0.999, 1e-8, step,
                                     ptr(norm), s)

    def adam_dev(npart=512, hd=ptr(hyper_dev)):
        return lib.dra_adam_step_dev.raw(P("p"), P("g"), P("s1"), P("s2"), 2052, ptr(partials), npart, 1.0, 0.9, 0.999, 1e-8, hd,
                                         ptr(norm), s)

    def sqnorm(g=P("g"), sl=ptr(slabs), ns=2, stride=528):
        return lib.dra_grad_sqnorm.raw(g, 516, sl, ns, stride, ptr(partials), s)

    def segs(g=P("g"), cnt=516, begin=0, count=516, sl=slabs, stride=528, ns=2):
        k = ctypes.c_int(0)
        return lib.dra_grad_sqnorm_segs.raw(g, cnt, ops._fold_seg_array([(begin, count, sl, stride, ns)]), 1, ptr(partials), ctypes.byref(k), s)

    def late(p=P("p"), g=P("g"), s2=P("s2"), cnt=1028, begin=0, count=516, sl=slabs, stride=528, ns=2, n_prior=0, opt=0, centered=1,
             sd=None, cp=P("cp"), s1=P("s1")):
        hp = (ctypes.c_float * 4)(1e-2, 0.9, 0.01, 0.999)
        return lib.dra_clip_step_late.raw(p, g, s1, s2, cnt, ops._fold_seg_array([(begin, count, sl, stride, ns)]), ptr(partials),
                                          n_prior, ptr(flag), opt, 1.0, hp, centered, sd, ptr(norm), cp, s)

    refused = {
        "rmsprop: param off by 4 bytes": rms(p=P("p", 1)), "rmsprop: grad off by 4 bytes": rms(g=P("g", 1)),
        "rmsprop: state off by 4 bytes": rms(s1=P("s1", 1)), "rmsprop: mirror off by 4 bytes": rms(cp=P("cp", 1)),
        "rmsprop: n = 3": rms(p=P("p", 4), g=P("g", 4), s1=P("s1", 4), s2=P("s2", 4), cp=P("cp", 4), cnt=3), "rmsprop: 0 partials": rms(npart=0), "rmsprop: 4097 partials": rms(npart=PMAX + 1),
        "rmsprop: centered without grad_avg": rms(s2=None),
        "adam_step_counter: param off by 4 bytes": ctr(p=P("p", 1)), "adam_step_counter: mirror off by 4 bytes": ctr(cp=P("cp", 1)),
        "adam_step_counter: n = 3": ctr(p=P("p", 4), cp=P("cp", 4), cnt=3, off=4), "adam_step_counter: 0 partials": ctr(npart=0),
        "adam_step_counter: 4097 partials": ctr(npart=PMAX + 1), "adam_step_counter: no step count": ctr(sd=None),
        "adam_step: 0 partials": adam(npart=0), "adam_step: 4097 partials": adam(npart=PMAX + 1), "adam_step: step 0": adam(step=0),
        "adam_step_dev: 0 partials": adam_dev(npart=0), "adam_step_dev: 4097 partials": adam_dev(npart=PMAX + 1),
        "adam_step_dev: no hyper tensor": adam_dev(hd=None),
        "grad_sqnorm: grad off by 4 bytes": sqnorm(g=P("g", 1)), "grad_sqnorm: slabs off by 4 bytes": sqnorm(sl=ptr(slabs.view(-1)[1:])),
        "grad_sqnorm: stride 530": sqnorm(stride=530), "grad_sqnorm: slabs missing": sqnorm(sl=None),
        "grad_sqnorm_segs: grad off by 4 bytes": segs(g=P("g", 1)), "grad_sqnorm_segs: n = 518": segs(cnt=518),
        "grad_sqnorm_segs: stride 530": segs(stride=530), "grad_sqnorm_segs: segment begins at 4": segs(cnt=520, begin=4),
        "grad_sqnorm_segs: slabs off by 4 bytes": segs(sl=slabs.view(-1)[1:]),
        "late: param off by 4 bytes": late(p=P("p", 1)), "late: grad off by 4 bytes": late(g=P("g", 1)),
        "late: mirror off by 4 bytes": late(cp=P("cp", 1)), "late: slabs off by 4 bytes": late(sl=slabs.view(-1)[1:]),
        "late: n = 3": late(p=P("p", 4), g=P("g", 4), s1=P("s1", 4), s2=P("s2", 4), cp=P("cp", 4), cnt=3, count=4), "late: stride 530": late(stride=530), "late: segment begins at 4": late(begin=4),
        "late: segment longer than n": late(cnt=512), "late: 161 slabs": late(ns=161), "late: 0 slabs": late(ns=0),
        "late: 257 fold workgroups": late(cnt=n, count=257 * 256, sl=one_slab, stride=n, ns=1),
        "late: n_prior + fold workgroups = 4097": late(n_prior=PMAX - 2), "late: negative n_prior": late(n_prior=-1),
        "late: Adam without a step count": late(opt=1), "late: centered RMSprop without state2": late(s2=None),
        "late: unknown optimizer": late(opt=2),
    }
    torch.cuda.synchronize()
    wrong = {k: rc for k, rc in refused.items() if rc != EINVAL}
    assert not wrong, "expected DRA_EINVAL (%d): %s" % (EINVAL, wrong)
    accepted = dict(late_256=lib.dra_clip_step_late_blocks.raw(ops._fold_seg_array([(0, 256 * 256, one_slab, n, 1)]), ctypes.byref(ctypes.c_int(0))))
    assert accepted["late_256"] == 0                              # the limit itself is valid
    for k in bufs:
        _same(bufs[k], keep[k], "a refused call wrote " + k)
    assert flag.item() == 0 and norm.item() == 0.0
