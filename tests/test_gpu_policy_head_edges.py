"""Edge-shape parity of the fused policy-head launches -- dra_linear_fwd_pair, dra_linear_bwd_pair, dra_policy_heads_sample /
_given / _given_fold / _sample_fold28 / _bwd, the head role of dra_rollout_conv1_heads_phi, and CategoricalActorCriticNet's
dispatch ladder over them -- against float64 references, at the shapes where the kernels change path.

Cases, references, the dispatch restatement and the bar live in tests/policy_head_edge_cases.py;
tests/test_policy_head_edge_cases_host.py proves on the CPU that every case reaches what it is named for and that its inputs carry
the bar.  Per case:
  parity        max |got - want64| <= 1e-5 * max |want64| per output tensor (E.bar); the measured fraction of the bar goes to the
                parity log, one record per case
  exactness     integer operand set: logits, v and all of linear_bwd_pair equal the int64 result; where float64 says exactly
                zero (A = 1, the ReLU mask, a null g_*) the kernel's value is zero; the fold is the numpy transcription bit for bit
  sampling      the sampled action is the float64 inverse CDF's on EVERY row (the host test proves the margins)
  bounds        every output sits in a buffer with NaN (int64: a marker) slack on both sides: those bits are unchanged; every
                input keeps its bits.  (The logits are one contiguous [B, A] block to every launch: no layout puts guards between rows.)
  determinism   two launches on fresh buffers are bit-identical
  refusals      DRA_EINVAL, and NaN-filled outputs stay NaN"""
import ctypes

import numpy as np
import pytest
import torch

import policy_head_edge_cases as E
from parity_log import record_parity

pytestmark = pytest.mark.gpu

SLACK = 64
EINVAL = -22
NAN_BITS = np.float32("nan").view(np.uint32)
I64_GUARD = -0x5EED5EED5EED
SENTINEL = np.float32(-7.03125e33)      # prefill of caller-owned gradient buffers: no gradient has this value


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    from deeprl_amd.support import select_device, Config
    select_device(0)
    return Config.DEVICE


def _ids(cases):
    return [c["name"] for c in cases]


class _Buf:
    """n elements with guard slack on both sides (float32: NaN, int64 / uint8: a marker); values given = an input whose bits are
    checked afterwards, else an output that starts as guard (or `fill`)."""

    def __init__(self, n, dev, values=None, dtype=torch.float32, fill=None):
        self.n, self.dtype = int(n), dtype
        self.guard = float("nan") if dtype == torch.float32 else (I64_GUARD if dtype == torch.int64 else 0xA5)
        self.whole = torch.full((SLACK + self.n + SLACK,), self.guard, dtype=dtype, device=dev)
        self.v = self.whole[SLACK:SLACK + self.n]
        self.values = None
        if values is not None:
            self.values = np.ascontiguousarray(values).reshape(-1).copy()
            assert self.values.size == self.n
            self.v.copy_(torch.from_numpy(self.values).to(dtype))
        elif fill is not None:
            self.v.fill_(float(fill))

    def ptr(self):
        return ctypes.c_void_p(self.v.data_ptr())

    def get(self, shape=None):
        a = self.v.detach().cpu().numpy().copy()
        return a if shape is None else a.reshape(shape)

    def _raw(self, a):
        return a.view(np.uint32) if a.dtype == np.float32 else a

    def slack_untouched(self, what):
        w = self.whole.detach().cpu().numpy()
        out = self._raw(np.concatenate([w[:SLACK], w[SLACK + self.n:]]))
        want = NAN_BITS if self.dtype == torch.float32 else self.guard
        assert np.all(out == want), what + ": written outside its buffer"

    def unchanged(self, what):
        self.slack_untouched(what)
        want = self.values.astype(np.float32) if self.dtype == torch.float32 else self.values
        assert np.array_equal(self._raw(self.get()), self._raw(want)), what + ": an input changed"

    def all_guard(self, what):
        w = self._raw(self.whole.detach().cpu().numpy())
        assert np.all(w == (NAN_BITS if self.dtype == torch.float32 else self.guard)), what + ": written"


def _p(b):
    return None if b is None else b.ptr()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype == np.float32:
        assert np.array_equal(_bits(a), _bits(b)), what
    else:
        assert np.array_equal(a, b), what


def _same_dicts(a, b, what):
    for k in a:
        _same(a[k], b[k], "%s: %s" % (what, k))


class _Figures:
    """The error / scale of every output tensor of one case: printed, recorded as a fraction of the bar, then judged."""

    def __init__(self, name):
        self.name, self.figs, self.fail = name, {}, []

    def add(self, key, got, want):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (self.name, key, got.shape, want.shape)
        if not np.all(np.isfinite(got)):
            self.fail.append("%s: non-finite output (%d elements)" % (key, int((~np.isfinite(got)).sum())))
            return
        scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
        fig = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
        b = E.bar(self.name, key.split(" ")[0])
        print("policy head edges %s %s: err/scale %.3g (bar %.1g), scale %.3g" % (self.name, key, fig, b, scale))
        self.figs[key] = max(self.figs.get(key, 0.0), fig / b)
        if not fig <= b:
            self.fail.append("%s: max abs err %.3e vs scale %.3e (%.2e of it, bar %.0e)" % (key, err, scale, fig, b))

    def exact(self, key, got, want):
        """The values of the exact result (-0.0 == 0.0), no NaN."""
        got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (self.name, key, got.shape, want.shape)
        bad = ~(got.astype(np.float64) == want)
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            self.fail.append("%s: %d of %d elements differ from the exact result, first at %s: got %r want %r" % (
                key, int(bad.sum()), bad.size, i, got[i], want[i]))

    def zero(self, key, got, where=None):
        got = np.asarray(got)
        sel = got if where is None else got[where]
        if (sel != 0).any() or np.isnan(sel).any():
            self.fail.append("%s: %d elements that float64 says are exactly zero are not" % (key, int((sel != 0).sum())))

    def actions(self, key, got, want):
        bad = np.asarray(got) != np.asarray(want)
        if bad.any():
            b = int(np.nonzero(bad)[0][0])
            self.fail.append("%s: %d of %d rows differ from the float64 inverse CDF, first row %d: got %d want %d" % (
                key, int(bad.sum()), bad.size, b, got[b], want[b]))

    def done(self):
        record_parity("policy head edges " + self.name, **{k.replace(" ", "_") + "_frac_of_bar": v for k, v in self.figs.items()})
        assert not self.fail, "%s: %s" % (self.name, "; ".join(self.fail))


def _sync():
    torch.cuda.synchronize()


def _lib():
    from deeprl_amd._lib import lib, stream_ptr
    return lib, stream_ptr


class _In:
    """The float32 / int64 operands of one launch on the device, each in its own guarded buffer; None stays a null pointer."""

    def __init__(self, dev, **arrays):
        self.b = {}
        for k, a in arrays.items():
            if a is None:
                self.b[k] = None
            else:
                a = np.asarray(a)
                dt = torch.int64 if a.dtype == np.int64 else torch.uint8 if a.dtype == np.uint8 else torch.float32
                self.b[k] = _Buf(a.size, dev, a, dtype=dt)

    def __getitem__(self, k):
        return _p(self.b[k])

    def unchanged(self, what):
        for k, b in self.b.items():
            if b is not None:
                b.unchanged("%s %s" % (what, k))


def _finish(name, rc, ins, outs):
    _sync()
    assert rc == 0, "%s returned %d" % (name, rc)
    ins.unchanged(name)
    for k, b in outs.items():
        b.slack_untouched("%s %s" % (name, k))


# ------------------------------------------------------------------------------------------------------- the launches
def _fwd_pair(dev, op, act):
    from deeprl_amd import ops
    lib, sp = _lib()
    B, K = op["x"].shape
    O0, O1 = op["w0"].shape[0], op["w1"].shape[0]
    ins = _In(dev, **{k: op[k] for k in ("x", "w0", "b0", "w1", "b1")})
    outs = dict(y0=_Buf(B * O0, dev), y1=_Buf(B * O1, dev))
    rc = lib.dra_linear_fwd_pair.raw(ins["x"], ins["w0"], ins["b0"], outs["y0"].ptr(), O0, ins["w1"], ins["b1"], outs["y1"].ptr(), O1,
                                     B, K, ops.ACT[act], sp())
    _finish("dra_linear_fwd_pair", rc, ins, outs)
    return dict(y0=outs["y0"].get((B, O0)), y1=outs["y1"].get((B, O1)))


def _sample(dev, op, x=None):
    lib, sp = _lib()
    x = op["x"] if x is None else x
    B, K = x.shape
    A = op["w0"].shape[0]
    ins = _In(dev, x=x, u=op["u"], **{k: op[k] for k in ("w0", "b0", "w1", "b1")})
    outs = dict(action=_Buf(B, dev, dtype=torch.int64), lp=_Buf(B, dev), ent=_Buf(B, dev), v=_Buf(B, dev), logits=_Buf(B * A, dev))
    rc = lib.dra_policy_heads_sample.raw(ins["x"], ins["w0"], ins["b0"], ins["w1"], ins["b1"], ins["u"], B, K, A, outs["action"].ptr(),
                                         outs["lp"].ptr(), outs["ent"].ptr(), outs["v"].ptr(), outs["logits"].ptr(), sp())
    _finish("dra_policy_heads_sample", rc, ins, outs)
    return {k: b.get((B, A) if k == "logits" else None) for k, b in outs.items()}


def _given(dev, op, action=None):
    lib, sp = _lib()
    B, K = op["x"].shape
    A = op["w0"].shape[0]
    ins = _In(dev, action=op["action"] if action is None else action, **{k: op[k] for k in ("x", "w0", "b0", "w1", "b1")})
    outs = dict(lp=_Buf(B, dev), ent=_Buf(B, dev), v=_Buf(B, dev), logits=_Buf(B * A, dev))
    rc = lib.dra_policy_heads_given.raw(ins["x"], ins["w0"], ins["b0"], ins["w1"], ins["b1"], ins["action"], B, K, A, outs["lp"].ptr(),
                                        outs["ent"].ptr(), outs["v"].ptr(), outs["logits"].ptr(), sp())
    _finish("dra_policy_heads_given", rc, ins, outs)
    return {k: b.get((B, A) if k == "logits" else None) for k, b in outs.items()}


def _given_fold(dev, op, KS):
    lib, sp = _lib()
    _, B, K = op["slabs"].shape
    A = op["w0"].shape[0]
    ins = _In(dev, slabs=op["slabs"], bias=op["bias"], action=op["action"], **{k: op[k] for k in ("w0", "b0", "w1", "b1")})
    outs = dict(lp=_Buf(B, dev), ent=_Buf(B, dev), v=_Buf(B, dev), logits=_Buf(B * A, dev), phi=_Buf(B * K, dev))
    rc = lib.dra_policy_heads_given_fold.raw(ins["slabs"], KS, ins["bias"], ins["w0"], ins["b0"], ins["w1"], ins["b1"], ins["action"], B, A,
                                             outs["lp"].ptr(), outs["ent"].ptr(), outs["v"].ptr(), outs["logits"].ptr(), outs["phi"].ptr(), sp())
    _finish("dra_policy_heads_given_fold", rc, ins, outs)
    return {k: b.get({"logits": (B, A), "phi": (B, K)}.get(k)) for k, b in outs.items()}


def _sample_fold28(dev, op):
    lib, sp = _lib()
    _, B, K = op["slabs"].shape
    A = op["w0"].shape[0]
    ins = _In(dev, slabs=op["slabs"], bias=op["bias"], u=op["u"], **{k: op[k] for k in ("w0", "b0", "w1", "b1")})
    outs = dict(action=_Buf(B, dev, dtype=torch.int64), lp=_Buf(B, dev), ent=_Buf(B, dev), v=_Buf(B, dev))
    rc = lib.dra_policy_heads_sample_fold28.raw(ins["slabs"], ins["bias"], ins["w0"], ins["b0"], ins["w1"], ins["b1"], ins["u"], B, A,
                                                outs["action"].ptr(), outs["lp"].ptr(), outs["ent"].ptr(), outs["v"].ptr(), sp())
    _finish("dra_policy_heads_sample_fold28", rc, ins, outs)
    return {k: b.get() for k, b in outs.items()}


def _grad_outs(dev, B, K, O0, O1, dx):
    """Caller-owned gradient buffers prefilled with the sentinel; dx null: a NaN stand-in that nothing may write."""
    outs = dict(dw0=_Buf(O0 * K, dev, fill=SENTINEL), db0=_Buf(O0, dev, fill=SENTINEL), dw1=_Buf(O1 * K, dev, fill=SENTINEL),
                db1=_Buf(O1, dev, fill=SENTINEL), dx=_Buf(B * K, dev, fill=SENTINEL if dx else None))
    return outs


def _grads_back(name, outs, B, K, O0, O1, dx):
    shapes = dict(dw0=(O0, K), db0=(O0,), dw1=(O1, K), db1=(O1,), dx=(B, K))
    got = {}
    for k, b in outs.items():
        if k == "dx" and not dx:
            b.all_guard(name + ": the dx stand-in of a null dx")
            continue
        got[k] = b.get(shapes[k])
        assert not np.any(_bits(got[k]) == _bits(SENTINEL)), "%s: %s is not fully overwritten" % (name, k)
    return got


def _heads_bwd(dev, op, c):
    lib, sp = _lib()
    B, K = op["x"].shape
    A = op["w0"].shape[0]
    ins = _In(dev, **{k: op[k] for k in ("logits", "action", "g_lp", "g_ent", "g_v", "x", "w0", "w1")})
    outs = _grad_outs(dev, B, K, A, 1, c["dx"])
    rc = lib.dra_policy_heads_bwd.raw(ins["logits"], ins["action"], ins["g_lp"], ins["g_ent"], ins["g_v"], ins["x"], ins["w0"], ins["w1"],
                                      outs["dx"].ptr() if c["dx"] else None, outs["dw0"].ptr(), outs["db0"].ptr(), outs["dw1"].ptr(),
                                      outs["db1"].ptr(), B, K, A, 1 if c["relu"] else 0, sp())
    _finish("dra_policy_heads_bwd", rc, ins, outs)
    return _grads_back(c["name"], outs, B, K, A, 1, c["dx"])


def _bwd_pair(dev, op, c):
    lib, sp = _lib()
    B, K = op["x"].shape
    O0, O1 = op["w0"].shape[0], op["w1"].shape[0]
    ins = _In(dev, **{k: op[k] for k in ("g0", "g1", "x", "w0", "w1")})
    outs = _grad_outs(dev, B, K, O0, O1, c["dx"])
    rc = lib.dra_linear_bwd_pair.raw(ins["g0"], ins["g1"], ins["x"], ins["w0"], ins["w1"], outs["dx"].ptr() if c["dx"] else None,
                                     outs["dw0"].ptr(), outs["db0"].ptr(), outs["dw1"].ptr(), outs["db1"].ptr(), B, K, O0, O1, sp())
    _finish("dra_linear_bwd_pair", rc, ins, outs)
    return _grads_back(c["name"], outs, B, K, O0, O1, c["dx"])


def _check_sampled(figs, got, op, tag=""):
    """A sampling launch's outputs against float64: the action on every row, log_pi_a of that action, entropy, v."""
    A = op["p"].shape[1]
    figs.actions("action" + tag, got["action"], op["sampled"])
    assert got["action"].min() >= 0 and got["action"].max() < A
    if np.array_equal(got["action"], op["sampled"]):
        figs.add("log_pi_a" + tag, got["lp"], op["lp_sampled"]) if A > 1 else figs.zero("log_pi_a" + tag, got["lp"])
    figs.add("entropy" + tag, got["ent"], op["ent"]) if A > 1 else figs.zero("entropy" + tag, got["ent"])


# --------------------------------------------------------------------------------------------------- forward tables
@pytest.mark.parametrize("c", E.FWD_CASES, ids=_ids(E.FWD_CASES))
def test_heads_forward_edges(dev, c):
    figs = _Figures(c["name"])
    op, ints = E.fwd_operands(c["name"], "random"), E.fwd_operands(c["name"], "integer")
    A = c["O0"]
    if c["kind"] == "fwd_pair":
        got = _fwd_pair(dev, op, c["act"])
        figs.add("y0", got["y0"], op["y0"])
        figs.add("y1", got["y1"], op["y1"])
        _same_dicts(got, _fwd_pair(dev, op, c["act"]), c["name"] + ": second launch differs")
        gi = _fwd_pair(dev, ints, None)
        figs.exact("y0 integer", gi["y0"], ints["y0"])
        figs.exact("y1 integer", gi["y1"], ints["y1"])
    else:
        run = _sample if c["kind"] == "sample" else _given
        got = run(dev, op)
        figs.add("logits", got["logits"], op["y0"])
        figs.add("v", got["v"], op["y1"][:, 0])
        if c["kind"] == "sample":
            _check_sampled(figs, got, op)
        elif A > 1:
            figs.add("log_pi_a", got["lp"], op["lp_given"])
            figs.add("entropy", got["ent"], op["ent"])
        else:       # one action: log 1 and the entropy of a point mass, exactly
            figs.zero("log_pi_a", got["lp"])
            figs.zero("entropy", got["ent"])
        _same_dicts(got, run(dev, op), c["name"] + ": second launch differs")
        gi = run(dev, ints)
        figs.exact("logits integer", gi["logits"], ints["y0"])
        figs.exact("v integer", gi["v"], ints["y1"][:, 0])
    figs.done()


# ------------------------------------------------------------------------------------------------------ fold tables
@pytest.mark.parametrize("c", E.FOLD_CASES, ids=_ids(E.FOLD_CASES))
def test_fold_forms_edges(dev, c):
    figs = _Figures(c["name"])
    op = E.fold_operands(c["name"])
    A = c["A"]
    if c["kind"] == "given_fold":
        got = _given_fold(dev, op, c["KS"])
        bad = _bits(got["phi"]) != _bits(op["phi"])
        assert not bad.any(), "%s: out_phi differs from the float32 transcription of the fold in %d of %d places (first %s)" % (
            c["name"], int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
        figs.add("logits", got["logits"], op["logits"])
        figs.add("v", got["v"], op["v"])
        if A > 1:
            figs.add("log_pi_a", got["lp"], op["lp_given"])
            figs.add("entropy", got["ent"], op["ent"])
        else:
            figs.zero("log_pi_a", got["lp"])
            figs.zero("entropy", got["ent"])
        _same_dicts(got, _given_fold(dev, op, c["KS"]), c["name"] + ": second launch differs")
        # the plain launch on the folded features: the same head, bit for bit
        plain = _given(dev, dict(op, x=op["phi"]))
        _same_dicts(plain, {k: got[k] for k in plain}, c["name"] + ": differs from dra_policy_heads_given on the same phi")
    else:
        got = _sample_fold28(dev, op)
        _check_sampled(figs, got, op)
        figs.add("v", got["v"], op["v"])
        _same_dicts(got, _sample_fold28(dev, op), c["name"] + ": second launch differs")
        plain = _sample(dev, op, x=op["phi"])
        _same_dicts(got, {k: plain[k] for k in got}, c["name"] + ": differs from dra_policy_heads_sample on the same phi")
        figs.add("logits", plain["logits"], op["logits"])
    figs.done()


@pytest.mark.parametrize("c", E.FC4_CASES, ids=_ids(E.FC4_CASES))
def test_fc4_policy_heads_given_through_ops(dev, c):
    """ops.fc4_policy_heads_given from fc4's input: the 8-slice one-pass forward and the folding head launch against one float64 chain."""
    from deeprl_amd import ops
    figs = _Figures(c["name"])
    op = E.fc4_operands(c["name"])
    t = {k: torch.from_numpy(op[k]).to(dev) for k in ("y3", "w4", "b4", "w0", "b0", "w1", "b1", "action")}
    keep = {k: v.clone() for k, v in t.items()}

    def run():
        out = ops.fc4_policy_heads_given(*[t[k] for k in ("y3", "w4", "b4", "w0", "b0", "w1", "b1", "action")])
        _sync()
        return dict(zip(("log_pi_a", "entropy", "v", "logits", "phi"), [o.cpu().numpy() for o in out]))

    got = run()
    for k, want in op["want"].items():
        figs.add(k, got[k], want)
    _same_dicts(got, run(), c["name"] + ": second call differs")
    for k in t:
        assert torch.equal(t[k], keep[k]), "%s: input %s changed" % (c["name"], k)
    # the stand-alone head on the phi this call returned: the same bits
    lp, ent, v, logits = ops.policy_heads_given(torch.from_numpy(got["phi"]).to(dev), t["w0"], t["b0"], t["w1"], t["b1"], t["action"])
    _sync()
    _same_dicts(dict(log_pi_a=lp.cpu().numpy(), entropy=ent.cpu().numpy(), v=v.cpu().numpy(), logits=logits.cpu().numpy()), got,
                c["name"] + ": differs from policy_heads_given on the same phi")
    figs.done()


# -------------------------------------------------------------------------------------------------- backward tables
@pytest.mark.parametrize("c", E.BWD_CASES, ids=_ids(E.BWD_CASES))
def test_heads_backward_edges(dev, c):
    from deeprl_amd import ops
    figs = _Figures(c["name"])
    op = E.bwd_operands(c["name"], "random")
    run = _heads_bwd if c["kind"] == "heads_bwd" else _bwd_pair
    got, w = run(dev, op, c), op["want"]
    for k in got:
        if float(np.abs(w[k]).max()) == 0.0:
            figs.zero(k, got[k])
        else:
            figs.add(k, got[k], w[k])
    if c["kind"] == "heads_bwd" and c["relu"] and c["dx"]:
        figs.zero("dx under the mask", got["dx"], op["x"] <= 0)
    _same_dicts(got, run(dev, op, c), c["name"] + ": second launch differs")
    # through ops: caller-owned buffers are the ones returned, with the same bits
    t = {k: None if op.get(k) is None else torch.from_numpy(op[k]).to(dev) for k in ("logits", "action", "g_lp", "g_ent", "g_v", "g0", "g1", "x", "w0", "w1") if k in op}
    own = [torch.full(got[k].shape, float(SENTINEL), dtype=torch.float32, device=dev) for k in ("dw0", "db0", "dw1", "db1")]
    if c["kind"] == "heads_bwd":
        back = ops.policy_heads_bwd(t["logits"], t["action"], t["g_lp"], t["g_ent"], t["g_v"], t["x"], t["w0"], t["w1"], *own,
                                    want_dx=c["dx"], relu_mask=c["relu"])
    else:
        back = ops.linear_bwd_pair(t["g0"], t["g1"], t["x"], t["w0"], t["w1"], *own, want_dx=c["dx"])
    _sync()
    assert (back[0] is None) == (not c["dx"])
    for k, o, r in zip(("dw0", "db0", "dw1", "db1"), own, back[1:]):
        assert r is o, "%s: ops returned another tensor than the caller's %s" % (c["name"], k)
        _same(o.cpu().numpy(), got[k], "%s: %s through ops differs from the raw launch" % (c["name"], k))
    if c["dx"]:
        _same(back[0].cpu().numpy(), got["dx"], c["name"] + ": dx through ops differs from the raw launch")
    if c["kind"] == "bwd_pair":
        ints = E.bwd_operands(c["name"], "integer")
        gi = run(dev, ints, c)
        for k in gi:
            figs.exact(k + " integer", gi[k], ints["want"][k])
    figs.done()


# ------------------------------------------------------------------------------------------- out-of-range given actions
@pytest.mark.parametrize("c", E.OOR_CASES, ids=_ids(E.OOR_CASES))
def test_out_of_range_actions_behave_as_the_nearest_valid_one(dev, c):
    """Forward AND backward: the gradient is the derivative of the value the forward returned."""
    from deeprl_amd import ops
    figs = _Figures(c["name"])
    op = E.oor_operands(c["name"])
    clamped = E.clamp_action(op["action"], c["A"])
    if c["kind"] == "categorical":
        logits, action = torch.from_numpy(op["logits"]).to(dev), torch.from_numpy(op["action"]).to(dev)
        _, lp, ent = ops.categorical_fwd(logits, action=action)
        dl = ops.categorical_bwd(logits, action, torch.from_numpy(op["g_lp"]).to(dev), torch.from_numpy(op["g_ent"]).to(dev))
        dl_c = ops.categorical_bwd(logits, torch.from_numpy(clamped).to(dev), torch.from_numpy(op["g_lp"]).to(dev),
                                   torch.from_numpy(op["g_ent"]).to(dev))
        _sync()
        figs.add("log_pi_a", lp.cpu().numpy(), op["lp"])
        figs.add("entropy", ent.cpu().numpy(), op["ent"])
        figs.add("dlogits", dl.cpu().numpy(), op["dlogits"])
        _same(dl.cpu().numpy(), dl_c.cpu().numpy(), c["name"] + ": dlogits differ from those of the clamped actions")
    else:
        got = _given(dev, op)
        figs.add("logits", got["logits"], op["logits"])
        figs.add("log_pi_a", got["lp"], op["lp"])
        figs.add("entropy", got["ent"], op["ent"])
        figs.add("v", got["v"], op["v"])
        bc = dict(name=c["name"], dx=True, relu=False)
        bop = dict(op, logits=got["logits"])
        back, want = _heads_bwd(dev, bop, bc), op["bwd"](got["logits"])
        for k in back:
            figs.add(k, back[k], want[k])
        _same_dicts(back, _heads_bwd(dev, dict(bop, action=clamped), bc), c["name"] + ": gradients differ from those of the clamped actions")
    figs.done()


# ---------------------------------------------------------------------------------------------------- sampling rows
@pytest.mark.parametrize("c", E.SAMPLING_CASES, ids=_ids(E.SAMPLING_CASES))
def test_sampling_rows_at_the_edge_uniforms(dev, c):
    from deeprl_amd import ops
    figs = _Figures(c["name"])
    op = E.sampling_operands(c["name"])
    got = _sample(dev, op) if c["kind"] == "sample" else _sample_fold28(dev, op)
    _check_sampled(figs, got, op)
    figs.add("v", got["v"], op["v"])
    if c["kind"] == "sample":
        figs.exact("logits", got["logits"], op["logits"])       # identity weights: the features themselves
        a, lp, ent = ops.categorical_fwd(torch.from_numpy(got["logits"]).to(dev), uniform=torch.from_numpy(op["u"]).to(dev))
        _sync()
        _same(a.cpu().numpy(), got["action"], c["name"] + ": dra_categorical_fwd samples differently")
        _same(lp.cpu().numpy(), got["lp"], c["name"] + ": dra_categorical_fwd log_pi_a")
        _same(ent.cpu().numpy(), got["ent"], c["name"] + ": dra_categorical_fwd entropy")
    figs.done()


# ------------------------------------------------------------------------------------------------------ riding head
def _riding(dev, c, op):
    lib, sp = _lib()
    B, A, mode = c["B"], c["A"], c["mode"]
    wt1 = np.ascontiguousarray(op["w1c"].transpose(1, 2, 3, 0))
    fold = mode.startswith("fold28")
    ins = _In(dev, frames=op["frames"], wt1=wt1, b1c=op["b1c"], u=op.get("u", np.zeros(B, np.float32)),
              prev=None if mode == "none" else op["slabs"] if fold else op["phi_plain"], bias=op["bias"] if fold else None,
              **{k: op[k] for k in ("w0", "b0", "w1", "b1")})
    outs = dict(y1=_Buf(B * 32 * 20 * 20, dev), action=_Buf(B, dev, dtype=torch.int64), lp=_Buf(B, dev), ent=_Buf(B, dev), v=_Buf(B, dev),
                phi=_Buf(B * 512, dev))
    rc = lib.dra_rollout_conv1_heads_phi.raw(ins["frames"], ins["wt1"], ins["b1c"], outs["y1"].ptr(), B, 1.0 / 255.0, ins["prev"], ins["bias"],
                                             ins["w0"], ins["b0"], ins["w1"], ins["b1"], ins["u"], A, outs["action"].ptr(), outs["lp"].ptr(),
                                             outs["ent"].ptr(), outs["v"].ptr(), outs["phi"].ptr() if mode == "fold28+phi" else None, sp())
    _finish("dra_rollout_conv1_heads_phi", rc, ins, outs)
    if mode == "none":
        for k in ("action", "lp", "ent", "v", "phi"):
            outs[k].all_guard("%s: %s without a head" % (c["name"], k))
    elif mode != "fold28+phi":
        outs["phi"].all_guard(c["name"] + ": out_phi was not given")
    return {k: b.get((B, 32, 20, 20) if k == "y1" else (B, 512) if k == "phi" else None) for k, b in outs.items()}


@pytest.mark.parametrize("c", E.RIDING_CASES, ids=_ids(E.RIDING_CASES))
def test_riding_head_edges(dev, c):
    from deeprl_amd import ops
    figs = _Figures(c["name"])
    op = E.riding_operands(c["name"])
    got = _riding(dev, c, op)
    frames = torch.from_numpy(op["frames"]).to(dev)
    wt1 = torch.from_numpy(np.ascontiguousarray(op["w1c"].transpose(1, 2, 3, 0))).to(dev)
    y1 = ops.conv_fwd_koc(1, [frames], [wt1], [torch.from_numpy(op["b1c"]).to(dev)], act="relu", u8_coef=1.0 / 255.0)[0]
    _sync()
    _same(got["y1"], y1.cpu().numpy(), c["name"] + ": y1 differs from ops.conv_fwd_koc of layer 1")
    if c["mode"] != "none":
        heads = ("action", "lp", "ent", "v")
        alone = _sample(dev, op, x=op["phi"]) if c["mode"] == "plain" else _sample_fold28(dev, op)
        _same_dicts({k: got[k] for k in heads}, {k: alone[k] for k in heads}, c["name"] + ": differs from the stand-alone launch")
        _check_sampled(figs, got, op)
        figs.add("v", got["v"], op["v"])
        if c["mode"] == "fold28+phi":
            assert np.array_equal(_bits(got["phi"]), _bits(op["phi_fold"])), c["name"] + ": out_phi differs from the float32 transcription of the fold"
    second = _riding(dev, c, op)
    _same_dicts({k: got[k] for k in ("y1", "v", "lp", "ent", "action", "phi")}, second, c["name"] + ": second launch differs")
    figs.done()


# ---------------------------------------------------------------------------------------------------- network level
class _Spy:
    """Counts calls of the ops entry points the ladder chooses between."""
    NAMES = ("policy_heads_sample", "policy_heads_given", "policy_heads_bwd", "linear_fwd_pair", "linear_bwd_pair", "linear_fwd",
             "categorical_fwd", "categorical_bwd")

    def __init__(self, monkeypatch):
        from deeprl_amd import ops
        self.n = {k: 0 for k in self.NAMES}
        for k in self.NAMES:
            monkeypatch.setattr(ops, k, self._wrap(k, getattr(ops, k)))

    def _wrap(self, k, fn):
        def call(*a, **kw):
            self.n[k] += 1
            return fn(*a, **kw)
        return call

    def path(self, body_linears):
        n = self.n
        if n["policy_heads_sample"]:
            return ("sample", "sample")
        if n["policy_heads_given"]:
            return ("policy_head_fn", "policy_head_fn")
        heads = ("linear_pair_fn" if n["linear_bwd_pair"] else "linear_fwd_pair") if n["linear_fwd_pair"] else "separate"
        if heads == "separate":
            assert n["linear_fwd"] == body_linears + 2, n
        return (heads, "categorical_policy" if n["categorical_fwd"] else "torch")


def _run_net(dev, c, op, direct, monkeypatch):
    import torch.nn.functional as Fn
    from deeprl_amd import nets
    with monkeypatch.context() as m:
        spy = _Spy(m)
        net = nets.CategoricalActorCriticNet(c["state_dim"], c["A"], nets.FCBody(c["state_dim"], (c["hidden"],), Fn.relu if c["gate"] == "relu" else torch.tanh))
        layer = net.phi_body.layers[0]
        params = dict(wb=layer.weight, bb=layer.bias, wa=net.fc_action.weight, ba=net.fc_action.bias, wc=net.fc_critic.weight, bc=net.fc_critic.bias)
        with torch.no_grad():
            for k, p in params.items():
                p.copy_(torch.from_numpy(op["params"][k]).to(dev))
        slots = {}
        if direct:      # contiguous .grad slots, as views of guarded buffers: the backward overwrites them in place
            for k, p in params.items():
                slots[k] = _Buf(p.numel(), dev, np.zeros(p.numel(), np.float32))
                p.grad = slots[k].v.view(p.shape)
        x = torch.from_numpy(op["x"]).to(dev).requires_grad_(c["grad"])
        net.rollout_slots.pin(torch.from_numpy(op["u"]).to(dev))
        action = torch.from_numpy(op["action"]).to(dev) if c["given"] else None
        with torch.set_grad_enabled(c["grad"]), nets.direct_param_grads(enable=direct):
            out = net(x, action)
            if c["grad"]:
                g = [torch.from_numpy(op[k]).to(dev) for k in ("g_lp", "g_ent", "g_v")]
                (g[0] * out["log_pi_a"].reshape(-1) + g[1] * out["entropy"].reshape(-1) + g[2] * out["v"].reshape(-1)).sum().backward()
        _sync()
        path = spy.path(1)
    got = {k: out[k].detach().reshape(-1).cpu().numpy() for k in ("log_pi_a", "entropy", "v")}
    got["action"] = out["action"].detach().cpu().numpy()
    if c["grad"]:
        got["dx"] = x.grad.cpu().numpy()
        for k, p in params.items():
            got["d" + k] = p.grad.detach().cpu().numpy().copy()
            if direct:
                slots[k].slack_untouched("%s %s .grad slot" % (c["name"], k))
    return got, path


@pytest.mark.parametrize("c", E.NET_CASES, ids=_ids(E.NET_CASES))
def test_net_dispatch_ladder_edges(dev, c, monkeypatch):
    figs = _Figures(c["name"])
    op = E.net_operands(c["name"])
    runs = [_run_net(dev, c, op, direct, monkeypatch) for direct in ((True, False) if c["grad"] else (False,))]
    for (got, path), form in zip(runs, ("direct", "accumulated")):
        assert path == c["reaches"] == E.head_path(c["hidden"], c["A"], c["B"], c["grad"], c["given"]), (c["name"], form, path)
        if c["given"]:
            assert np.array_equal(got["action"], op["action"])
        elif c["reaches"][1] != "torch":        # the uniforms the net consumed are the pinned ones
            figs.actions("action " + form, got["action"], op["sampled"])
        assert got["action"].min() >= 0 and got["action"].max() < c["A"]
        want = E.net_ref(op, c, got["action"])
        for k in got:
            if k != "action":
                figs.add("%s %s" % (k, form), got[k], want[k])
    figs.done()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_argument_limits_are_refused_before_any_launch(dev):
    """Every argument check of the launchers, through .raw: DRA_EINVAL, nothing launched -- the buffers are real and large enough
    for any launch the accepted arguments would describe, and the NaN-filled outputs keep their bits."""
    lib, sp = _lib()
    n = 1 << 17
    f = lambda: _Buf(n, dev, np.zeros(n, np.float32))
    x, w0, b0, w1, b1, u, g = (f() for _ in range(7))
    act = _Buf(n, dev, np.zeros(n, np.int64), dtype=torch.int64)
    frames = _Buf(4 * 84 * 84, dev, np.zeros(4 * 84 * 84, np.uint8), dtype=torch.uint8)
    o = [_Buf(n, dev) for _ in range(6)]
    oa = _Buf(n, dev, dtype=torch.int64)
    P = lambda b: b.ptr()
    calls = []

    def refuse(what, fn, *args):
        rc = fn.raw(*args)
        calls.append(what)
        assert rc == EINVAL, "%s: returned %d" % (what, rc)

    for B, K, A, what in ((0, 8, 4, "batch 0"), (65537, 1, 1, "batch 65537"), (4, 0, 4, "K 0"), (4, 513, 4, "K 513"), (4, 8, 0, "A 0"), (4, 8, 65, "A 65")):
        refuse("sample " + what, lib.dra_policy_heads_sample, P(x), P(w0), P(b0), P(w1), P(b1), P(u), B, K, A, P(oa), P(o[0]), P(o[1]), P(o[2]), P(o[3]), sp())
        refuse("given " + what, lib.dra_policy_heads_given, P(x), P(w0), P(b0), P(w1), P(b1), P(act), B, K, A, P(o[0]), P(o[1]), P(o[2]), P(o[3]), sp())
        if "A" not in what:
            refuse("fwd_pair " + what, lib.dra_linear_fwd_pair, P(x), P(w0), P(b0), P(o[0]), 1, P(w1), P(b1), P(o[1]), 1, B, K, 0, sp())
        if "K" not in what:
            refuse("given_fold " + what, lib.dra_policy_heads_given_fold, P(x), 8, P(b0), P(w0), P(b0), P(w1), P(b1), P(act), B, A, P(o[0]), P(o[1]),
                   P(o[2]), P(o[3]), P(o[4]), sp())
            refuse("sample_fold28 " + what, lib.dra_policy_heads_sample_fold28, P(x), P(b0), P(w0), P(b0), P(w1), P(b1), P(u), B, A, P(oa), P(o[0]),
                   P(o[1]), P(o[2]), sp())
    refuse("fwd_pair out0 0", lib.dra_linear_fwd_pair, P(x), P(w0), P(b0), P(o[0]), 0, P(w1), P(b1), P(o[1]), 1, 4, 8, 0, sp())
    refuse("fwd_pair out1 0", lib.dra_linear_fwd_pair, P(x), P(w0), P(b0), P(o[0]), 1, P(w1), P(b1), P(o[1]), 0, 4, 8, 0, sp())
    for B, K, A, what in ((0, 8, 4, "batch 0"), (8193, 1, 1, "batch 8193"), (4, 0, 4, "K 0"), (4, 513, 4, "K 513"), (4, 8, 0, "A 0"), (4, 8, 65, "A 65")):
        refuse("heads_bwd " + what, lib.dra_policy_heads_bwd, P(x), P(act), P(g), P(g), P(g), P(x), P(w0), P(w1), P(o[0]), P(o[1]), P(o[2]), P(o[3]),
               P(o[4]), B, K, A, 0, sp())
    for B, K, what in ((0, 8, "batch 0"), (4, 0, "K 0"), (4, 513, "K 513")):
        refuse("bwd_pair " + what, lib.dra_linear_bwd_pair, P(g), P(g), P(x), P(w0), P(w1), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), B, K, 4, 1, sp())
    for ks in (0, 7, 9, 13, 15, 28):
        refuse("given_fold n_slabs %d" % ks, lib.dra_policy_heads_given_fold, P(x), ks, P(b0), P(w0), P(b0), P(w1), P(b1), P(act), 2, 4, P(o[0]), P(o[1]),
               P(o[2]), P(o[3]), P(o[4]), sp())

    def nulls(what, fn, args, required):
        """Each required pointer null in turn (the optional ones stay as they are)."""
        for i in required:
            a = list(args)
            a[i] = None
            refuse("%s null argument %d" % (what, i), fn, *a)

    nulls("sample", lib.dra_policy_heads_sample, (P(x), P(w0), P(b0), P(w1), P(b1), P(u), 4, 8, 4, P(oa), P(o[0]), P(o[1]), P(o[2]), P(o[3]), sp()),
          (0, 1, 3, 5, 9, 10, 11, 12))
    nulls("given", lib.dra_policy_heads_given, (P(x), P(w0), P(b0), P(w1), P(b1), P(act), 4, 8, 4, P(o[0]), P(o[1]), P(o[2]), P(o[3]), sp()),
          (0, 1, 3, 5, 9, 10, 11, 12))
    nulls("given_fold", lib.dra_policy_heads_given_fold, (P(x), 8, P(b0), P(w0), P(b0), P(w1), P(b1), P(act), 2, 4, P(o[0]), P(o[1]), P(o[2]), P(o[3]),
                                                         P(o[4]), sp()), (0, 2, 3, 5, 7, 10, 11, 12, 13, 14))
    nulls("sample_fold28", lib.dra_policy_heads_sample_fold28, (P(x), P(b0), P(w0), P(b0), P(w1), P(b1), P(u), 2, 4, P(oa), P(o[0]), P(o[1]), P(o[2]), sp()),
          (0, 1, 2, 4, 6, 9, 10, 11, 12))
    nulls("fwd_pair", lib.dra_linear_fwd_pair, (P(x), P(w0), P(b0), P(o[0]), 1, P(w1), P(b1), P(o[1]), 1, 4, 8, 0, sp()), (0, 1, 3, 5, 7))
    nulls("heads_bwd", lib.dra_policy_heads_bwd, (P(x), P(act), P(g), P(g), P(g), P(x), P(w0), P(w1), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), 4, 8, 4,
                                                  0, sp()), (0, 1, 5, 6, 7, 9, 10, 11, 12))
    nulls("bwd_pair", lib.dra_linear_bwd_pair, (P(g), P(g), P(x), P(w0), P(w1), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), 4, 8, 4, 1, sp()),
          (0, 1, 2, 3, 4, 6, 7, 8, 9))
    # the riding launch: batch 4097, out_phi without fold_bias, and its required pointers (the head's only with a head)
    ride = (P(frames), P(w0), P(b0), P(o[5]), 1, 1.0 / 255.0, P(x), P(b1), P(w0), P(b0), P(w1), P(b1), P(u), 4, P(oa), P(o[0]), P(o[1]), P(o[2]), P(o[3]), sp())
    for B in (0, 4097):
        a = list(ride)
        a[4] = B
        refuse("riding batch %d" % B, lib.dra_rollout_conv1_heads_phi, *a)
    a = list(ride)
    a[7] = None
    refuse("riding out_phi without fold_bias", lib.dra_rollout_conv1_heads_phi, *a)
    a[6] = None
    refuse("riding out_phi without phi_prev", lib.dra_rollout_conv1_heads_phi, *a)
    for A in (0, 65):
        a = list(ride)
        a[13] = A
        refuse("riding A %d" % A, lib.dra_rollout_conv1_heads_phi, *a)
    nulls("riding", lib.dra_rollout_conv1_heads_phi, ride[:18] + (None, sp()), (0, 1, 2, 3, 8, 10, 12, 14, 15, 16, 17))
    _sync()
    assert len(calls) == len(set(calls)) and len(calls) >= 100
    for b in o + [oa]:
        b.all_guard("an output of a refused call")
    for b in (x, w0, b0, w1, b1, u, g, act, frames):
        b.unchanged("an input of a refused call")
