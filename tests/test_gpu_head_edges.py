"""Edge-shape parity of the n-step DQN, option-critic and Rainbow kernels against float64 references, at the shapes where their
code paths change: dra_nstep_q_loss_bwd and dra_oc_loss_bwd up to their 2048 rows (second trips of the environment loop and of
the ballot compaction, row lists of 0 .. 2048 rows, short last four-row groups, one action / one option), the noisy layer's
column, MFMA and scalar kernels (ragged passes, half-filled K chunks, clamped rows, operands at a 4-byte offset, the workspace
contract), the dueling combination with a ragged last workgroup, the PER weights of 1 .. 1024 rows, the Gaussian head of
a2c_continuous, and the rollout heads (dra_q_heads_fold28 / dra_oc_heads_fold28 and their riders in conv1's launch) at every
output count around a chunk of eight and a round of four waves.

Cases, references and the bar live in tests/head_edge_cases.py; tests/test_head_edge_cases_host.py proves on the CPU that the
inputs carry the bar and reach the paths they are named for.  Every check holds
  continuous   max |got - want64| <= 1e-5 * max |want64| per output tensor; exactly zero where float64 is; every measured
               error / scale goes to the parity log (tools/parity_summary.py sums it up)
  discrete     equal to the decision rule applied to the kernel's own float32 scores (np.argmax; the inverse CDF in the
               kernel's float32 order); a row may be left out only within 1e-6 of a boundary in cumulative probability, at most
               1 % of a case's rows, none in the exact cases
  outputs      NaN before the launch, finite after it; guard words around every output keep their bits
  determinism  a second launch gives the same bits"""
import ctypes

import numpy as np
import pytest
import torch

import head_edge_cases as H
from parity_log import record_parity

pytestmark = pytest.mark.gpu

GUARD = 32
EINVAL = -22


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    from deeprl_amd.support import select_device, Config
    select_device(0)
    return Config.DEVICE


@pytest.fixture(scope="module")
def dra(dev):
    import deeprl_amd as d
    return d


def _ids(cases):
    return [c["name"] for c in cases]


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[x.dtype.itemsize])


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


class _Out:
    """A NaN-filled float32 output of `shape` at `offset` floats into a buffer with GUARD NaN words behind it."""

    def __init__(self, shape, dev, offset=0, values=None):
        self.n, self.offset = int(np.prod(shape)), offset
        self.whole = torch.full((offset + self.n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.t = self.whole[offset:offset + self.n].view(*shape)
        if values is not None:
            self.t.copy_(_T(np.asarray(values, dtype=np.float32), dev).view(*shape))

    def np(self):
        return self.t.detach().cpu().numpy().copy()

    def guards_ok(self, what):
        w = self.whole.detach().cpu().numpy()
        out = np.concatenate([w[:self.offset], w[self.offset + self.n:]])
        assert np.all(_bits(out) == _bits(np.float32("nan"))), what + ": written outside the output"

    def untouched(self, what):
        assert np.all(_bits(self.whole) == _bits(np.float32("nan"))), what + ": written by a refused call"


def _close(kernel, case, what, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    got = got.reshape(want.shape)
    assert np.all(np.isfinite(got)), "%s[%s] %s: non-finite output" % (kernel, case, what)
    scale = np.abs(want).max() if want.size else 0.0
    if scale == 0.0:
        print("%s[%s] %s: float64 is exactly zero" % (kernel, case, what))
        assert np.all(got == 0.0), "%s[%s] %s: float64 says exactly zero, the kernel wrote %r" % (kernel, case, what, np.abs(got).max())
        return
    err = np.abs(got - want).max()
    print("%s[%s] %s: err/scale %.3g (bar %.1g), scale %.3g" % (kernel, case, what, err / scale, H.BAR, scale))
    record_parity("head_edges %s.%s[%s]" % (kernel, what, case), err_over_scale=err / scale, scale=scale)
    assert err <= H.BAR * scale, "%s[%s] %s: max abs err %.3e vs scale %.3e (%.2e of it, bar %.0e)" % (
        kernel, case, what, err, scale, err / scale, H.BAR)


def _close_all(kernel, case, got, want):
    for k, w in want.items():
        _close(kernel, case, k, got[k], w)


# ------------------------------------------------------------------------------------------------ dra_nstep_q_loss_bwd
def _nstep_outs(c, dev):
    return dict(ret=_Out((c["T"], c["N"]), dev), loss=_Out((1,), dev), dw=_Out((c["A"], 512), dev), db=_Out((c["A"],), dev),
                dphi=_Out((c["R"], 512), dev))


def _run_nstep(c, dev, ops):
    outs = _nstep_outs(c, dev)
    ops.nstep_q_loss_bwd(_T(c["q"], dev), _T(c["action"], dev), _T(c["reward"], dev), _T(c["mask"], dev), _T(c["boot"], dev), c["gamma"],
                         _T(c["phi"], dev), _T(c["w"], dev), out={k: o.t for k, o in outs.items()})
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.guards_ok("nstep_q_loss_bwd[%s] %s" % (c["name"], k))
    return {k: o.np() for k, o in outs.items()}


@pytest.mark.parametrize("c", H.nstep_cases(), ids=_ids(H.nstep_cases()))
def test_nstep_q_loss_bwd_edges(dra, dev, c):
    got = _run_nstep(c, dev, dra.ops)
    _close_all("nstep_q_loss_bwd", c["name"], got, H.nstep_ref(c))
    assert np.all(got["dphi"][c["phi"] == 0] == 0), "dphi is not exactly zero where phi is +0 / -0"
    if c["unused"] is not None:
        assert not got["dw"][c["unused"]].any() and got["db"][c["unused"]] == 0, "an action no row took has a gradient"
    again = _run_nstep(c, dev, dra.ops)
    for k in got:
        _same(again[k], got[k], "nstep_q_loss_bwd[%s]: second run differs in %s" % (c["name"], k))


def test_nstep_q_loss_bwd_limits_are_refused(dra, dev):
    from deeprl_amd._lib import DraError, lib, ptr, stream_ptr
    big = dict(T=1, N=2049, A=65, R=2049)                     # buffers large enough for every call below
    outs = _nstep_outs(big, dev)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    q, act, rew, msk, boot, phi, w = z(2049 * 65), z(2049, dt=torch.int64), z(2049), z(2049), z(2049), z(2049, 512), z(65, 512)

    def raw(t_len, n, a):
        return lib.dra_nstep_q_loss_bwd.raw(ptr(q), ptr(act), ptr(rew), ptr(msk), ptr(boot), 0.99, ptr(phi), ptr(w), t_len, n, a,
                                            *[ptr(outs[k].t) for k in ("ret", "loss", "dw", "db", "dphi")], stream_ptr())

    refused = {"R = 2049": raw(1, 2049, 2), "R = 2049 (T = 2049)": raw(2049, 1, 2), "A = 0": raw(2, 4, 0), "A = 65": raw(2, 4, 65),
               "T = 0": raw(0, 4, 2), "N = 0": raw(4, 0, 2)}
    for t_len, n, a in ((1, 2049, 2), (2, 4, 65), (2, 4, 0), (0, 4, 2)):         # the wrapper's error, on views of the same buffers
        rows = t_len * n
        with pytest.raises(DraError):
            dra.ops.nstep_q_loss_bwd(q[:rows * a].view(t_len, n, a), act[:rows].view(t_len, n), rew[:rows], msk[:rows], boot[:n], 0.99,
                                     phi[:rows], w[:a], out=dict(ret=outs["ret"].t.view(-1)[:rows], loss=outs["loss"].t, dw=outs["dw"].t[:a],
                                                                 db=outs["db"].t[:a], dphi=outs["dphi"].t[:rows]))
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in refused.values()), refused
    for k, o in outs.items():
        o.untouched("nstep_q_loss_bwd " + k)


# ----------------------------------------------------------------------------------------------------- dra_oc_loss_bwd
_OC_SHAPES = lambda c: dict(ret=(c["T"], c["N"]), adv=(c["T"], c["N"]), beta_adv=(c["T"], c["N"]), loss=(4,), dw_q=(c["O"], 512),
                            db_q=(c["O"],), dw_pi=(c["O"] * c["A"], 512), db_pi=(c["O"] * c["A"],), dw_beta=(c["O"], 512),
                            db_beta=(c["O"],), dphi=(c["R"], 512))


def _run_oc(c, dev, ops):
    outs = {k: _Out(s, dev) for k, s in _OC_SHAPES(c).items()}
    roll = dict(q=c["q"], beta=c["beta"], logits=c["logits"], option=c["option"], action=c["action"], prev_option=c["prev"],
                init=c["init"], log_pi_a=c["log_pi_a"], entropy=c["entropy"])
    ops.oc_loss_bwd({k: _T(v, dev) for k, v in roll.items()}, _T(c["reward"], dev), _T(c["mask"], dev), _T(c["boot"], dev),
                    _T(c["eps"], dev), c["gamma"], c["term_reg"], c["ent_w"], _T(c["phi"], dev), _T(c["wq"], dev), _T(c["wp"], dev),
                    _T(c["wb"], dev), out={k: o.t for k, o in outs.items()})
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.guards_ok("oc_loss_bwd[%s] %s" % (c["name"], k))
    return {k: o.np() for k, o in outs.items()}


@pytest.mark.parametrize("c", H.oc_cases(), ids=_ids(H.oc_cases()))
def test_oc_loss_bwd_edges(dra, dev, c):
    got = _run_oc(c, dev, dra.ops)
    want = H.oc_ref(c)
    _close_all("oc_loss_bwd", c["name"], got, want)
    assert np.all(got["dphi"][c["phi"] == 0] == 0), "dphi is not exactly zero where phi is +0 / -0"
    if c["variant"] == "init1":
        assert got["loss"][3] == 0 and not got["dw_beta"].any() and not got["db_beta"].any(), "init all 1: the beta head has a gradient"
    path = H.oc_path(c)
    for o in np.nonzero(path["by_option"] == 0)[0]:           # a list of length 0: the rows are still written, as zeros
        assert not got["dw_q"][o].any() and got["db_q"][o] == 0 and not got["dw_pi"][o * c["A"]:(o + 1) * c["A"]].any()
    for o in np.nonzero(path["by_prev"] == 0)[0]:
        assert not got["dw_beta"][o].any() and got["db_beta"][o] == 0
    again = _run_oc(c, dev, dra.ops)
    for k in got:
        _same(again[k], got[k], "oc_loss_bwd[%s]: second run differs in %s" % (c["name"], k))


def test_oc_loss_bwd_limits_are_refused(dra, dev):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    big = dict(T=1, N=2049, O=9, A=19, R=2049)
    outs = {k: _Out(s, dev) for k, s in _OC_SHAPES(big).items()}
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    f = {k: z(2049 * 19) for k in ("q", "beta", "logits", "init", "lp", "ent", "rew", "msk", "boot", "eps")}
    i = {k: z(2049, dt=torch.int64) for k in ("option", "action", "prev")}
    phi, wq, wp, wb = z(2049, 512), z(9, 512), z(9 * 19, 512), z(9, 512)

    def raw(t_len, n, o, a):
        return lib.dra_oc_loss_bwd.raw(ptr(f["q"]), ptr(f["beta"]), ptr(f["logits"]), ptr(i["option"]), ptr(i["action"]), ptr(i["prev"]),
                                       ptr(f["init"]), ptr(f["lp"]), ptr(f["ent"]), ptr(f["rew"]), ptr(f["msk"]), ptr(f["boot"]),
                                       ptr(f["eps"]), 0.99, 0.01, 0.01, ptr(phi), ptr(wq), ptr(wp), ptr(wb), t_len, n, o, a,
                                       *[ptr(outs[k].t) for k in dra.ops._OC_LOSS_OUTS], stream_ptr())

    refused = {"R = 2049": raw(1, 2049, 2, 2), "R = 2049 (T = 2049)": raw(2049, 1, 2, 2), "O = 9": raw(2, 4, 9, 2), "O = 0": raw(2, 4, 0, 2),
               "A = 19": raw(2, 4, 2, 19), "A = 0": raw(2, 4, 2, 0), "T = 0": raw(0, 4, 2, 2)}

    def wrapper(t_len, n, o, a):
        rows = t_len * n
        roll = dict(q=f["q"][:rows * o].view(t_len, n, o), beta=f["beta"][:rows * o].view(t_len, n, o),
                    logits=f["logits"][:rows * a].view(t_len, n, a), option=i["option"][:rows], action=i["action"][:rows],
                    prev_option=i["prev"][:rows], init=f["init"][:rows], log_pi_a=f["lp"][:rows], entropy=f["ent"][:rows])
        shapes = _OC_SHAPES(dict(T=t_len, N=n, O=o, A=a, R=rows))
        with pytest.raises(ValueError):
            dra.ops.oc_loss_bwd(roll, f["rew"][:rows], f["msk"][:rows], f["boot"][:n], f["eps"][:t_len], 0.99, 0.01, 0.01, phi[:rows],
                                wq[:o], wp[:o * a], wb[:o], out={k: outs[k].t.view(-1)[:int(np.prod(s))].view(*s) for k, s in shapes.items()})

    wrapper(1, 2049, 2, 2), wrapper(2, 4, 9, 2), wrapper(2, 4, 2, 19)
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in refused.values()), refused
    for k, o in outs.items():
        o.untouched("oc_loss_bwd " + k)


# ---------------------------------------------------------------------------------------- dueling over atoms, PER weights
def _run_dueling(c, dev):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    b, a, z = c["B"], c["A"], c["Z"]
    outs = dict(logits=_Out((b, a, z), dev), d_value=_Out((b, z), dev), d_adv=_Out((b, a, z), dev))
    value, adv, g = _T(c["value"], dev), _T(c["adv"], dev), _T(c["g"], dev)
    lib.dra_dueling_atoms_fwd(ptr(value), ptr(adv), b, a, z, ptr(outs["logits"].t), stream_ptr())
    lib.dra_dueling_atoms_bwd(ptr(g), b, a, z, ptr(outs["d_value"].t), ptr(outs["d_adv"].t), stream_ptr())
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.guards_ok("dueling_atoms[%s] %s" % (c["name"], k))
    return {k: o.np() for k, o in outs.items()}


@pytest.mark.parametrize("c", H.dueling_cases(), ids=_ids(H.dueling_cases()))
def test_dueling_atoms_edges(dra, dev, c):
    got = _run_dueling(c, dev)
    _close_all("dueling_atoms", c["name"], got, H.dueling_ref(c))
    if c["A"] == 1:
        _same(got["logits"][:, 0], c["value"], "one action: the logits are not the value")
    wrapped = dra.ops.dueling_atoms_fwd(_T(c["value"], dev), _T(c["adv"], dev)), dra.ops.dueling_atoms_bwd(_T(c["g"], dev))
    _same(wrapped[0], got["logits"], "ops.dueling_atoms_fwd")
    _same(wrapped[1][0], got["d_value"], "ops.dueling_atoms_bwd d_value")
    _same(wrapped[1][1], got["d_adv"], "ops.dueling_atoms_bwd d_advantage")
    again = _run_dueling(c, dev)
    for k in got:
        _same(again[k], got[k], "dueling_atoms[%s]: second run differs in %s" % (c["name"], k))


def _run_per(c, dev, with_loss=True):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    outs = dict(prio=_Out((c["B"],), dev), w=_Out((c["B"],), dev))
    beta_dev = torch.tensor([c["beta"]], dtype=torch.float32, device=dev)
    loss_vec, sp = _T(c["loss_vec"], dev), _T(c["sp"], dev)
    lib.dra_per_weights_dev(ptr(loss_vec) if with_loss else None, ptr(sp), c["B"], ptr(beta_dev), c["eps"],
                            c["alpha"], ptr(outs["prio"].t), ptr(outs["w"].t), stream_ptr())
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.guards_ok("per_weights_dev[%s] %s" % (c["name"], k))
    return {k: o.np() for k, o in outs.items()}


@pytest.mark.parametrize("c", H.per_cases(), ids=_ids(H.per_cases()))
def test_per_weights_dev_edges(dra, dev, c):
    got = _run_per(c, dev)
    _close_all("per_weights_dev", c["name"], got, H.per_ref(c))
    assert got["w"].max() == 1.0 and got["w"][c["argmax"]] == 1.0, "the largest weight is not exactly one"
    prio, w = dra.ops.per_weights(_T(c["loss_vec"], dev), _T(c["sp"], dev), c["beta"], c["eps"], c["alpha"])
    _same(prio, got["prio"], "per_weights_dev differs from per_weights in the priorities")
    _same(w, got["w"], "per_weights_dev differs from per_weights in the weights")
    prio2, w2 = dra.ops.per_weights_dev(_T(c["loss_vec"], dev), _T(c["sp"], dev), torch.tensor([c["beta"]], device=dev), c["eps"], c["alpha"])
    _same(prio2, got["prio"], "ops.per_weights_dev priorities")
    _same(w2, got["w"], "ops.per_weights_dev weights")
    none = _run_per(c, dev, with_loss=False)                 # loss_vec None: the weights alone, no priority written
    _same(none["w"], got["w"], "loss_vec = None changes the weights")
    assert np.all(np.isnan(none["prio"])), "priorities written without a loss vector"
    again = _run_per(c, dev)
    for k in got:
        _same(again[k], got[k], "per_weights_dev[%s]: second run differs in %s" % (c["name"], k))


def test_per_weights_dev_limits_are_refused(dev):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    outs = dict(prio=_Out((1025,), dev), w=_Out((1025,), dev))
    x, beta_dev = torch.ones(1025, device=dev), torch.ones(1, device=dev)
    rcs = [lib.dra_per_weights_dev.raw(ptr(x), ptr(x), b, bd, 0.01, 0.5, ptr(outs["prio"].t), ptr(outs["w"].t), stream_ptr())
           for b, bd in ((0, ptr(beta_dev)), (1025, ptr(beta_dev)), (-1, ptr(beta_dev)), (32, None))]
    torch.cuda.synchronize()
    assert rcs == [EINVAL] * 4, rcs
    for k, o in outs.items():
        o.untouched("per_weights_dev " + k)


# ------------------------------------------------------------------------------------------------------- noisy layers
class _In:
    """A float32 operand at `offset` floats into its own buffer (offset 0: 16-byte aligned, as torch allocates)."""

    def __init__(self, values, dev, offset=0):
        values = np.ascontiguousarray(values, dtype=np.float32)
        self.whole = torch.zeros(offset + values.size + 4, dtype=torch.float32, device=dev)
        self.t = self.whole[offset:offset + values.size].view(*values.shape)
        self.t.copy_(_T(values, dev))
        assert self.t.data_ptr() % 16 == 4 * (offset % 4) and self.t.is_contiguous()


def _workspace(floats, dev, short=0):
    """Exactly `floats` - `short` floats of workspace (NaN) with guard words behind; None for no workspace at all."""
    return _Out((max(0, floats - short),), dev) if floats > 0 else None


def _noisy_fwd(c, act, dev, offset=0, noise_offsets=(0, 0, 0), ws_short=0):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, ptr, stream_ptr
    rows, k, n = c["rows"], c["K"], c["N"]
    x, wm, ws_ = (_In(c[key], dev, offset) for key in ("x", "w_mu", "w_sigma"))
    e_in, e_out, e_b = (_In(c[key], dev, o) for key, o in zip(("e_in", "e_out", "e_b"), noise_offsets))
    y = _Out((rows, n), dev)
    work = _workspace(H.noisy_workspace(rows, k, n)[0], dev, ws_short)
    b_mu, b_sigma = _T(c["b_mu"], dev), _T(c["b_sigma"], dev)
    rc = lib.dra_noisy_linear_fwd.raw(ptr(x.t), ptr(wm.t), ptr(ws_.t), ptr(b_mu), ptr(b_sigma), ptr(e_in.t),
                                      ptr(e_out.t), ptr(e_b.t), ptr(y.t), rows, k, n, ops.ACT[act], ptr(work.t) if work else None,
                                      work.n if work else 0, stream_ptr())
    torch.cuda.synchronize()
    y.guards_ok("noisy_linear_fwd[%s] y" % c["name"])
    if work:
        work.guards_ok("noisy_linear_fwd[%s] workspace" % c["name"])
    return rc, y, work


def _noisy_bwd(c, dev, offset=0, noise_offsets=(0, 0, 0), want_dx=True, x_relu=False, dx_add=False, ws_short=0, want_dw=True):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    rows, k, n = c["rows"], c["K"], c["N"]
    x, wm, ws_ = (_In(c[key], dev, offset) for key in ("x", "w_mu", "w_sigma"))
    e_in, e_out, e_b = (_In(c[key], dev, o) for key, o in zip(("e_in", "e_out", "e_b"), noise_offsets))
    outs = dict(dw_mu=_Out((n, k), dev, offset), dw_sigma=_Out((n, k), dev, offset), db_mu=_Out((n,), dev), db_sigma=_Out((n,), dev),
                dx=_Out((rows, k), dev))
    work = _workspace(H.noisy_workspace(rows, k, n)[1], dev, ws_short)
    p = lambda key, on=True: ptr(outs[key].t) if on else None
    g, add = _T(c["g"], dev), _T(c["dx_add"], dev)
    rc = lib.dra_noisy_linear_bwd.raw(ptr(g), ptr(x.t), ptr(wm.t), ptr(ws_.t), ptr(e_in.t), ptr(e_out.t), ptr(e_b.t),
                                      ptr(x.t) if x_relu else None, ptr(add) if dx_add else None, p("dw_mu", want_dw),
                                      p("dw_sigma", want_dw), p("db_mu", want_dw), p("db_sigma", want_dw), p("dx", want_dx), rows, k, n,
                                      ptr(work.t) if work else None, work.n if work else 0, stream_ptr())
    torch.cuda.synchronize()
    for key, o in outs.items():
        o.guards_ok("noisy_linear_bwd[%s] %s" % (c["name"], key))
    if work:
        work.guards_ok("noisy_linear_bwd[%s] workspace" % c["name"])
    return rc, outs, work


_NOISY_GRADS = ("dw_mu", "dw_sigma", "db_mu", "db_sigma", "dx")


@pytest.mark.parametrize("c", H.noisy_cases(), ids=_ids(H.noisy_cases()))
def test_noisy_linear_shape_edges(dev, c):
    """The shape table through the C ABI, the workspace sized to exactly what dra_noisy_workspace_floats reports."""
    from deeprl_amd._lib import lib
    f, b = ctypes.c_int64(0), ctypes.c_int64(0)
    lib.dra_noisy_workspace_floats(c["rows"], c["K"], c["N"], ctypes.byref(f), ctypes.byref(b))
    assert (f.value, b.value) == H.noisy_workspace(c["rows"], c["K"], c["N"])
    path = H.noisy_path(c["rows"], c["K"], c["N"])
    for act in H.NOISY_ACTS:
        want = H.noisy_ref(c, act)
        rc, y, _ = _noisy_fwd(c, act, dev)
        assert rc == 0
        _close("noisy_linear_fwd", "%s %s" % (c["name"], act), "y", y.np(), want["y"])
        rc2, y2, _ = _noisy_fwd(c, act, dev)
        _same(y2.np(), y.np(), "noisy_linear_fwd[%s %s]: second run differs" % (c["name"], act))
    rc, outs, _ = _noisy_bwd(c, dev)
    assert rc == 0
    got = {k: outs[k].np() for k in _NOISY_GRADS}
    _close_all("noisy_linear_bwd", c["name"], got, {k: want[k] for k in _NOISY_GRADS})
    _, outs2, _ = _noisy_bwd(c, dev)
    for k in _NOISY_GRADS:
        _same(outs2[k].np(), got[k], "noisy_linear_bwd[%s]: second run differs in %s" % (c["name"], k))
    # one float less of workspace: refused where the launch uses it, and nothing written
    if path["fwd"].startswith("mfma"):
        rc, y, work = _noisy_fwd(c, "none", dev, ws_short=1)
        assert rc == EINVAL
        y.untouched("noisy_linear_fwd y"), work.untouched("noisy_linear_fwd workspace")
    if path["bwd_x"] == "mfma":
        rc, outs, work = _noisy_bwd(c, dev, ws_short=1)       # every output requested: the parameter gradients stay NaN too
        assert rc == EINVAL
        work.untouched("noisy_linear_bwd workspace")
        for k in _NOISY_GRADS:
            outs[k].untouched("noisy_linear_bwd " + k)


@pytest.mark.parametrize("shape", H.NOISY_OFFSET_SHAPES, ids=lambda s: "rows%d-K%d-N%d" % s)
def test_noisy_linear_offset_views_and_variants(dra, dev, shape):
    """K % 4 == 0 with x / w_mu / w_sigma / dw_* one float into a buffer (the parameters are views into a flat buffer): the
    scalar kernels through alignment; the noise vectors at 1, 2 and 3 floats; the optional pieces of the backward."""
    c = H.noisy_case(shape)
    name = c["name"]
    for act in H.NOISY_ACTS:
        want = H.noisy_ref(c, act)
        for tag, off, noff in (("offset1", 1, (0, 0, 0)), ("noise-offsets", 0, (1, 2, 3)), ("offset1+noise-offsets", 1, (3, 1, 2))):
            rc, y, _ = _noisy_fwd(c, act, dev, offset=off, noise_offsets=noff)
            assert rc == 0
            _close("noisy_linear_fwd", "%s %s %s" % (name, act, tag), "y", y.np(), want["y"])
    for tag, off, noff in (("offset1", 1, (0, 0, 0)), ("noise-offsets", 0, (1, 2, 3)), ("offset1+noise-offsets", 1, (3, 1, 2))):
        rc, outs, _ = _noisy_bwd(c, dev, offset=off, noise_offsets=noff)
        assert rc == 0
        _close_all("noisy_linear_bwd", "%s %s" % (name, tag), {k: outs[k].np() for k in _NOISY_GRADS}, {k: want[k] for k in _NOISY_GRADS})
    rc, base, _ = _noisy_bwd(c, dev)
    for x_relu in (False, True):
        for dx_add in (False, True):
            rc, outs, _ = _noisy_bwd(c, dev, x_relu=x_relu, dx_add=dx_add)
            assert rc == 0
            _close("noisy_linear_bwd", "%s x_relu=%d dx_add=%d" % (name, x_relu, dx_add), "dx", outs["dx"].np(),
                   H.noisy_ref(c, "none", x_relu=x_relu, dx_add=dx_add)["dx"])
            if x_relu:
                assert np.all(outs["dx"].np()[c["x"] <= 0] == 0)
            for k in _NOISY_GRADS[:4]:
                _same(outs[k].np(), base[k].np(), "the dx options changed " + k)
    # the same options on the scalar kernels (noisy_bwd_x_any_kernel, noisy_bwd_w_kernel<1>): every operand one float in
    rc, off1, _ = _noisy_bwd(c, dev, offset=1)
    for x_relu, dx_add in ((True, True), (True, False), (False, True)):
        rc, outs, _ = _noisy_bwd(c, dev, offset=1, noise_offsets=(1, 2, 3), x_relu=x_relu, dx_add=dx_add)
        assert rc == 0
        _close("noisy_linear_bwd", "%s offset1 x_relu=%d dx_add=%d" % (name, x_relu, dx_add), "dx", outs["dx"].np(),
               H.noisy_ref(c, "none", x_relu=x_relu, dx_add=dx_add)["dx"])
        if x_relu:
            assert np.all(outs["dx"].np()[c["x"] <= 0] == 0)
        for k in _NOISY_GRADS[:4]:
            _same(outs[k].np(), off1[k].np(), "offset 1: the dx options changed " + k)
    for kw in (dict(want_dx=False), dict(want_dw=False)):
        rc, outs, _ = _noisy_bwd(c, dev, offset=1, **kw)
        asked = _NOISY_GRADS[:4] if "want_dx" in kw else _NOISY_GRADS[4:]
        assert rc == 0 and all(np.all(np.isnan(outs[k].np())) for k in _NOISY_GRADS if k not in asked), "offset 1: an output nobody asked for"
        for k in asked:
            _same(outs[k].np(), off1[k].np(), "offset 1, %s: %s differs" % (kw, k))
    rc, outs, _ = _noisy_bwd(c, dev, want_dx=False)
    assert rc == 0 and np.all(np.isnan(outs["dx"].np())), "want_dx = False wrote dx"
    for k in _NOISY_GRADS[:4]:
        _same(outs[k].np(), base[k].np(), "want_dx = False changed " + k)
    rc, outs, _ = _noisy_bwd(c, dev, want_dw=False)
    assert rc == 0 and all(np.all(np.isnan(outs[k].np())) for k in _NOISY_GRADS[:4]), "parameter gradients written without being asked for"
    _same(outs["dx"].np(), base["dx"].np(), "dx without the parameter gradients differs")
    # the wrappers give the bits of the raw launches
    t = {k: _T(c[k], dev) for k in ("x", "w_mu", "w_sigma", "b_mu", "b_sigma", "e_in", "e_out", "e_b", "g")}
    y = dra.ops.noisy_linear_fwd(t["x"], t["w_mu"], t["w_sigma"], t["b_mu"], t["b_sigma"], t["e_in"], t["e_out"], t["e_b"], act="relu")
    _same(y, _noisy_fwd(c, "relu", dev)[1].np(), "ops.noisy_linear_fwd")
    for k, v in zip(("dx",) + _NOISY_GRADS[:4], dra.ops.noisy_linear_bwd(t["g"], t["x"], t["w_mu"], t["w_sigma"], t["e_in"], t["e_out"], t["e_b"])):
        _same(v, base[k].np(), "ops.noisy_linear_bwd " + k)
    # noise all +0 / -0: the plain linear layer, and no gradient for the sigmas
    z = H.noisy_case(shape, zero_noise=True)
    wz = H.noisy_ref(z, "none")
    for off in (0, 1):
        rc, y, _ = _noisy_fwd(z, "none", dev, offset=off)
        _close("noisy_linear_fwd", "%s offset%d" % (z["name"], off), "y", y.np(), wz["plain"])
        rc, outs, _ = _noisy_bwd(z, dev, offset=off)
        assert not outs["dw_sigma"].np().any() and not outs["db_sigma"].np().any(), "zero noise: the sigmas have a gradient"
        _close_all("noisy_linear_bwd", "%s offset%d" % (z["name"], off), {k: outs[k].np() for k in ("dw_mu", "db_mu", "dx")},
                   {k: wz[k] for k in ("dw_mu", "db_mu", "dx")})


def test_noisy_linear_limits_are_refused(dev):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    rows, k, n = 1025, 8, 8
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    x, w, e, g = z(rows, k), z(n, k), z(8), z(rows, n)
    outs = dict(y=_Out((rows, n), dev), dw_mu=_Out((n, k), dev), dw_sigma=_Out((n, k), dev), db_mu=_Out((n,), dev),
                db_sigma=_Out((n,), dev), dx=_Out((rows, k), dev), ws=_Out((4 * rows * k,), dev))
    o = lambda key: ptr(outs[key].t)

    def fwd(r, act):
        return lib.dra_noisy_linear_fwd.raw(ptr(x), ptr(w), ptr(w), ptr(e), ptr(e), ptr(e), ptr(e), ptr(e), o("y"), r, k, n, act, o("ws"),
                                            outs["ws"].n, stream_ptr())

    def bwd(r, dw_mu="dw_mu", dw_sigma="dw_sigma", db_mu="db_mu", db_sigma="db_sigma"):
        q = lambda key: o(key) if key else None
        return lib.dra_noisy_linear_bwd.raw(ptr(g), ptr(x), ptr(w), ptr(w), ptr(e), ptr(e), ptr(e), None, None, q(dw_mu), q(dw_sigma),
                                            q(db_mu), q(db_sigma), o("dx"), r, k, n, o("ws"), outs["ws"].n, stream_ptr())

    refused = {"fwd rows 0": fwd(0, 0), "fwd rows 1025": fwd(1025, 0), "fwd act tanh": fwd(8, 2), "fwd act 7": fwd(8, 7), "fwd act -1": fwd(8, -1),
               "bwd rows 0": bwd(0), "bwd rows 1025": bwd(1025), "bwd dw_mu without dw_sigma": bwd(8, dw_sigma=None),
               "bwd dw_sigma without dw_mu": bwd(8, dw_mu=None), "bwd db_mu without db_sigma": bwd(8, db_sigma=None),
               "bwd db_sigma without db_mu": bwd(8, db_mu=None), "bwd biases without weights": bwd(8, dw_mu=None, dw_sigma=None)}
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in refused.values()), refused
    for key, out in outs.items():
        out.untouched("noisy_linear " + key)


# ------------------------------------------------------------------------------------------------- the rollout heads
class _IOut:
    """An int64 output prefilled with a value no head writes, with guard words behind."""
    FILL = -(2 ** 62) - 12345

    def __init__(self, n, dev):
        self.n = n
        self.whole = torch.full((n + GUARD,), self.FILL, dtype=torch.int64, device=dev)
        self.t = self.whole[:n]

    def np(self):
        return self.t.detach().cpu().numpy().copy()

    def guards_ok(self, what):
        assert bool((self.whole[self.n:] == self.FILL).all()), what + ": written outside the output"


@pytest.fixture(scope="module")
def conv1(dev):
    """conv1's operands for the fused launches: 33 frames, the weights in KOC layout, and the plain launch's output."""
    from deeprl_amd import ops
    g = torch.Generator().manual_seed(77)
    frames = torch.randint(0, 256, (33, 4, 84, 84), dtype=torch.uint8, generator=g).to(dev)
    wt1 = (torch.randn(32, 4, 8, 8, generator=g) * 0.05).permute(1, 2, 3, 0).contiguous().to(dev)
    b1 = (torch.randn(32, generator=g) * 0.05).to(dev)
    want = {b: ops.conv_fwd_koc(1, [frames[:b].contiguous()], [wt1], [b1], act="relu", u8_coef=1.0 / 255.0)[0] for b in (1, 3, 5, 33)}
    torch.cuda.synchronize()
    return dict(frames=frames, wt1=wt1, b1=b1, coef=1.0 / 255.0, want=want)


def _opt(x, dev):
    return None if x is None else _T(x, dev)


def _run_q_head(c, dev, ops, conv1=None, only=None):
    """Stand-alone (conv1 None) or in conv1's launch; only: the one output requested (None: all the launch has)."""
    b, a = c["B"], c["A"]
    outs = dict(q=_Out((b, a), dev), action=_IOut(b, dev), phi=_Out((b, 512), dev), max=_Out((b,), dev))
    ask = lambda k: outs[k].t if only in (None, k) else None
    args = (_T(c["slabs"], dev), _T(c["fold_bias"], dev), _T(c["w"], dev), _opt(c["b"], dev), _T(c["explore"], dev), _T(c["random_action"], dev))
    if conv1 is None:
        ops.q_heads_fold28(*args, out_q=ask("q"), out_action=ask("action"), out_phi=ask("phi"), out_max=ask("max"))
    else:
        y1 = _Out((b, 32, 20, 20), dev)
        ops.rollout_conv1_qheads(conv1["frames"][:b].contiguous(), conv1["wt1"], conv1["b1"], y1.t, conv1["coef"], *args,
                                 out_q=outs["q"].t, out_action=outs["action"].t, out_phi=outs["phi"].t)
        torch.cuda.synchronize()
        y1.guards_ok("rollout_conv1_qheads[%s] y1" % c["name"])
        _same(y1.t, conv1["want"][b], "rollout_conv1_qheads[%s]: conv1 differs from the plain launch" % c["name"])
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.guards_ok("q_heads[%s] %s" % (c["name"], k))
    return {k: o.np() for k, o in outs.items()}


@pytest.mark.parametrize("c", H.q_head_cases(), ids=_ids(H.q_head_cases()))
def test_q_heads_edges(dra, dev, conv1, c):
    got = _run_q_head(c, dev, dra.ops)
    want = H.q_head_ref(c)
    _same(got["phi"], want["phi"], "q_heads_fold28[%s]: phi is not the float32 fold" % c["name"])
    _close("q_heads_fold28", c["name"], "q", got["q"], want["q"])
    dec = H.q_head_decide(c, got["q"])
    assert np.array_equal(got["action"], dec["action"]), (got["action"], dec["action"])
    _same(got["max"], dec["max"], "out_max is not the maximum of the row's q")
    record_parity("head_edges q_heads_fold28.action[%s]" % c["name"], rows=c["B"], exemptable_rows=0, exemptions_used=0)
    if c["winner"] is not None:                               # exact ties at the top: the lowest index wins
        greedy = c["explore"] == 0
        assert all(np.array_equal(got["q"][:, t], got["q"][:, c["winner"]]) for t in c["tied"])
        assert np.all(np.argmax(got["q"], -1) == c["winner"]) and np.all(got["action"][greedy] == c["winner"])
    for only in ("q", "action", "phi", "max"):                # each optional output alone (max alone: the bootstrap use)
        alone = _run_q_head(c, dev, dra.ops, only=only)
        _same(alone[only], got[only], "q_heads_fold28[%s]: %s requested alone differs" % (c["name"], only))
        for k in ("q", "phi", "max"):
            assert k == only or np.all(np.isnan(alone[k])), "%s written without being requested" % k
        assert only == "action" or np.all(alone["action"] == _IOut.FILL)
    fused = _run_q_head(c, dev, dra.ops, conv1=conv1)         # the same head in conv1's launch: bit for bit
    for k in ("q", "action", "phi"):
        _same(fused[k], got[k], "rollout_conv1_qheads[%s]: %s differs from the stand-alone head" % (c["name"], k))
    again = _run_q_head(c, dev, dra.ops)
    for k in got:
        _same(again[k], got[k], "q_heads_fold28[%s]: second run differs in %s" % (c["name"], k))


def test_q_heads_nan_row_follows_np_argmax(dra, dev):
    """One row whose q holds a NaN (an infinite feature against a zero weight) behind a +inf: np.argmax's rule, the first NaN
    wins and is the maximum; the other rows are untouched by it."""
    c = H.q_head_case(9, 3, ties="none", explore="none", bias=True)
    c["slabs"][0, 1, 100] = np.inf
    c["w"][:, 100] = np.abs(c["w"][:, 100]) + F32_TINY
    c["w"][5, 100] = 0.0
    got = _run_q_head(c, dev, dra.ops)
    assert np.isnan(got["q"][1, 5]) and np.all(np.isposinf(np.delete(got["q"][1], 5))) and np.all(np.isfinite(got["q"][[0, 2]]))
    assert got["action"].tolist() == np.argmax(got["q"], -1).tolist() and got["action"][1] == 5 and np.isnan(got["max"][1])
    _same(got["max"][[0, 2]], got["q"][[0, 2]].max(-1), "out_max of the finite rows")


F32_TINY = np.float32(1e-3)

_OC_F = ("q", "beta", "logits", "log_pi_a", "entropy", "init", "phi")
_OC_I = ("option", "action", "prev_option")


def _run_oc_head(c, dev, ops, conv1=None):
    b, n_opt, n_act = c["B"], c["O"], c["A"]
    shapes = dict(q=(b, n_opt), beta=(b, n_opt), logits=(b, n_act), log_pi_a=(b,), entropy=(b,), init=(b,), phi=(b, 512))
    outs = {k: _Out(shapes[k], dev) for k in _OC_F}
    outs.update({k: _IOut(b, dev) for k in _OC_I})
    prev, init = _T(c["prev_option"], dev), _T(c["init"], dev)
    heads = tuple(_opt(c[k], dev) for k in ("wq", "bq", "wb", "bb", "wp", "bp"))
    kw = dict(uniform=_T(c["uniform"], dev), eps=torch.tensor([c["eps"]], dtype=torch.float32, device=dev), mask=_T(c["mask"], dev),
              prev_option=prev, is_initial=init, out={k: o.t for k, o in outs.items()})
    if conv1 is None:
        ops.oc_heads_fold28(_T(c["slabs"], dev), _T(c["fold_bias"], dev), *heads, **kw)
    else:
        y1 = _Out((b, 32, 20, 20), dev)
        ops.rollout_conv1_ocheads(conv1["frames"][:b].contiguous(), conv1["wt1"], conv1["b1"], y1.t, conv1["coef"], _T(c["slabs"], dev),
                                  _T(c["fold_bias"], dev), heads, **kw)
        torch.cuda.synchronize()
        _same(y1.t, conv1["want"][b], "rollout_conv1_ocheads[%s]: conv1 differs from the plain launch" % c["name"])
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.guards_ok("oc_heads[%s] %s" % (c["name"], k))
    got = {k: o.np() for k, o in outs.items()}
    got.update(carried_prev=prev.cpu().numpy(), carried_init=init.cpu().numpy())
    return got


def _check_oc_head(kernel, c, got):
    want = H.oc_head_ref(c)
    rows = np.arange(c["B"])
    _same(got["phi"], want["phi"], "%s[%s]: phi is not the float32 fold" % (kernel, c["name"]))
    _close(kernel, c["name"], "q", got["q"], want["q"])
    _close(kernel, c["name"], "beta", got["beta"], want["beta"])
    # the decisions, from the kernel's own q / beta / logits
    dec = H.oc_head_decide(c, got["q"], got["beta"], lambda r, o: got["logits"][r])
    assert np.array_equal(got["option"], dec["option"]), (got["option"], dec["option"])
    near = dec["margin"] < 1e-6
    record_parity("head_edges %s.action[%s]" % (kernel, c["name"]), rows=c["B"], exemptable_rows=int(near.sum()),
                  exemptions_used=int((got["action"] != dec["action"])[near].sum()))
    assert near.sum() <= 0.01 * c["B"] and not (c["exact"] and near.any()), "%d rows within 1e-6 of a boundary" % near.sum()
    assert np.array_equal(got["action"][~near], dec["action"][~near]), (got["action"], dec["action"])
    # the continuous outputs of the chosen option against float64
    chosen = want["logits"][rows, got["option"]]
    _close(kernel, c["name"], "logits", got["logits"], chosen)
    lp = chosen - np.log(np.exp(chosen - chosen.max(-1, keepdims=True)).sum(-1, keepdims=True)) - chosen.max(-1, keepdims=True)
    _close(kernel, c["name"], "log_pi_a", got["log_pi_a"], lp[rows, got["action"]])
    _close(kernel, c["name"], "entropy", got["entropy"], -(np.exp(lp) * lp).sum(-1))
    # the carried state: what was read is recorded (raw), then prev <- option, init <- terminal
    assert np.array_equal(got["prev_option"], c["prev_option"]) and np.array_equal(got["init"], c["init"].astype(np.float32))
    assert np.array_equal(got["carried_prev"], got["option"]) and np.array_equal(got["carried_init"], (c["mask"] == 0).astype(np.uint8))
    return dec


@pytest.mark.parametrize("c", H.oc_head_cases(), ids=_ids(H.oc_head_cases()))
def test_oc_heads_edges(dra, dev, conv1, c):
    got = _run_oc_head(c, dev, dra.ops)
    _check_oc_head("oc_heads_fold28", c, got)
    col, value = (int(c["uniforms"][3]), c["uniforms"][5:]) if c["uniforms"] != "random" else (None, None)
    fresh, g = c["init"] != 0, np.argmax(got["q"], -1)
    if col == 0 and value == "zero":                         # u = 0: the first option with any probability
        assert np.all(got["option"][fresh] == (g[fresh] if c["eps"] == 0.0 else 0))
    if col == 0 and value == "almost-one":                   # u just under 1: the last option with any probability
        assert np.all(got["option"][fresh] == (g[fresh] if c["eps"] == 0.0 else c["O"] - 1))
    if col == 2 and value == "zero":
        assert np.all(got["action"] == 0)
    fused = _run_oc_head(c, dev, dra.ops, conv1=conv1)       # the same head in conv1's launch: bit for bit
    again = _run_oc_head(c, dev, dra.ops)
    for k in got:
        _same(fused[k], got[k], "rollout_conv1_ocheads[%s]: %s differs from the stand-alone head" % (c["name"], k))
        _same(again[k], got[k], "oc_heads_fold28[%s]: second run differs in %s" % (c["name"], k))


def test_fused_heads_at_their_limits_equal_the_stand_alone_heads(dra, dev, conv1):
    """A = 64 at B = 3 (Q head) and (O, A) = (8, 18) at B = 3 (option-critic head) in conv1's launch."""
    c = H.q_head_case(64, 3)
    alone, fused = _run_q_head(c, dev, dra.ops), _run_q_head(c, dev, dra.ops, conv1=conv1)
    for k in ("q", "action", "phi"):
        _same(fused[k], alone[k], "rollout_conv1_qheads A = 64, B = 3: " + k)
    c = H.oc_head_case(8, 18, 3, 0.3, k=0)
    alone, fused = _run_oc_head(c, dev, dra.ops), _run_oc_head(c, dev, dra.ops, conv1=conv1)
    _check_oc_head("rollout_conv1_ocheads", c, fused)
    for k in alone:
        _same(fused[k], alone[k], "rollout_conv1_ocheads (8, 18), B = 3: " + k)


@pytest.mark.parametrize("n_opt,batch,k", [(1, 1, 3), (2, 5, 4), (8, 5, 5), (3, 5, 1)])
def test_oc_heads_bootstrap_mode_edges(dra, dev, n_opt, batch, k):
    """Bootstrap mode with w_pi NULL (and, for k = 1, NULL biases): q, beta and boot against float64, the carried state untouched."""
    c = H.oc_head_case(n_opt, 2, batch, 0.3, k=k)
    outs = dict(q=_Out((batch, n_opt), dev), beta=_Out((batch, n_opt), dev), boot=_Out((batch,), dev))
    prev = _T(c["prev_option"], dev)
    for _ in range(2):
        dra.ops.oc_heads_fold28(_T(c["slabs"], dev), _T(c["fold_bias"], dev), _T(c["wq"], dev), _opt(c["bq"], dev), _T(c["wb"], dev),
                                _opt(c["bb"], dev), prev_option=prev, boot=outs["boot"].t, out=dict(q=outs["q"].t, beta=outs["beta"].t))
        torch.cuda.synchronize()
        got = {k_: o.np() for k_, o in outs.items()}
        first = got if _ == 0 else first
    for k_, o in outs.items():
        o.guards_ok("oc_heads_fold28 bootstrap " + k_)
        _same(got[k_], first[k_], "bootstrap mode: second run differs in " + k_)
    assert np.array_equal(prev.cpu().numpy(), c["prev_option"]), "bootstrap mode replaced the carried option"
    want = H.oc_head_ref(c)
    p = np.clip(c["prev_option"], 0, n_opt - 1)
    r = np.arange(batch)
    name = "%s bootstrap" % c["name"]
    _close("oc_heads_fold28", name, "q", got["q"], want["q"])
    _close("oc_heads_fold28", name, "beta", got["beta"], want["beta"])
    _close("oc_heads_fold28", name, "boot", got["boot"], (1 - want["beta"][r, p]) * want["q"][r, p] + want["beta"][r, p] * want["q"].max(-1))


# ------------------------------------------------------------------------------------------------------ Gaussian head
@pytest.mark.parametrize("c", H.gauss_cases(), ids=_ids(H.gauss_cases()))
def test_gauss_head_edges(dra, dev, c):
    import a2c_mlp_restatement as R
    from deeprl_amd._lib import lib, ptr, stream_ptr
    n, a = c["n"], c["A"]
    t = {k: _T(c[k], dev) for k in ("z", "std", "action", "g_lp", "g_ent")}

    def run():
        outs = dict(mean=_Out((n, a), dev), log_pi_a=_Out((n, 1), dev), entropy=_Out((n, 1), dev), dz=_Out((n, a), dev), dstd=_Out((a,), dev))
        lib.dra_gauss_head_fwd(ptr(t["z"]), ptr(t["std"]), ptr(t["action"]), n, a, ptr(outs["mean"].t), ptr(outs["log_pi_a"].t),
                               ptr(outs["entropy"].t), stream_ptr())
        lib.dra_gauss_head_bwd(ptr(t["z"]), ptr(t["std"]), ptr(t["action"]), ptr(t["g_lp"]), ptr(t["g_ent"]), n, a, ptr(outs["dz"].t),
                               ptr(outs["dstd"].t), stream_ptr())
        torch.cuda.synchronize()
        for k, o in outs.items():
            o.guards_ok("gauss_head[%s] %s" % (c["name"], k))
        return {k: o.np() for k, o in outs.items()}

    got = run()
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)
    mean, lp, ent = R.head(t64(c["z"]), t64(c["std"]), t64(c["action"]))
    dz, dstd = R.head_grads(c["z"], c["std"], c["action"], c["g_lp"], c["g_ent"])
    _close_all("gauss_head", c["name"], got, dict(mean=mean.numpy(), log_pi_a=lp.numpy(), entropy=ent.numpy(), dz=dz, dstd=dstd))
    assert np.abs(got["mean"]).max() > 0.999                 # the case does reach the saturated tanh
    again = run()
    for k in got:
        _same(again[k], got[k], "gauss_head[%s]: second run differs in %s" % (c["name"], k))


def test_gauss_head_limits_are_refused(dev):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    x = torch.zeros(4 * 65, device=dev)
    outs = {k: _Out((4 * 65,), dev) for k in ("mean", "log_pi_a", "entropy", "dz", "dstd")}
    o = lambda k: ptr(outs[k].t)
    rcs = [lib.dra_gauss_head_fwd.raw(ptr(x), ptr(x), ptr(x), n, a, o("mean"), o("log_pi_a"), o("entropy"), stream_ptr())
           for n, a in ((0, 4), (4, 0), (4, 65))]
    rcs += [lib.dra_gauss_head_bwd.raw(ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), n, a, o("dz"), o("dstd"), stream_ptr())
            for n, a in ((0, 4), (4, 0), (4, 65))]
    torch.cuda.synchronize()
    assert rcs == [EINVAL] * 6, rcs
    for k, out in outs.items():
        out.untouched("gauss_head " + k)
