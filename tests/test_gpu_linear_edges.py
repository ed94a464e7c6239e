"""Edge-shape parity of the generic linear-layer kernels behind nets.linear -- dra_linear_fwd's four kernels (gemv, rows, slabs,
K-chunked GEMM with and without its split-K finish), dra_linear_fwd_slabs(_one), dra_linear_bwd_w, dra_linear_bwd_x,
dra_linear_bwd_xw_one512, dra_act_bwd -- against float64 references, at the shapes where the launchers change kernel, tile or
split count.

Cases, references, the dispatch restatement and the bar live in tests/linear_edge_cases.py; tests/test_linear_edge_cases_host.py
proves on the CPU that every case reaches the path it is named for and that its inputs carry the bar.  Per case:
  parity        max |got - want64| <= 1e-5 * max |want64| per output tensor (E.bar: BAR, or the case's BAR_OVERRIDES entry); the
                measured error / scale goes to the parity log, one record per case
  exactness     on the integer operand set the outputs equal the int64 result
  bounds        every output sits in a buffer with NaN slack on both sides, the workspace has NaN behind the size that was passed:
                those bits are unchanged; every input has NaN behind it, so a stray read that reaches a result shows as NaN
  path          the workspace is NaN before the call; afterwards exactly E.workspace_written floats are not -- what ties the
                Python restatement of the dispatch to what the library did
  batch         gemv and rows: row b of the B-row call has the bits of the 1-row call on that row (first and last row of every
                32-row block)
  determinism   two fresh runs are bit-identical
  refusals      DRA_EINVAL, and NaN-filled outputs stay NaN"""
import ctypes

import numpy as np
import pytest
import torch

import linear_edge_cases as E
from parity_log import record_parity

pytestmark = pytest.mark.gpu

SLACK = 64           # floats: 256 bytes, so a view keeps the 16-byte alignment of its allocation (+ 4 bytes where a case says so)
EINVAL = -22
NAN_BITS = np.float32("nan").view(np.uint32)


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
    """n floats with NaN slack on both sides, the first of them `off` floats beyond a 16-byte boundary."""

    def __init__(self, n, dev, values=None, off=0):
        self.n, self.lo = int(n), SLACK + off
        self.whole = torch.full((self.lo + self.n + SLACK,), float("nan"), dtype=torch.float32, device=dev)
        self.v = self.whole[self.lo:self.lo + self.n]
        assert self.v.data_ptr() % 16 == (4 * off) % 16, "the allocation is not 16-byte aligned"
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
            assert values.size == self.n
            self.v.copy_(torch.from_numpy(values))

    def ptr(self):
        return ctypes.c_void_p(self.v.data_ptr())

    def get(self, shape=None):
        a = self.v.detach().cpu().numpy().copy()
        return a if shape is None else a.reshape(shape)

    def slack_untouched(self, what):
        w = self.whole.detach().cpu().numpy()
        out = np.concatenate([w[:self.lo], w[self.lo + self.n:]])
        assert np.all(out.view(np.uint32) == NAN_BITS), what + ": written outside its buffer"

    def all_nan(self, what):
        assert np.all(self.whole.detach().cpu().numpy().view(np.uint32) == NAN_BITS), what + ": written"


def _parr(bufs):
    arr = (ctypes.c_void_p * max(1, len(bufs)))()
    for i, b in enumerate(bufs):
        arr[i] = None if b is None else b.v.data_ptr()
    return arr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


class _Figures:
    """The error / scale of every output tensor of one case: printed, recorded (one record per case), then judged."""

    def __init__(self, name):
        self.name, self.figs, self.fail = name, {}, []

    def add(self, key, got, want):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (self.name, key, got.shape, want.shape)
        if not np.all(np.isfinite(got)):
            self.fail.append("%s: non-finite output (%d elements)" % (key, int((~np.isfinite(got)).sum())))
            return
        scale = float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        fig = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
        tensor = key.split("[")[0].split(" ")[0]
        print("linear edges %s %s: err/scale %.3g (bar %.1g), scale %.3g" % (self.name, key, fig, E.bar(self.name, tensor), scale))
        self.figs[key] = max(self.figs.get(key, 0.0), fig)
        if not fig <= E.bar(self.name, tensor):
            self.fail.append("%s: max abs err %.3e vs scale %.3e (%.2e of it, bar %.0e)" % (key, err, scale, fig, E.bar(self.name, tensor)))

    def exact(self, key, got, want):
        """Integer operand set: the values of the int64 result (-0.0 == 0.0), no NaN."""
        got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
        bad = ~(got.astype(np.float64) == want)
        if bad.any():
            i = np.argwhere(bad)[0]
            self.fail.append("%s: %d of %d elements differ from the int64 result, first at %s: got %r want %r" % (
                key, int(bad.sum()), bad.size, tuple(i), got[tuple(i)], want[tuple(i)]))

    def done(self):
        record_parity("linear edges " + self.name, **{k.replace("[", "_").replace("]", "").replace(" ", "_") + "_err_over_scale": v
                                                       for k, v in self.figs.items()})
        assert not self.fail, "%s: %s" % (self.name, "; ".join(self.fail))


def _sync():
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------- dra_linear_fwd
class _Fwd:
    """One case's weights and biases on the device (uploaded once), and runs of dra_linear_fwd on given input rows."""

    def __init__(self, c, op, dev):
        self.c, self.dev = c, dev
        woff = 1 if "w" in c["off"] else 0
        self.w = [_Buf(c["O"] * c["K"], dev, w, woff) for w in op["w"]]
        self.bias = [None if b is None else _Buf(c["O"], dev, b) for b in op["bias"]]

    def run(self, xs, act):
        from deeprl_amd import ops
        from deeprl_amd._lib import lib, stream_ptr
        c, dev = self.c, self.dev
        B, K, O, nz = xs[0].shape[0], c["K"], c["O"], c["nz"]
        x = [_Buf(B * K, dev, a, 1 if "x" in c["off"] else 0) for a in xs]
        y = [_Buf(B * O, dev) for _ in range(nz)]
        ws = _Buf(c["ws_floats"], dev)
        rc = lib.dra_linear_fwd.raw(nz, _parr(x), _parr(self.w), None if c["null_bias"] == "array" else _parr(self.bias), _parr(y), B, K, O,
                                    ops.ACT[act], None if c["ws_null"] else ws.ptr(), c["ws_floats"], stream_ptr())
        _sync()
        assert rc == 0, "%s: dra_linear_fwd returned %d" % (c["name"], rc)
        for z in range(nz):
            y[z].slack_untouched("%s y[%d]" % (c["name"], z))
        wsn = ws.whole.detach().cpu().numpy()
        return [b.get((B, O)) for b in y], wsn


def _check_workspace(c, wsn, B, what):
    """Only the first E.workspace_written floats of the workspace are written (the slabs are [z][split][B][O] from its start)."""
    want = E.workspace_written(c["reaches"], B, c["O"], c["nz"])
    written = ~(wsn.view(np.uint32) == NAN_BITS)
    assert int(written.sum()) == want, "%s %s: %d workspace floats written, the path %r writes %d" % (
        c["name"], what, int(written.sum()), c["reaches"], want)
    assert want <= c["ws_floats"] and np.all(written[SLACK:SLACK + want]), "%s %s: written outside the workspace that was passed" % (c["name"], what)


@pytest.mark.parametrize("c", E.FWD_CASES, ids=_ids(E.FWD_CASES))
def test_linear_fwd_edges(dev, c):
    figs = _Figures(c["name"])
    op = E.fwd_operands(c["name"], "random")
    st = _Fwd(c, op, dev)
    ys, wsn = st.run(op["x"], c["act"])
    _check_workspace(c, wsn, c["B"], "random")
    for z in range(c["nz"]):
        figs.add("y[%d]" % z, ys[z], op["want"][z])
    # determinism: a second run on fresh buffers
    ys2, wsn2 = _Fwd(c, op, dev).run(op["x"], c["act"])
    for z in range(c["nz"]):
        _same(ys2[z], ys[z], "%s: second run differs in y[%d]" % (c["name"], z))
    _same(wsn2, wsn, c["name"] + ": second run differs in the workspace")
    # batch independence of the gemv / rows kernels
    if c["reaches"][0] in ("gemv", "rows"):
        for b in E.rows_to_compare(c["B"]):
            one, _ = st.run([x[b:b + 1] for x in op["x"]], c["act"])
            for z in range(c["nz"]):
                _same(one[z][0], ys[z][b], "%s: row %d of the %d-row call is not the 1-row call's (z = %d)" % (c["name"], b, c["B"], z))
    # the integer operand set
    ints = E.fwd_operands(c["name"], "integer")
    yi, wsi = _Fwd(c, ints, dev).run(ints["x"], None)
    _check_workspace(c, wsi, c["B"], "integer")
    for z in range(c["nz"]):
        figs.exact("integer y[%d]" % z, yi[z], ints["want"][z])
    figs.done()


# -------------------------------------------------------------------------- dra_linear_fwd_slabs / dra_linear_fwd_slabs_one
def _slab_ranges(c):
    """K range of every split: whole 64-wide chunks, ceil(chunks / ksplit) each (igemm.h:85-88); equal slices for the one-pass form."""
    K, ks = c["K"], c["ksplit"]
    if c["one_pass"]:
        return [(s * (K // ks), (s + 1) * (K // ks)) for s in range(ks)]
    cper = ((K + 63) // 64 + ks - 1) // ks
    return [(min(K, s * cper * 64), min(K, (s + 1) * cper * 64)) for s in range(ks)]


def _run_slabs(c, op, dev):
    from deeprl_amd._lib import lib, stream_ptr
    B, K, O, nz, ks = c["B"], c["K"], c["O"], c["nz"], c["ksplit"]
    x = [_Buf(B * K, dev, a) for a in op["x"]]
    w = [_Buf(O * K, dev, a) for a in op["w"]]
    slabs = _Buf(nz * ks * B * O, dev)
    fn = lib.dra_linear_fwd_slabs_one if c["one_pass"] else lib.dra_linear_fwd_slabs
    rc = fn.raw(nz, _parr(x), _parr(w), B, K, O, ks, slabs.ptr(), stream_ptr())
    _sync()
    assert rc == 0, (c["name"], rc)
    slabs.slack_untouched(c["name"] + " slabs")
    return slabs.get((nz, ks, B, O))


@pytest.mark.parametrize("c", E.SLABS_CASES + E.SLABS_ONE_CASES, ids=_ids(E.SLABS_CASES + E.SLABS_ONE_CASES))
def test_linear_fwd_slabs_edges(dev, c):
    figs = _Figures(c["name"])
    op = E.slabs_operands(c["name"], "random")
    s = _run_slabs(c, op, dev)
    assert np.all(np.isfinite(s)), c["name"] + ": a slab element was not written"
    for z in range(c["nz"]):
        figs.add("sum[%d]" % z, s[z].astype(np.float64).sum(0), op["want"][z])
    _same(_run_slabs(c, op, dev), s, c["name"] + ": second run differs")
    ints = E.slabs_operands(c["name"], "integer")
    si = _run_slabs(c, ints, dev)
    assert np.all(np.isfinite(si)), c["name"] + ": a slab element was not written (integer set)"
    for z in range(c["nz"]):
        figs.exact("integer sum[%d]" % z, si[z].astype(np.float64).sum(0), ints["want"][z])
        X, W = ints["x"][z].astype(np.int64), ints["w"][z].astype(np.int64)
        for k, (k0, k1) in enumerate(_slab_ranges(c)):      # every slab is its own K range (zeros where a split owns no chunk)
            figs.exact("integer slab[%d][%d]" % (z, k), si[z, k], X[:, k0:k1] @ W[:, k0:k1].T)
    figs.done()


def test_linear_fwd_slabs_one_refusals(dev):
    from deeprl_amd._lib import lib, stream_ptr
    B, O = 33, 40
    for what, K, ks, off in E.SLABS_ONE_REFUSALS:
        assert not E.slabs_one_accepts(K, ks, off is None)
        x = _Buf(B * K, dev, np.ones(B * K), 1 if off == "x" else 0)
        w = _Buf(O * K, dev, np.ones(O * K), 1 if off == "w" else 0)
        slabs = _Buf(max(ks, 8) * B * O, dev)
        rc = lib.dra_linear_fwd_slabs_one.raw(1, _parr([x]), _parr([w]), B, K, O, ks, slabs.ptr(), stream_ptr())
        _sync()
        assert rc == EINVAL, "dra_linear_fwd_slabs_one, %s: returned %d" % (what, rc)
        slabs.all_nan("dra_linear_fwd_slabs_one, %s: refused, but the slabs were" % what)


# --------------------------------------------------------------------------------------------------- dra_linear_bwd_w
def _run_bwd_w(c, op, dev):
    from deeprl_amd._lib import lib, stream_ptr
    B, I, O = c["B"], c["I"], c["O"]
    dy, x = _Buf(B * O, dev, op["dy"]), _Buf(B * I, dev, op["x"])
    dw, db = _Buf(O * I, dev), _Buf(O, dev)
    rc = lib.dra_linear_bwd_w.raw(dy.ptr(), x.ptr(), dw.ptr(), db.ptr() if c["db"] else None, B, I, O, stream_ptr())
    _sync()
    assert rc == 0, (c["name"], rc)
    dw.slack_untouched(c["name"] + " dw")
    if c["db"]:
        db.slack_untouched(c["name"] + " db")
    else:
        db.all_nan(c["name"] + ": db = NULL, but a bias gradient was")
    return dw.get((O, I)), db.get()


@pytest.mark.parametrize("c", E.BWD_W_CASES, ids=_ids(E.BWD_W_CASES))
def test_linear_bwd_w_edges(dev, c):
    figs = _Figures(c["name"])
    op = E.bwd_w_operands(c["name"], "random")
    dw, db = _run_bwd_w(c, op, dev)
    figs.add("dw", dw, op["dw"])
    if c["db"]:
        figs.add("db", db, op["db"])
    dw2, db2 = _run_bwd_w(c, op, dev)
    _same(dw2, dw, c["name"] + ": second run differs in dw")
    _same(db2, db, c["name"] + ": second run differs in db")
    ints = E.bwd_w_operands(c["name"], "integer")
    dwi, dbi = _run_bwd_w(c, ints, dev)
    figs.exact("integer dw", dwi, ints["dw"])
    if c["db"]:
        figs.exact("integer db", dbi, ints["db"])
    figs.done()


# --------------------------------------------------------------------------------------------------- dra_linear_bwd_x
def _run_bwd_x(c, op, dev):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, stream_ptr
    B, I, O = c["B"], c["I"], c["O"]
    dy, w = _Buf(B * O, dev, op["dy"]), _Buf(O * I, dev, op["w"])
    xact = None if op["xact"] is None else _Buf(B * I, dev, op["xact"])
    dx = _Buf(B * I, dev)
    rc = lib.dra_linear_bwd_x.raw(dy.ptr(), w.ptr(), None if xact is None else xact.ptr(), dx.ptr(), B, I, O, ops.ACT[op["mask"]],
                                  stream_ptr())
    _sync()
    assert rc == 0, (c["name"], rc)
    dx.slack_untouched(c["name"] + " dx")
    return dx.get((B, I))


@pytest.mark.parametrize("c", E.BWD_X_CASES, ids=_ids(E.BWD_X_CASES))
def test_linear_bwd_x_edges(dev, c):
    figs = _Figures(c["name"])
    op = E.bwd_x_operands(c["name"], "random")
    dx = _run_bwd_x(c, op, dev)
    figs.add("dx", dx, op["dx"])
    _same(_run_bwd_x(c, op, dev), dx, c["name"] + ": second run differs")
    ints = E.bwd_x_operands(c["name"], "integer")
    figs.exact("integer dx", _run_bwd_x(c, ints, dev), ints["dx"])
    figs.done()


# ------------------------------------------------------------------------------------------- dra_linear_bwd_xw_one512
def _run_xw(c, op, dev):
    """-> the one launch's (dx, dw, db) and the two separate launches' on the same device operands."""
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, stream_ptr
    B, I, O = c["B"], c["I"], 512
    dy, w, x = _Buf(B * O, dev, op["dy"]), _Buf(O * I, dev, op["w"]), _Buf(B * I, dev, op["x"])
    out = {}
    for form in ("one", "two"):
        dx, dw, db = _Buf(B * I, dev), _Buf(O * I, dev), _Buf(O, dev)
        dbp = db.ptr() if c["db"] else None
        if form == "one":
            rc = lib.dra_linear_bwd_xw_one512.raw(dy.ptr(), w.ptr(), x.ptr(), 1 if c["relu"] else 0, dx.ptr(), dw.ptr(), dbp, B, I, stream_ptr())
        else:
            rc = lib.dra_linear_bwd_x.raw(dy.ptr(), w.ptr(), x.ptr() if c["relu"] else None, dx.ptr(), B, I, O,
                                          ops.ACT["relu" if c["relu"] else None], stream_ptr())
            rc = rc or lib.dra_linear_bwd_w.raw(dy.ptr(), x.ptr(), dw.ptr(), dbp, B, I, O, stream_ptr())
        _sync()
        assert rc == 0, (c["name"], form, rc)
        for k, b in (("dx", dx), ("dw", dw)):
            b.slack_untouched("%s %s (%s)" % (c["name"], k, form))
        if c["db"]:
            db.slack_untouched("%s db (%s)" % (c["name"], form))
        else:
            db.all_nan("%s (%s): db = NULL, but a bias gradient was" % (c["name"], form))
        out[form] = (dx.get((B, I)), dw.get((O, I)), db.get())
    return out


@pytest.mark.parametrize("c", E.XW_CASES, ids=_ids(E.XW_CASES))
def test_linear_bwd_xw_one512_edges(dev, c):
    figs = _Figures(c["name"])
    op = E.xw_operands(c["name"], "random")
    r = _run_xw(c, op, dev)
    for k, got, sep in zip(("dx", "dw", "db"), r["one"], r["two"]):
        if k != "db" or c["db"]:
            figs.add(k, got, op[k])
        _same(got, sep, "%s: %s of the one launch is not dra_linear_bwd_x + dra_linear_bwd_w's" % (c["name"], k))
    again = _run_xw(c, op, dev)
    for k, got, g2 in zip(("dx", "dw", "db"), r["one"], again["one"]):
        _same(g2, got, "%s: second run differs in %s" % (c["name"], k))
    ints = E.xw_operands(c["name"], "integer")
    ri = _run_xw(c, ints, dev)
    for k, got in zip(("dx", "dw", "db"), ri["one"]):
        if k != "db" or c["db"]:
            figs.exact("integer " + k, got, ints[k])
    figs.done()


# -------------------------------------------------------------------------------------------------------- dra_act_bwd
@pytest.mark.parametrize("c", E.ACT_BWD_CASES, ids=_ids(E.ACT_BWD_CASES))
def test_act_bwd_edges(dev, c):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, stream_ptr
    dy_np, y_np, want = E.act_bwd_operands(c["name"])
    n = c["n"]
    got = []
    for _ in range(2):
        dy, y, out = _Buf(n, dev, dy_np), _Buf(n, dev, y_np), _Buf(n, dev)
        rc = lib.dra_act_bwd.raw(dy.ptr(), y.ptr(), out.ptr(), n, ops.ACT[c["act"]], stream_ptr())
        _sync()
        assert rc == 0
        out.slack_untouched(c["name"])
        got.append(out.get())
    bad = _bits(got[0]) != _bits(want)
    record_parity("linear edges " + c["name"], differing_elements=int(bad.sum()))
    assert not bad.any(), "%s: %d of %d elements are not float32(dy * act'(y)), first at %d" % (c["name"], int(bad.sum()), n, int(np.argmax(bad)))
    _same(got[1], got[0], c["name"] + ": second run differs")


def test_act_bwd_of_nothing_writes_nothing(dev):
    from deeprl_amd._lib import lib, stream_ptr
    dy, y, out = _Buf(4, dev, np.ones(4)), _Buf(4, dev, np.ones(4)), _Buf(4, dev)
    for act in (0, 1, 2):
        assert lib.dra_act_bwd.raw(dy.ptr(), y.ptr(), out.ptr(), 0, act, stream_ptr()) == 0
    _sync()
    out.all_nan("dra_act_bwd(n = 0): the output was")


# ------------------------------------------------------------------------------------------- nets.linear under autograd
def _run_autograd(c, op, dev, direct):
    from deeprl_amd import nets
    x = torch.from_numpy(op["x"]).to(dev).requires_grad_(True)
    w = torch.nn.Parameter(torch.from_numpy(op["w"]).to(dev))
    b = torch.nn.Parameter(torch.from_numpy(op["b"]).to(dev))
    dy = torch.from_numpy(op["dy"]).to(dev)
    slots = None
    if direct:      # contiguous .grad slots, as views of NaN-slacked buffers: the backward overwrites them in place
        slots = (_Buf(w.numel(), dev, np.zeros(w.numel())), _Buf(b.numel(), dev, np.zeros(b.numel())))
        w.grad, b.grad = slots[0].v.view(w.shape), slots[1].v.view(b.shape)
        assert w.grad.is_contiguous() and b.grad.is_contiguous()
    with nets.direct_param_grads(enable=direct):
        y = nets.linear(x, w, b, act=c["act"], x_relu=c["x_relu"])
        y.backward(dy)
    _sync()
    if direct:
        assert w.grad.data_ptr() == slots[0].v.data_ptr() and b.grad.data_ptr() == slots[1].v.data_ptr(), "the .grad slots were replaced"
        slots[0].slack_untouched(c["name"] + " dW slot")
        slots[1].slack_untouched(c["name"] + " db slot")
    return {k: t.detach().cpu().numpy().copy() for k, t in (("y", y), ("dx", x.grad), ("dw", w.grad), ("db", b.grad))}


@pytest.mark.parametrize("c", E.AUTOGRAD_CASES, ids=_ids(E.AUTOGRAD_CASES))
def test_nets_linear_autograd_edges(dev, c):
    figs = _Figures(c["name"])
    op = E.autograd_operands(c["name"])
    direct, plain = _run_autograd(c, op, dev, True), _run_autograd(c, op, dev, False)
    for k in ("y", "dx", "dw", "db"):
        figs.add(k, direct[k], op[k])
        _same(plain[k], direct[k], "%s: %s with .grad slots written in place differs from autograd's accumulation" % (c["name"], k))
    figs.done()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_argument_limits_are_refused_before_any_launch(dev):
    """Every argument check of the launchers, through .raw: DRA_EINVAL, nothing launched -- the buffers are real and large enough
    for the launch each call describes, and the NaN-filled outputs keep their bits."""
    from deeprl_amd._lib import lib, stream_ptr
    s = stream_ptr()
    refused = {}
    outs = []
    # dra_linear_fwd at one shape per path: (B, K, O)
    for path, (B, K, O) in (("gemv", (4, 8, 3)), ("rows", (4, 1024, 3)), ("slabs", (33, 3136, 2)), ("igemm", (33, 1092, 2))):
        assert E.fwd_path(B, K, O, 2, True, 2 * 32 * B * O)[0].startswith(path)
        x = [_Buf(B * K, dev, np.ones(B * K)) for _ in range(5)]
        w = [_Buf(O * K, dev, np.ones(O * K)) for _ in range(5)]
        bias = [_Buf(O, dev, np.ones(O)) for _ in range(5)]
        y = [_Buf(B * O, dev) for _ in range(5)]
        ws = _Buf(5 * 32 * B * O, dev)
        outs += y + [ws]

        def fwd(nz=2, xs=_parr(x), wp=_parr(w), bp=_parr(bias), yp=_parr(y), B=B, K=K, O=O):
            return lib.dra_linear_fwd.raw(nz, xs, wp, bp, yp, B, K, O, 0, ws.ptr(), ws.n, s)

        refused.update({
            path + ": nz = 0": fwd(nz=0), path + ": nz = 5": fwd(nz=5), path + ": batch 0": fwd(B=0), path + ": in_features 0": fwd(K=0),
            path + ": out_features 0": fwd(O=0), path + ": no x array": fwd(xs=None), path + ": no w array": fwd(wp=None),
            path + ": no y array": fwd(yp=None), path + ": x[1] null": fwd(xs=_parr([x[0], None])),
            path + ": w[1] null": fwd(wp=_parr([w[0], None])), path + ": y[0] null": fwd(yp=_parr([None, y[1]])),
        })
    B, I, O = 5, 1024, 512
    dy, x, w = _Buf(B * O, dev, np.ones(B * O)), _Buf(B * I, dev, np.ones(B * I)), _Buf(O * I, dev, np.ones(O * I))
    dx, dw, db, slabs = _Buf(B * I, dev), _Buf(O * I, dev), _Buf(O, dev), _Buf(4 * 4 * B * O, dev)
    outs += [dx, dw, db, slabs]

    def bw(dyp=dy.ptr(), xp=x.ptr(), dwp=dw.ptr(), B=B, I=I, O=O):
        return lib.dra_linear_bwd_w.raw(dyp, xp, dwp, db.ptr(), B, I, O, s)

    def bx(dyp=dy.ptr(), wp=w.ptr(), dxp=dx.ptr(), B=B, I=I, O=O):
        return lib.dra_linear_bwd_x.raw(dyp, wp, x.ptr(), dxp, B, I, O, 1, s)

    def xw(dyp=dy.ptr(), wp=w.ptr(), xp=x.ptr(), dxp=dx.ptr(), dwp=dw.ptr(), B=B, I=I):
        return lib.dra_linear_bwd_xw_one512.raw(dyp, wp, xp, 1, dxp, dwp, db.ptr(), B, I, s)

    def sl(nz=1, xs=_parr([x]), wp=_parr([w]), B=B, K=I, O=O, ks=4, sp=slabs.ptr()):
        return lib.dra_linear_fwd_slabs.raw(nz, xs, wp, B, K, O, ks, sp, s)

    def ab(dyp=dy.ptr(), yp=x.ptr(), outp=dx.ptr(), n=B * O):
        return lib.dra_act_bwd.raw(dyp, yp, outp, n, 1, s)

    refused.update({
        "bwd_w: no dy": bw(dyp=None), "bwd_w: no x": bw(xp=None), "bwd_w: no dw": bw(dwp=None), "bwd_w: batch 0": bw(B=0),
        "bwd_w: in_features 0": bw(I=0), "bwd_w: out_features 0": bw(O=0),
        "bwd_x: no dy": bx(dyp=None), "bwd_x: no w": bx(wp=None), "bwd_x: no dx": bx(dxp=None), "bwd_x: batch 0": bx(B=0),
        "bwd_x: in_features 0": bx(I=0), "bwd_x: out_features 0": bx(O=0),
        "bwd_xw: in_features 1023": xw(I=1023), "bwd_xw: no dy": xw(dyp=None), "bwd_xw: no w": xw(wp=None), "bwd_xw: no x": xw(xp=None),
        "bwd_xw: no dx": xw(dxp=None), "bwd_xw: no dw": xw(dwp=None), "bwd_xw: batch 0": xw(B=0),
        "slabs: nz = 0": sl(nz=0), "slabs: nz = 5": sl(nz=5, xs=_parr([x] * 5), wp=_parr([w] * 5)), "slabs: batch 0": sl(B=0),
        "slabs: in_features 0": sl(K=0), "slabs: out_features 0": sl(O=0), "slabs: ksplit 1": sl(ks=1), "slabs: no x array": sl(xs=None),
        "slabs: no w array": sl(wp=None), "slabs: no slabs": sl(sp=None), "slabs: x[0] null": sl(xs=_parr([None])),
        "slabs: w[0] null": sl(wp=_parr([None])),
        "act_bwd: no dy": ab(dyp=None), "act_bwd: no y": ab(yp=None), "act_bwd: no output": ab(outp=None), "act_bwd: n = -1": ab(n=-1),
    })
    _sync()
    wrong = {k: rc for k, rc in refused.items() if rc != EINVAL}
    assert not wrong, "expected DRA_EINVAL (%d): %s" % (EINVAL, wrong)
    assert not E.xw_one512_accepts(1023)
    for b in outs:
        b.all_nan("a refused call's output or workspace was")
