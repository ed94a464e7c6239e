"""Edge-batch parity of the Nature-CNN conv kernels -- dra_conv_fwd_koc on every path of launch_conv_v2 (eight- and four-wave latency
shapes, the persistent throughput kernels, conv1's own uint8 throughput kernel with each (spg, tp), the two-tile grid of float conv1),
dra_conv_bwd_fused with the slab count of dra_conv_wgrad_slabs on every weight-gradient role and input-gradient form,
dra_conv1_fwd_koc_ring, dra_transpose_f32 -- against float64 references, at the batches where the launchers change kernel, share size
or launch count.

Cases, references, the dispatch restatement and the bar live in tests/conv_edge_cases.py; tests/test_conv_edge_cases_host.py proves on
the CPU that every case reaches the path it is named for and that its inputs carry the bar.  Per case:
  parity        max |got - want64| <= 1e-5 * max |want64| per output tensor (E.bar); with act none on the pre-activations themselves;
                the measured error / scale goes to the parity log, one record per case
  exactness     on the integer operand set the outputs equal the integer result
  bounds        every output, slab and dX buffer is called through the C entry point with a buffer the test owns, between 4 KB of
                NaN sentinels: the sentinels keep their bits and every element between them is written
  path          the slab buffer is NaN before the call and two slabs longer than dra_conv_wgrad_slabs says: exactly that many
                slabs are written and the count is the restatement's -- what ties the Python restatement to what the library did
  determinism   a second launch is bit-identical (no atomics anywhere)
and, across cases: the bit-identities the code states (shared batch prefix / suffix against the four-wave latency shape, one launch of
nz nets against nz launches, uint8 against float conv1, slabs with and without the scatter bit), batch independence, refusals.
profiles/conv_edges_parity_errors.json is tools/parity_summary.py over this file's "conv edges" records."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_edge_cases as E
from parity_log import record_parity

pytestmark = pytest.mark.gpu

SLACK = 1024         # floats: 4 KB of sentinels on each side; a view keeps the 16-byte alignment of its allocation
EXTRA_SLABS = 2      # rows behind the slab count that must stay untouched
EINVAL = -22
NAN_BITS = int(np.float32("nan").view(np.int32))
N_CU = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
FWD_CASES = E.fwd_cases(N_CU)


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
    """n floats between two NaN-filled sentinel regions of SLACK floats, checked on the device."""

    def __init__(self, n, dev, values=None):
        self.n = int(n)
        self.whole = torch.full((2 * SLACK + self.n,), float("nan"), dtype=torch.float32, device=dev)
        self.v = self.whole[SLACK:SLACK + self.n]
        assert self.v.data_ptr() % 16 == 0, "the allocation is not 16-byte aligned"
        if values is not None:
            self.v.copy_(torch.as_tensor(values, dtype=torch.float32).reshape(-1))

    def ptr(self):
        return ctypes.c_void_p(self.v.data_ptr())

    def _bits(self):
        return self.whole.view(torch.int32)

    def sentinels_intact(self, what):
        b = self._bits()
        assert bool((b[:SLACK] == NAN_BITS).all()) and bool((b[SLACK + self.n:] == NAN_BITS).all()), what + ": written outside its buffer"

    def written(self, what, n=None):
        n = self.n if n is None else n
        bad = int(torch.isnan(self.v[:n]).sum())
        assert bad == 0, "%s: %d of %d elements were not written" % (what, bad, n)

    def untouched(self, what, start=None):
        """Nothing at all was written (start None), or nothing from element `start` on."""
        b = self._bits() if start is None else self._bits()[SLACK + start:]
        assert bool((b == NAN_BITS).all()), what + ": written"


def _parr(items):
    arr = (ctypes.c_void_p * max(1, len(items)))()
    for i, t in enumerate(items):
        arr[i] = None if t is None else (t.v.data_ptr() if isinstance(t, _Buf) else t.data_ptr())
    return arr


def _p(t):
    return None if t is None else ctypes.c_void_p(t.v.data_ptr() if isinstance(t, _Buf) else t.data_ptr())


def _sync():
    torch.cuda.synchronize()


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
        print("conv edges %s %s: err/scale %.3g (bar %.1g), scale %.3g" % (self.name, key, fig, E.bar(self.name, tensor), scale))
        self.figs[key] = max(self.figs.get(key, 0.0), fig)
        if not fig <= E.bar(self.name, tensor):
            self.fail.append("%s: max abs err %.3e vs scale %.3e (%.2e of it, bar %.0e)" % (key, err, scale, fig, E.bar(self.name, tensor)))

    def exact(self, key, got, want):
        """Integer operand set: the values of the integer result (-0.0 == 0.0), no NaN."""
        got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (self.name, key, got.shape, want.shape)
        bad = ~(got.astype(np.float64) == want)
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            self.fail.append("%s: %d of %d elements differ from the integer result, first at %s: got %r want %r" % (
                key, int(bad.sum()), bad.size, i, got[i], want[i]))

    def done(self):
        record_parity("conv edges " + self.name, **{k.replace("[", "_").replace("]", "").replace(" ", "_") + "_err_over_scale": v
                                                     for k, v in self.figs.items()})
        assert not self.fail, "%s: %s" % (self.name, "; ".join(self.fail))


# --------------------------------------------------------------------------------------------------- dra_conv_fwd_koc
class _Fwd:
    """One forward problem on the device (inputs, KOC weights and biases uploaded once) and launches of dra_conv_fwd_koc on it."""

    def __init__(self, layer, u8, xs, ws, bs, coef, dev):
        self.layer, self.u8, self.coef, self.dev = layer, u8, float(coef if u8 else 1.0), dev
        self.x = [torch.as_tensor(x).to(dev).contiguous() for x in xs]
        assert all(x.dtype == (torch.uint8 if u8 else torch.float32) for x in self.x)
        self.wt = [torch.as_tensor(E.to_koc(w)).to(dev) for w in ws]
        self.b = [torch.as_tensor(b).to(dev) for b in bs]

    def run(self, act, rows=None, nets=None, what=""):
        """-> one [B, OC, OH, OH] tensor per net (views of guarded buffers); rows: a slice of the batch; nets: a subset of the nets."""
        from deeprl_amd import ops
        from deeprl_amd._lib import lib, stream_ptr
        nets = list(range(len(self.x))) if nets is None else nets
        xs = [self.x[z] if rows is None else self.x[z][rows].contiguous() for z in nets]
        batch, o, oc = xs[0].shape[0], E.out_hw(self.layer), E.GEOM[self.layer][2]
        ys = [_Buf(batch * oc * o * o, self.dev) for _ in nets]
        rc = lib.dra_conv_fwd_koc.raw(self.layer, len(nets), _parr(xs), _parr([self.wt[z] for z in nets]), _parr([self.b[z] for z in nets]),
                                      _parr(ys), batch, int(self.u8), self.coef, ops.ACT[act], stream_ptr())
        _sync()
        assert rc == 0, "%s: dra_conv_fwd_koc returned %d" % (what, rc)
        for i, y in enumerate(ys):
            y.sentinels_intact("%s y[%d]" % (what, i))
            y.written("%s y[%d]" % (what, i))
        return [y.v.view(batch, oc, o, o) for y in ys]


def _fwd_of(c, op, dev, u8=None):
    u8 = c["u8"] if u8 is None else u8
    return _Fwd(c["layer"], u8, op["x8"] if u8 else op["x"], op["w"], op["b"], op["coef"], dev)


@pytest.mark.parametrize("c", FWD_CASES, ids=_ids(FWD_CASES))
def test_conv_fwd_edges(dev, c):
    figs = _Figures(c["name"])
    for kind in ("random", "integer"):
        op = E.fwd_operands(c["layer"], c["batch"], c["nz"], kind, N_CU)
        act = c["act"] if kind == "random" else None        # the integer set is judged on the pre-activations
        st = _fwd_of(c, op, dev)
        ys = st.run(act, what=c["name"] + " " + kind)
        keep = torch.as_tensor(op["keep"], device=dev)
        for z in range(c["nz"]):
            got = ys[z][keep].cpu().numpy()
            if kind == "random":
                figs.add("y[%d]" % z, got, E.act64(op["pre"][z], act))
            else:
                figs.exact("integer y[%d]" % z, got, op["pre"][z])
        again = st.run(act, what=c["name"] + " " + kind + " second launch")
        for z in range(c["nz"]):
            assert torch.equal(again[z], ys[z]), "%s %s: the second launch differs in y[%d]" % (c["name"], kind, z)
    figs.done()


@pytest.mark.parametrize("layer,u8,batch", E.PREFIX_CASES, ids=["L%d-%s-b%d" % (l, "u8" if u else "f32", b) for l, u, b in E.PREFIX_CASES])
def test_throughput_shapes_share_the_latency_shape_bits(dev, layer, u8, batch):
    """Every throughput shape states the same arithmetic per output position as the four-wave latency shape (17 .. 127 samples): a
    prefix and a suffix of the big launch are the small launch's bits -- 127 of 128 across the 127 | 128 switch, 40 elsewhere."""
    op = E.fwd_operands(layer, batch, 1, "random", N_CU)
    c = dict(layer=layer, u8=u8)
    st = _fwd_of(c, op, dev)
    n = 127 if batch == 128 else 40
    assert E.fwd_path(layer, u8, n, 1, N_CU) == ("latency four-wave",) and E.fwd_path(layer, u8, batch, 1, N_CU) != ("latency four-wave",)
    for act in ("relu", None):
        big = st.run(act, what="prefix big")[0]
        head = st.run(act, rows=slice(0, n), what="prefix head")[0]
        tail = st.run(act, rows=slice(batch - n, batch), what="prefix tail")[0]
        assert torch.equal(big[:n], head), "conv%d batch %d (%s): the first %d samples are not the %d-sample launch's" % (layer, batch, act, n, n)
        assert torch.equal(big[batch - n:], tail), "conv%d batch %d (%s): the last %d samples are not the %d-sample launch's" % (layer, batch, act, n, n)


NZ_CASES = [c for c in FWD_CASES if c["nz"] > 1 and (c["batch"] == 131 and c["nz"] == 3 or c["reaches"][0] == "conv1-u8-tp")]


@pytest.mark.parametrize("c", NZ_CASES, ids=_ids(NZ_CASES))
def test_one_launch_of_nz_nets_is_nz_launches(dev, c):
    op = E.fwd_operands(c["layer"], c["batch"], c["nz"], "random", N_CU)
    st = _fwd_of(c, op, dev)
    together = st.run(c["act"], what=c["name"])
    for z in range(c["nz"]):
        alone = st.run(c["act"], nets=[z], what=c["name"] + " net %d alone" % z)[0]
        assert torch.equal(together[z], alone), "%s: net %d of the %d-net launch is not its own launch's" % (c["name"], z, c["nz"])


@pytest.mark.parametrize("batch", E.U8_F32_BATCHES)
def test_conv1_uint8_equals_float_on_the_normalised_values(dev, batch):
    """The uint8 paths normalise f32(f64(v) * coef) exactly and contract in the float paths' order: the same bits at every shape."""
    op = E.fwd_operands(1, batch, 1, "random", N_CU)
    c = dict(layer=1)
    assert E.fwd_path(1, True, batch, 1, N_CU) != E.fwd_path(1, False, batch, 1, N_CU) or batch < 128
    for act in ("relu", None):
        y8 = _fwd_of(c, op, dev, u8=True).run(act, what="u8 %d" % batch)[0]
        yf = _fwd_of(c, op, dev, u8=False).run(act, what="f32 %d" % batch)[0]
        diff = int((y8 != yf).sum())
        assert diff == 0, "conv1 batch %d (%s): %d of %d outputs differ between uint8 and float frames" % (batch, act, diff, y8.numel())


FWD_INDEPENDENCE = E.fwd_independence(N_CU)


@pytest.mark.parametrize("layer,u8,batch,nz", FWD_INDEPENDENCE, ids=["L%d-%s-b%d" % (l, "u8" if u else "f32", b) for l, u, b, _ in FWD_INDEPENDENCE])
def test_forward_batch_independence(dev, layer, u8, batch, nz):
    rs = E._rs("independence", layer, u8, batch)
    w, b = E.draw_weights(rs, layer, "random")
    x8, x, coef = E.draw_input(rs, layer, batch, "random")
    x = x8 if u8 else x
    j = (batch // 2) | 1 if batch > 2 else 1              # an odd sample: the second of a two-sample group
    x2 = x.copy()
    x2[j] = (255 - x[j]) if u8 else x[j] + 1.0
    y = _Fwd(layer, u8, [x], [w], [b], coef, dev).run(None, what="independence")[0]
    y2 = _Fwd(layer, u8, [x2], [w], [b], coef, dev).run(None, what="independence, changed")[0]
    others = [i for i in range(batch) if i != j]
    assert torch.equal(y[others], y2[others]), "conv%d batch %d: changing sample %d changed another sample's outputs" % (layer, batch, j)
    assert not torch.equal(y[j], y2[j]), "conv%d batch %d: changing sample %d did not change its outputs" % (layer, batch, j)


# -------------------------------------------------------------------------------- dra_conv_bwd_fused + dra_conv_wgrad_slabs
@functools.lru_cache(maxsize=2)
def _bwd_device(layer, batch, kind, dev):
    op = E.bwd_operands(layer, batch, kind)
    d = dict(dy=torch.as_tensor(op["dy"]).to(dev), x=torch.as_tensor(op["x"]).to(dev), wt=torch.as_tensor(E.to_koc(op["w"])).to(dev))
    if op["x8"] is not None:
        d["x8"] = torch.as_tensor(op["x8"]).to(dev)
    return d


def _run_bwd(layer, u8, batch, variant, t, coef, dev, xact, what):
    """t: device operands (dy, x / x8, wt).  -> dict(n_slabs, slabs: the guarded slab buffer, dx: the guarded dX buffer or None)"""
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, stream_ptr
    c, h, oc, k, s = E.GEOM[layer]
    n = ctypes.c_int(-1)
    rc = lib.dra_conv_wgrad_slabs.raw(layer, batch, E.KSPLIT, int(variant), ctypes.byref(n))
    assert rc == 0 and n.value == E.wgrad_slabs(layer, batch, E.KSPLIT, variant), "%s: dra_conv_wgrad_slabs gives %d (rc %d), the restatement %r" % (
        what, n.value, rc, E.wgrad_slabs(layer, batch, E.KSPLIT, variant))
    stride, kk = E.slab_stride(layer), E.k_of(layer)
    slabs = _Buf((n.value + EXTRA_SLABS) * stride, dev)
    dx = _Buf(batch * c * h * h, dev) if layer > 1 else None
    x = t["x8"] if u8 else t["x"]
    rc = lib.dra_conv_bwd_fused.raw(layer, _p(t["dy"]), _p(x), _p(t["wt"]) if layer > 1 else None, _p(t["x"]) if (xact and layer > 1) else None,
                                    slabs.ptr(), ctypes.c_void_p(slabs.v.data_ptr() + 4 * oc * kk), stride, E.KSPLIT, _p(dx), batch, int(u8),
                                    float(coef if u8 else 1.0), ops.ACT["relu"], int(variant), stream_ptr())
    _sync()
    assert rc == 0, "%s: dra_conv_bwd_fused returned %d" % (what, rc)
    slabs.sentinels_intact(what + " slabs")
    slabs.written(what + " slabs", n.value * stride)
    slabs.untouched(what + ": a slab beyond the count", n.value * stride)
    if dx is not None:
        dx.sentinels_intact(what + " dx")
        dx.written(what + " dx")
    return dict(n_slabs=n.value, slabs=slabs, dx=dx)


def _fold(layer, r, dev, what):
    """The slab fold of production (dra_grad_sqnorm_segs) into a guarded gradient segment -> (dW [OC, C, KH, KW], db) as numpy."""
    from deeprl_amd import ops
    oc, kk = E.GEOM[layer][2], E.k_of(layer)
    seg = oc * kk + oc
    grad = _Buf(seg, dev, np.zeros(seg, dtype=np.float32))
    partials = torch.zeros(ops.norm_partials_max(), dtype=torch.float64, device=dev)
    ops.grad_sqnorm_segs(grad.v, [(0, seg, r["slabs"].v, E.slab_stride(layer), r["n_slabs"])], partials)
    _sync()
    grad.sentinels_intact(what + " folded gradient")
    g = grad.v.cpu().numpy()
    return E.from_koc(g[:oc * kk], layer), g[oc * kk:]


@pytest.mark.parametrize("c", E.BWD_CASES, ids=_ids(E.BWD_CASES))
def test_conv_bwd_edges(dev, c):
    layer, u8, batch, variant = c["layer"], c["u8"], c["batch"], c["variant"]
    figs = _Figures(c["name"])
    for kind in ("random", "integer"):
        op, t = E.bwd_operands(layer, batch, kind), _bwd_device(layer, batch, kind, dev)
        what = c["name"] + " " + kind
        r = _run_bwd(layer, u8, batch, variant, t, op["coef"], dev, True, what)
        assert r["n_slabs"] == c["reaches"]["n_slabs"]
        dw, db = _fold(layer, r, dev, what)
        judge = figs.add if kind == "random" else figs.exact
        pre = "" if kind == "random" else "integer "
        judge(pre + "dw", dw, op["dw"])
        judge(pre + "db", db, op["db"])
        shape = (batch,) + E.GEOM[layer][:1] + (E.GEOM[layer][1],) * 2
        if layer > 1:
            judge(pre + "dx masked", r["dx"].v.cpu().numpy().reshape(shape), op["dx"] * (op["x"] > 0))
        again = _run_bwd(layer, u8, batch, variant, t, op["coef"], dev, True, what + " second launch")
        n = r["n_slabs"] * E.slab_stride(layer)
        assert torch.equal(again["slabs"].v[:n], r["slabs"].v[:n]), what + ": the second launch differs in the slabs"
        if layer > 1:
            assert torch.equal(again["dx"].v, r["dx"].v), what + ": the second launch differs in dx"
            plain = _run_bwd(layer, u8, batch, variant, t, op["coef"], dev, False, what + " without xact")
            judge(pre + "dx", plain["dx"].v.cpu().numpy().reshape(shape), op["dx"])
            assert torch.equal(plain["slabs"].v[:n], r["slabs"].v[:n]), what + ": the slabs depend on xact"
    figs.done()


SCATTER_PAIRS = [(2, 256), (2, 768), (3, 256), (3, 512)]


@pytest.mark.parametrize("layer,batch", SCATTER_PAIRS)
def test_weight_gradient_slabs_do_not_depend_on_the_scatter_bit(dev, layer, batch):
    """The scatter form replaces the input-gradient role only: the weight-gradient role and so its slabs are the same, in one launch or two."""
    op, t = E.bwd_operands(layer, batch, "random"), _bwd_device(layer, batch, "random", dev)
    runs = {v: _run_bwd(layer, False, batch, E.VARIANTS[v], t, 1.0, dev, True, "L%d b%d %s" % (layer, batch, v)) for v in ("oo", "oo-s", "oo-fs")}
    n = runs["oo"]["n_slabs"] * E.slab_stride(layer)
    assert {E.bwd_path(layer, False, batch, E.VARIANTS[v])["wgrad"] for v in runs} == {"WG%d%s" % (layer, "p" if batch >= E.PERSIST_FROM[layer] else "l")}
    for v in ("oo-s", "oo-fs"):
        assert runs[v]["n_slabs"] == runs["oo"]["n_slabs"]
        assert torch.equal(runs[v]["slabs"].v[:n], runs["oo"]["slabs"].v[:n]), "conv%d batch %d: the slabs of %s are not those without the scatter bit" % (layer, batch, v)


@pytest.mark.parametrize("layer,batch,variant,form", E.BWD_INDEPENDENCE, ids=["L%d-b%d-%s" % (l, b, f) for l, b, _, f in E.BWD_INDEPENDENCE])
def test_input_gradient_batch_independence(dev, layer, batch, variant, form):
    assert E.dgrad_role(E.bwd_path(layer, False, batch, variant)) == form
    rs = E._rs("independence bwd", layer, batch)
    c, h, oc, k, s = E.GEOM[layer]
    w, _ = E.draw_weights(rs, layer, "random")
    _, x, _ = E.draw_input(rs, layer, batch, "random")
    o = E.out_hw(layer)
    dy = rs.standard_normal((batch, oc, o, o)).astype(np.float32)
    j = (batch // 2) | 1
    dy2 = dy.copy()
    dy2[j] = 2.0 * dy[j] + 1.0
    t = dict(dy=torch.as_tensor(dy).to(dev), x=torch.as_tensor(x).to(dev), wt=torch.as_tensor(E.to_koc(w)).to(dev))
    x2 = x.copy()
    x2[j] = np.maximum(1.0 - x[j], 0)                      # ... and its mask
    t2 = dict(t, dy=torch.as_tensor(dy2).to(dev), x=torch.as_tensor(x2).to(dev))
    a = _run_bwd(layer, False, batch, variant, t, 1.0, dev, True, "independence")["dx"].v.view(batch, -1)
    b = _run_bwd(layer, False, batch, variant, t2, 1.0, dev, True, "independence, changed")["dx"].v.view(batch, -1)
    others = [i for i in range(batch) if i != j]
    assert torch.equal(a[others], b[others]), "conv%d batch %d %s: changing sample %d changed another sample's dX rows" % (layer, batch, form, j)
    assert not torch.equal(a[j], b[j])


# --------------------------------------------------------------------------------------------- dra_conv1_fwd_koc_ring
@pytest.mark.parametrize("newest,age", E.RING_CASES, ids=["newest%d-age%s" % (n, "null" if a is None else a) for n, a in E.RING_CASES])
def test_conv1_ring_forward_gathers_its_stack(dev, newest, age):
    """The actor's conv1 reading its 4-frame stack from ring slots (wrapping below slot 0, older channels clamped to newest - age)
    against the plain NCHW forward of the stack gathered on the host: the same kernel, bit for bit."""
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, stream_ptr
    rs = E._rs("ring", newest, age)
    w, b = E.draw_weights(rs, 1, "random")
    frames = rs.randint(0, 256, size=(E.RING_CAPACITY, 84, 84)).astype(np.uint8)
    assert len({f.tobytes() for f in frames}) == E.RING_CAPACITY
    stack = frames[E.ring_stack_slots(newest, age)][None]
    st = _Fwd(1, True, [stack], [w], [b], 1.0 / 255, dev)
    fr = torch.as_tensor(frames).to(dev)
    slot = torch.tensor([newest], dtype=torch.int64, device=dev)
    age_dev = None if age is None else torch.tensor([age], dtype=torch.int32, device=dev)
    for act in ("relu", None):
        want = st.run(act, what="ring reference")[0]
        y = _Buf(want.numel(), dev)
        rc = lib.dra_conv1_fwd_koc_ring.raw(_p(fr), _p(slot), _p(age_dev), E.RING_CAPACITY, _p(st.wt[0]), _p(st.b[0]), y.ptr(), 1.0 / 255, ops.ACT[act],
                                            stream_ptr())
        _sync()
        assert rc == 0
        y.sentinels_intact("ring y")
        y.written("ring y")
        assert torch.equal(y.v.view_as(want), want), "newest %d, age %r (%s): not the forward of slots %r" % (newest, age, act, E.ring_stack_slots(newest, age))
    # a ring shorter than the stack is refused
    y = _Buf(32 * 400, dev)
    assert lib.dra_conv1_fwd_koc_ring.raw(_p(fr), _p(slot), _p(age_dev), 3, _p(st.wt[0]), _p(st.b[0]), y.ptr(), 1.0 / 255, 1, stream_ptr()) == EINVAL
    _sync()
    y.untouched("a refused ring forward's output")


# ------------------------------------------------------------------------------------------------- dra_transpose_f32
@pytest.mark.parametrize("rows,cols", E.TRANSPOSE_SHAPES)
def test_transpose_edges(dev, rows, cols):
    from deeprl_amd._lib import lib, stream_ptr
    a = E._rs("transpose", rows, cols).standard_normal((rows, cols)).astype(np.float32)
    src, out = _Buf(rows * cols, dev, a), _Buf(rows * cols, dev)
    assert lib.dra_transpose_f32.raw(src.ptr(), out.ptr(), rows, cols, stream_ptr()) == 0
    _sync()
    out.sentinels_intact("transpose")
    out.written("transpose")
    assert torch.equal(out.v.view(cols, rows), src.v.view(rows, cols).T)
    refused = _Buf(rows * cols, dev)
    rcs = [lib.dra_transpose_f32.raw(None, refused.ptr(), rows, cols, stream_ptr()), lib.dra_transpose_f32.raw(src.ptr(), None, rows, cols, stream_ptr()),
           lib.dra_transpose_f32.raw(src.ptr(), refused.ptr(), 0, cols, stream_ptr()), lib.dra_transpose_f32.raw(src.ptr(), refused.ptr(), rows, 0, stream_ptr())]
    _sync()
    assert rcs == [EINVAL] * 4
    refused.untouched("a refused transpose's output")


# ---------------------------------------------------------------------------------------------------------- refusals
def test_argument_limits_are_refused_before_any_launch(dev):
    """Every argument check of the entry points, through .raw: DRA_EINVAL, nothing launched -- the buffers are real and large enough
    for the launch each call describes, and the NaN-filled outputs keep their bits."""
    from deeprl_amd._lib import lib, stream_ptr
    s = stream_ptr()
    refused, outs = {}, []
    batch, nmax = 2, E.MAX_Z + 1
    for layer in (1, 2, 3):
        c, h, oc, k, _ = E.GEOM[layer]
        o = E.out_hw(layer)
        x = [torch.zeros((batch, c, h, h), dtype=torch.float32, device=dev) for _ in range(nmax)]        # (large enough as uint8 too)
        wt = [torch.zeros((c * k * k, oc), dtype=torch.float32, device=dev) for _ in range(nmax)]
        bias = [torch.zeros(oc, dtype=torch.float32, device=dev) for _ in range(nmax)]
        y = [_Buf(batch * oc * o * o, dev) for _ in range(nmax)]
        outs += y

        def fwd(layer=layer, nz=2, xs=_parr(x), wp=_parr(wt), bp=_parr(bias), yp=_parr(y), batch=batch, u8=0):
            return lib.dra_conv_fwd_koc.raw(layer, nz, xs, wp, bp, yp, batch, u8, 1.0, 1, s)

        L = "fwd conv%d: " % layer
        refused.update({
            L + "nz = 0": fwd(nz=0), L + "nz = DRA_MAX_Z + 1": fwd(nz=nmax), L + "batch 0": fwd(batch=0), L + "no x array": fwd(xs=None),
            L + "no wt array": fwd(wp=None), L + "no bias array": fwd(bp=None), L + "no y array": fwd(yp=None),
            L + "x[1] null": fwd(xs=_parr([x[0], None])), L + "wt[1] null": fwd(wp=_parr([wt[0], None])),
            L + "bias[0] null": fwd(bp=_parr([None, bias[1]])), L + "y[1] null": fwd(yp=_parr([y[0], None])),
        })
        if layer > 1:
            refused[L + "uint8 input"] = fwd(u8=1)
        if layer == 1:
            refused.update({"fwd layer 0": fwd(layer=0), "fwd layer 4": fwd(layer=4)})
        # backward
        dy = torch.zeros((batch, oc, o, o), dtype=torch.float32, device=dev)
        stride = E.slab_stride(layer)
        slabs, dx = _Buf(E.KSPLIT * 5 * stride, dev), _Buf(batch * c * h * h, dev)
        outs += [slabs, dx]

        def bwd(layer=layer, dyp=_p(dy), xp=_p(x[0]), wp=_p(wt[0]), dwp=slabs.ptr(), dbp=ctypes.c_void_p(slabs.v.data_ptr() + 4 * oc * c * k * k),
                ks=E.KSPLIT, dxp=dx.ptr(), batch=batch, u8=0, variant=E.OO):
            return lib.dra_conv_bwd_fused.raw(layer, dyp, xp, wp, None, dwp, dbp, stride, ks, dxp, batch, u8, 1.0, 1, variant, s)

        L = "bwd conv%d: " % layer
        refused.update({L + "no dy": bwd(dyp=None), L + "no x": bwd(xp=None), L + "no dw": bwd(dwp=None), L + "no db": bwd(dbp=None),
                        L + "batch 0": bwd(batch=0), L + "ksplit 0": bwd(ks=0)})
        if layer > 1:
            refused.update({L + "uint8 input": bwd(u8=1), L + "no wt": bwd(wp=None), L + "no dx": bwd(dxp=None)})
            assert E.bwd_path(layer, True, batch, E.OO) is None
        if layer == 2:
            refused.update({"bwd layer 0": bwd(layer=0), "bwd layer 4": bwd(layer=4), "bwd layer 4, split-K": bwd(layer=4, variant=0)})
    n = ctypes.c_int(-7)
    refused.update({"slabs: layer 0": lib.dra_conv_wgrad_slabs.raw(0, 32, 16, E.OO, ctypes.byref(n)),
                    "slabs: layer 4": lib.dra_conv_wgrad_slabs.raw(4, 32, 16, E.OO, ctypes.byref(n)),
                    "slabs: batch 0": lib.dra_conv_wgrad_slabs.raw(1, 0, 16, E.OO, ctypes.byref(n)),
                    "slabs: ksplit 0": lib.dra_conv_wgrad_slabs.raw(1, 32, 0, E.OO, ctypes.byref(n)),
                    "slabs: no result": lib.dra_conv_wgrad_slabs.raw(1, 32, 16, E.OO, None)})
    _sync()
    assert n.value == -7, "a refused dra_conv_wgrad_slabs wrote its result"
    assert E.wgrad_slabs(0, 32, 16, E.OO) is None and E.wgrad_slabs(1, 0, 16, E.OO) is None and E.fwd_path(2, True, 2, 1, N_CU) == ("refused",)
    wrong = {k: rc for k, rc in refused.items() if rc != EINVAL}
    assert not wrong, "expected DRA_EINVAL (%d): %s" % (EINVAL, wrong)
    for b in outs:
        b.untouched("a refused call's output")


def test_restated_constants_match_the_library(dev):
    from deeprl_amd import ops
    assert (E.FUSED, E.ODGRAD, E.OWGRAD, E.SCATTER) == (ops.VAR_FUSED_BWD, ops.VAR_ONESHOT_DGRAD, ops.VAR_ONESHOT_WGRAD, ops.VAR_DGRAD_SCATTER)
    assert E.GEOM == ops._CONV_GEOM and E.MAX_BATCH > 1024        # 1025 is above nets._ONESHOT_WGRAD_MAX_BATCH's default
