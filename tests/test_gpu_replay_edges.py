"""Edge-shape parity of the replay data path -- csrc/ring.hip, csrc/sumtree.hip and the stand-alone launch of csrc/per_chain2.h --
against the references of tests/replay_edge_cases.py, through deeprl_amd.ops or, where ops has no wrapper (or a test needs its
own output buffers), the C ABI.  tests/test_replay_edge_cases_host.py proves on the CPU that every case reaches the path it is
named for and that these inputs tell a subtly wrong kernel from a right one.

Everything is compared BIT FOR BIT (floats through their integer views) except priorities that went through powf and the
importance weights: rtol 1e-6 against float64 pow rounded to float32, their measured maxima going to the parity log.  Every
gather output has 64 bytes of 0xA5 behind it that must be unchanged after the launch; the table kernels' outputs NaN slack.
Cases that share a ring or tree shape run on one handle; gathers run twice (determinism)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import replay_edge_cases as E
from oracle.numerics_oracle import image_lut, image_normalize_sync
from parity_log import record_parity

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


def _ids(cases):
    return [c["name"] for c in cases]


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


class _Out:
    """nbytes of output with SLACK bytes of 0xA5 behind (offset: bytes in front, for a misaligned pointer)."""

    def __init__(self, nbytes, dev, offset=0):
        self.nbytes, self.offset = int(nbytes), offset
        self.buf = torch.full((offset + self.nbytes + E.SLACK,), E.SLACK_BYTE, dtype=torch.uint8, device=dev)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + offset)

    def get(self, dtype=np.uint8):
        host = self.buf.cpu().numpy()
        assert (host[:self.offset] == E.SLACK_BYTE).all() and (host[self.offset + self.nbytes:] == E.SLACK_BYTE).all(), "bytes outside the output changed"
        return host[self.offset:self.offset + self.nbytes].copy().view(dtype)


def _filled_ring(d, case, dev):
    """The case's ring with all of RingContents put into it in one dra_ring_put; returns (ring, contents)."""
    c = E.RingContents(case["capacity"], case["frame_bytes"], case["action_bytes"], case["seed"], case.get("rewards"), case.get("masks"))
    ring = d.ops.Ring(c.capacity, c.frame_bytes, c.action_bytes, case["history"], case["n_step"], case["discount"])
    ring.put_device(0, _t(c.frames.ravel(), dev), actions=_t(c.actions.ravel(), dev), rewards=_t(c.rewards, dev), masks=_t(c.masks, dev),
                    count=c.capacity)
    return ring, c


def _gather(lib, ring, case, idx, dev, block, misaligned=False):
    b, h, n, fb, ab = len(idx), case["history"], case["n_step"], case["frame_bytes"], case["action_bytes"]
    off = 8 if misaligned else 0
    idx_t = _t(idx, dev)
    o = dict(action=_Out(b * ab, dev), reward=_Out(8 * b, dev), mask=_Out(4 * b, dev), reward_f32=_Out(4 * b, dev), mask_f32=_Out(4 * b, dev))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if block:
        o["block"] = _Out(b * (h + n) * fb, dev, off)
        lib.dra_ring_gather_block(ring.h, ctypes.c_void_p(idx_t.data_ptr()), b, o["block"].ptr, o["action"].ptr, o["reward"].ptr, o["mask"].ptr,
                                  o["reward_f32"].ptr, o["mask_f32"].ptr, stream)
    else:
        o["state"], o["next_state"] = _Out(b * h * fb, dev, off), _Out(b * h * fb, dev, off)
        lib.dra_ring_gather(ring.h, ctypes.c_void_p(idx_t.data_ptr()), b, o["state"].ptr, o["next_state"].ptr, o["action"].ptr, o["reward"].ptr,
                            o["mask"].ptr, o["reward_f32"].ptr, o["mask_f32"].ptr, stream)
    torch.cuda.synchronize()
    types = dict(reward=np.float64, mask=np.int32, reward_f32=np.float32, mask_f32=np.float32)
    return {k: v.get(types.get(k, np.uint8)) for k, v in o.items()}


def _check_gather(got, want, what):
    for k, g in got.items():
        w = np.ascontiguousarray(want[k])
        assert np.array_equal(_bits(g).ravel(), _bits(w).ravel()), "%s: %s" % (what, k)


# ================================================================================================ ring gather
_GATHER = E.GATHER_CASES + E.FOLD_CASES


@pytest.mark.parametrize("case", _GATHER, ids=_ids(_GATHER))
def test_gather_edge_shapes(dra, case):
    from deeprl_amd._lib import lib
    dev = dra.Config.DEVICE
    ring, c = _filled_ring(dra, case, dev)
    try:
        idx = case["idx"] if "idx" in case else E.gather_indices(case["capacity"], case["history"], case["n_step"], case["batch"], case["seed"])
        want = E.ref_gather(c, idx, case["history"], case["n_step"], case["discount"])
        with np.errstate(over="ignore"):
            assert np.array_equal(_bits(want["reward_f32"]), _bits(want["reward"].astype(np.float32)))
        for block in (False, True):
            for rep in range(2):
                got = _gather(lib, ring, case, idx, dev, block, case.get("misaligned", False))
                _check_gather(got, want, "%s block=%d run %d" % (case["name"], block, rep))
    finally:
        ring.close()


@pytest.mark.parametrize("case", E.STREAM_CASES, ids=_ids(E.STREAM_CASES))
def test_gather_streaming_threshold(dra, case):
    """One launch on either side of the 256 MiB output threshold (and the block form at its own): the nontemporal-store
    variant writes what the cached one writes.  Compared on the host in chunks."""
    from deeprl_amd._lib import lib
    dev = dra.Config.DEVICE
    ring, c = _filled_ring(dra, case, dev)
    try:
        h, n, fb, b = case["history"], case["n_step"], case["frame_bytes"], case["batch"]
        idx = E.gather_indices(case["capacity"], h, n, b, 3)
        got = _gather(lib, ring, case, idx, dev, case["block"])
        small = E.ref_gather(c, idx, h, n, case["discount"])
        for k in ("action", "reward", "mask", "reward_f32", "mask_f32"):
            assert np.array_equal(_bits(got[k]).ravel(), _bits(np.ascontiguousarray(small[k])).ravel()), k
        run = idx[:, None] - h + 1 + np.arange(h + n)[None, :]
        for s in range(0, b, 256):
            blk = c.frames[run[s:s + 256]]
            if case["block"]:
                assert np.array_equal(got["block"].reshape(b, h + n, fb)[s:s + 256], blk), s
            else:
                assert np.array_equal(got["state"].reshape(b, h, fb)[s:s + 256], blk[:, :h]), s
                assert np.array_equal(got["next_state"].reshape(b, h, fb)[s:s + 256], blk[:, n:]), s
    finally:
        ring.close()


# ================================================================================================ ring put
def _ring_arrays(ring):
    f, a, r, m = ring.arrays()
    torch.cuda.synchronize()
    return (f.cpu().numpy().reshape(ring.capacity, -1), a.cpu().numpy().reshape(ring.capacity, -1), r.cpu().numpy(), m.cpu().numpy())


@pytest.mark.parametrize("ab", E.PUT_ACTION_BYTES)
def test_put_edge_shapes(dra, ab):
    """dra_ring_put with count 1 / 7 / capacity ending exactly at the capacity, array and by-value action / reward / mask, a
    frame source one byte off alignment, action records of 1 .. 264 bytes (stored AND gathered whole), the argument checks."""
    from deeprl_amd._lib import lib
    dev = dra.Config.DEVICE
    cap, fb = E.PUT_CAP, 32
    ring = dra.ops.Ring(cap, fb, ab, 1, 1, 0.99)
    try:
        held = [np.zeros((cap, fb), np.uint8), np.zeros((cap, ab), np.uint8), np.zeros(cap), np.zeros(cap, np.int32)]
        ring.put_device(0, torch.zeros(cap * fb, dtype=torch.uint8, device=dev), actions=torch.zeros(cap * ab, dtype=torch.uint8, device=dev),
                        rewards=torch.zeros(cap, dtype=torch.float64, device=dev), masks=torch.zeros(cap, dtype=torch.int32, device=dev), count=cap)
        for k, count in enumerate(E.PUT_COUNTS):
            c = E.RingContents(count, fb, ab, 10 * ab + k)
            slot0 = cap - count
            src = torch.zeros(1 + count * fb, dtype=torch.uint8, device=dev)
            src[1:] = _t(c.frames.ravel(), dev)
            frames = src[1:] if k == 1 else _t(c.frames.ravel(), dev)        # count 7: the byte path by a misaligned source
            assert (frames.data_ptr() % 16 != 0) == (k == 1)
            ring.put_device(slot0, frames, actions=_t(c.actions.ravel(), dev), rewards=_t(c.rewards, dev), masks=_t(c.masks, dev), count=count)
            held[0][slot0:], held[1][slot0:], held[2][slot0:], held[3][slot0:] = c.frames, c.actions, c.rewards, c.masks
            for got, want in zip(_ring_arrays(ring), held):
                assert np.array_equal(_bits(got), _bits(want)), (ab, count)
        if ab <= 8:        # by value: the little-endian bytes of the int64, one reward, one mask for every slot of the put
            c = E.RingContents(7, fb, ab, 99)
            val = 0x1122334455667788
            ring.put_device(2, _t(c.frames.ravel(), dev), action_val=val, reward_val=-1.0 / 3.0, mask_val=0, count=7)
            held[0][2:9], held[1][2:9], held[2][2:9], held[3][2:9] = c.frames, E.action_from_value(val, ab), -1.0 / 3.0, 0
            for got, want in zip(_ring_arrays(ring), held):
                assert np.array_equal(_bits(got), _bits(want)), (ab, "by value")
        else:              # no action source for a record that does not fit the by-value int64: refused before any launch
            rc = lib.dra_ring_put.raw(ring.h, 0, 1, ctypes.c_void_p(frames.data_ptr()), None, 0, None, 0.0, None, 1, None)
            assert rc == EINVAL
        rc = lib.dra_ring_put.raw(ring.h, cap - 3, 4, ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(frames.data_ptr()), 0, None, 0.0, None, 1,
                                  None)
        assert rc == EINVAL        # slot0 + count > capacity
        # the gather returns the whole record
        case = dict(history=1, n_step=1, frame_bytes=fb, action_bytes=ab)
        idx = np.arange(0, cap - 1, dtype=np.int64)
        got = _gather(lib, ring, case, idx, dev, block=False)
        assert np.array_equal(got["action"].reshape(len(idx), ab), held[1][idx]), ab
        # the host feed stages the same record (its put kernel reads the pinned slot)
        c = E.RingContents(3, fb, ab, 5 * ab)
        for s in range(3):
            ring.put_host(4 + s, c.frames[s], c.actions[s], float(c.rewards[s]), int(c.masks[s]))
        held[0][4:7], held[1][4:7], held[2][4:7], held[3][4:7] = c.frames, c.actions, c.rewards, c.masks
        for got, want in zip(_ring_arrays(ring), held):
            assert np.array_equal(_bits(got), _bits(want)), (ab, "put_host")
    finally:
        ring.close()


def test_put_host_wraps_its_staging_ring_twice(dra):
    """130 consecutive host feeds of distinct 7056-byte frames with no synchronisation in between (the 64-slot pinned staging
    ring wraps twice; a slot must not be reused before its kernel has read it), then one read-back."""
    cap = 64
    ring = dra.ops.Ring(cap, E.PUT_HOST_FRAME, 8, 1, 1, 0.99)
    try:
        assert E.PUT_HOST_FEEDS > 2 * E.STAGE_SLOTS
        c = E.RingContents(E.PUT_HOST_FEEDS, E.PUT_HOST_FRAME, 8, 1)
        for t in range(E.PUT_HOST_FEEDS):
            ring.put_host(t % cap, c.frames[t], c.actions[t], float(c.rewards[t]), int(c.masks[t]))
        last = np.asarray([max(t for t in range(E.PUT_HOST_FEEDS) if t % cap == s) for s in range(cap)])
        for got, want in zip(_ring_arrays(ring), (c.frames[last], c.actions[last], c.rewards[last], c.masks[last])):
            assert np.array_equal(_bits(got), _bits(want))
    finally:
        ring.close()


def test_put_rows_wraps_exactly_the_capacity(dra):
    dev = dra.Config.DEVICE
    cap, fb = 8, 48
    ring = dra.ops.Ring(cap, fb, 8, 1, 1, 0.99)
    try:
        c = E.RingContents(cap, fb, 8, 2)
        ring.put_rows(cap, _t(c.frames.ravel(), dev), fb, _t(c.actions.view("<i8").ravel(), dev), _t(c.rewards, dev), _t(c.masks, dev), slot0=3)
        order = (np.arange(cap) - 3) % cap         # slot s holds transition (s - 3) mod capacity
        for got, want in zip(_ring_arrays(ring), (c.frames[order], c.actions[order], c.rewards[order], c.masks[order])):
            assert np.array_equal(_bits(got), _bits(want))
    finally:
        ring.close()


# ================================================================================================ table kernels, row gather
def test_u8_lut_edge_sizes(dra):
    """dra_u8_to_f32_lut below one vector, around it, and past its 2048-block grid cap with a tail (one launch each), against
    the reference's uint8 -> float64 / 255 -> float32; NaN slack behind the output stays."""
    from deeprl_amd._lib import lib
    dev = dra.Config.DEVICE
    lut = _t(image_lut(), dev)
    for n in E.LUT_N:
        x = E.lut_input(n)
        out = torch.full((n + 16,), float("nan"), dtype=torch.float32, device=dev)
        lib.dra_u8_to_f32_lut(dra.ops.ptr(_t(x, dev)), dra.ops.ptr(out), n, dra.ops.ptr(lut), None)
        got = out.cpu().numpy()
        assert np.array_equal(_bits(got[:n]), _bits(image_normalize_sync(x))) and np.isnan(got[n:]).all(), n
        if n <= 4097:
            assert np.array_equal(_bits(dra.ops.u8_to_f32(_t(x, dev), lut).cpu().numpy()), _bits(image_normalize_sync(x))), n


def test_u8_lut_rows_and_dispatch(dra):
    from deeprl_amd._lib import lib
    dev = dra.Config.DEVICE
    lut = _t(image_lut(), dev)
    for c in E.LUT_ROWS:
        rows, elems, stride = c["rows"], c["elems"], c["stride"]
        x = E.lut_input(rows * stride).reshape(rows, stride)
        x_t = _t(x, dev)
        out = torch.full((rows * elems + 16,), float("nan"), dtype=torch.float32, device=dev)
        lib.dra_u8_to_f32_lut_rows(dra.ops.ptr(x_t), dra.ops.ptr(out), rows, elems, stride, dra.ops.ptr(lut), None)
        got = out.cpu().numpy()
        want = image_normalize_sync(x[:, :elems])
        assert np.array_equal(_bits(got[:rows * elems]), _bits(want).ravel()) and np.isnan(got[rows * elems:]).all(), c
        if stride > elems:      # ops.u8_to_f32 takes the rows kernel for this view
            assert np.array_equal(_bits(dra.ops.u8_to_f32(x_t[:, :elems], lut).cpu().numpy()), _bits(want)), c
    # a view whose row stride is no multiple of 16: the contiguous-copy path, same values
    x = E.lut_input(3 * 20).reshape(3, 20)
    view = _t(x, dev)[:, :16]
    assert not view.is_contiguous() and view.stride(0) % 16 != 0
    assert np.array_equal(_bits(dra.ops.u8_to_f32(view, lut).cpu().numpy()), _bits(image_normalize_sync(x[:, :16])))


def test_gather_rows_edge_shapes(dra):
    from deeprl_amd._lib import lib
    dev = dra.Config.DEVICE
    rows = E.GATHER_ROWS_SRC
    idx = np.asarray(E.GATHER_ROWS_IDX, dtype=np.int64)
    rs = np.random.RandomState(4)
    src = [rs.randint(0, 256, size=(rows, rb)).astype(np.uint8) for rb in E.GATHER_ROWS_BYTES]
    # 1 field, then 8 fields (every row size twice; the second 4096-byte one read from a source 8 bytes off alignment)
    outs = dra.ops.gather_rows([_t(src[0], dev)], _t(idx, dev))
    assert np.array_equal(outs[0].cpu().numpy(), src[0][idx])
    off = torch.zeros(8 + rows * 4096, dtype=torch.uint8, device=dev)
    off[8:] = _t(src[0].ravel(), dev)
    mis = off[8:].view(rows, 4096)
    assert mis.is_contiguous() and mis.data_ptr() % 16 == 8
    fields = [_t(s, dev) for s in src] + [mis] + [_t(s, dev) for s in src[1:]]
    assert len(fields) == 8
    outs = dra.ops.gather_rows(fields, _t(idx, dev))
    for o, w in zip(outs, src + [src[0]] + src[1:]):
        assert np.array_equal(o.cpu().numpy(), w[idx]), w.shape
    with pytest.raises(ValueError):
        dra.ops.gather_rows(fields + [fields[0]], _t(idx, dev))
    nine = fields + [fields[0]]
    outs9 = [torch.empty((len(idx),) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in nine]
    rc = lib.dra_gather_rows.raw(9, (ctypes.c_void_p * 9)(*[t.data_ptr() for t in nine]), (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs9]),
                                 (ctypes.c_int64 * 9)(*[t.shape[1] for t in nine]), dra.ops.ptr(_t(idx, dev)), len(idx), rows, None)
    assert rc == EINVAL


# ================================================================================================ sum tree
def _device_tree(d, orc_tree, cap):
    tree = d.ops.SumTree(cap)
    tree.as_tensor().copy_(torch.from_numpy(np.ascontiguousarray(orc_tree)))
    return tree


def _tree_bits(tree):
    torch.cuda.synchronize()
    return _bits(tree.as_tensor().cpu().numpy())


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
@pytest.mark.parametrize("cap,n", E.update_cases(), ids=["cap%d_n%d" % cn for cn in E.update_cases()])
def test_tree_update_many_leaves(dra, cap, n, ordered):
    dev = dra.Config.DEVICE
    orc = E.filled_oracle(cap, cap)
    tree = _device_tree(dra, orc.tree, cap)
    try:
        leaves, prio = E.update_inputs(cap, n, ordered)
        E.oracle_updates(orc, leaves, prio)
        tree.update(_t(leaves, dev), _t(prio, dev), ordered=ordered)
        assert np.array_equal(_tree_bits(tree), _bits(orc.tree))
        if not ordered:        # the exactness regime: the heap is left + right everywhere, on the device's rebuild too
            assert np.array_equal(_bits(orc.rebuilt()), _bits(orc.tree))
            tree.rebuild()
            assert np.array_equal(_tree_bits(tree), _bits(orc.tree))
    finally:
        tree.close()


@pytest.mark.parametrize("cap", E.TREE_CAPS)
def test_tree_adds_follow_the_oracle(dra, cap):
    """set / set_from / set_many_from against a sequence of oracle.add: a wrapping run of single adds, then 64 adds (every
    leaf below 64) in one launch that wraps at the capacity, level-parallel (stat given) and as ordered delta walks (no stat).
    Both launches run inside the exactness regime, where the two branches give the same bits: this test holds each to the
    oracle but cannot tell which one ran; that the branch follows `stat` is what test_adds_after_the_unforced_ordered_fallback
    shows (there the level-parallel branch would leave the oracle's values)."""
    from deeprl_amd._lib import lib
    dev = dra.Config.DEVICE
    orc = E.TreeRef(cap)
    tree = dra.ops.SumTree(cap)
    try:
        rs = np.random.RandomState(cap)
        for k, p in enumerate(E.f32_priorities(rs, cap + 3 if cap < 64 else 70)):
            leaf = orc.write + cap - 1
            orc.add(float(p))
            if k % 2:
                tree.set_from(leaf, _t(np.asarray([p]), dev))
            else:
                tree.set(leaf, float(p))
        assert np.array_equal(_tree_bits(tree), _bits(orc.tree))
        write0, n = E.many_add_plan(cap)
        for with_stat in (True, False):
            p = float(E.f32_priorities(rs, 1)[0])
            leaves = orc.tree[cap - 1:]
            stat = _t(np.asarray([max(p, leaves.max()), min(p, leaves[leaves > 0].min())]), dev)
            orc.write = write0
            for _ in range(n):
                orc.add(p)
            tree.set_many_from(write0, n, _t(np.asarray([p]), dev), stat=stat if with_stat else None)
            assert np.array_equal(_tree_bits(tree), _bits(orc.tree)), with_stat
        pd = dra.ops.ptr(stat)
        assert lib.dra_sumtree_set_many_from.raw(tree.h, 0, 65, pd, pd, None) == EINVAL
        assert lib.dra_sumtree_set_many_from.raw(tree.h, cap, 1, pd, pd, None) == EINVAL
    finally:
        tree.close()


def test_tree_commit_f32(dra):
    """commit_f32: n = 0 (only stat moves), n < batch through a permuted pos, n = batch = 1024, force_ordered; stat is the
    running {max, min} over every OFFERED priority, written or not."""
    dev = dra.Config.DEVICE
    cap = 1025
    orc = E.filled_oracle(cap, 3)
    tree = _device_tree(dra, orc.tree, cap)
    try:
        rs = np.random.RandomState(8)
        hi, lo = float(orc.tree[cap - 1:].max()), float(orc.tree[cap - 1:].min())
        stat = _t(np.asarray([hi, lo]), dev)
        plans = [(0, 7, False), (5, 9, False), (1024, 1024, False), (33, 64, True), (0, 1, False)]
        for k, (n, batch, force) in enumerate(plans):
            prio = E.f32_priorities(rs, batch).astype(np.float32)
            if k == 0:
                prio[3], prio[5] = np.float32(9.0), np.float32(2.0 ** -4)        # offered, not written: stat still moves
            pos = rs.permutation(batch)[:n].astype(np.int32)
            leaves = (rs.permutation(cap)[:n] + cap - 1).astype(np.int64)
            hi, lo = max(hi, float(prio.max())), min(lo, float(prio.min()))
            assert E.exact_regime(cap, hi, lo)
            E.oracle_updates(orc, leaves, prio[pos].astype(np.float64))
            tree.commit_f32(_t(leaves, dev) if n else None, _t(pos, dev) if n else None, _t(prio, dev), stat, force_ordered=force)
            assert np.array_equal(_tree_bits(tree), _bits(orc.tree)), k
            assert stat.cpu().tolist() == [hi, lo], k
    finally:
        tree.close()


@pytest.mark.parametrize("cap", E.FALLBACK_CAPS)
def test_adds_after_the_unforced_ordered_fallback(dra, cap):
    """Rounds of commit_f32 whose priorities span 2^-40 .. 2^20 fall back to the ordered walk by themselves and leave the heap
    off left + right; adds at max_priority through set, set_from and set_many_from must then follow the reference's delta walk:
    every node equal to the oracle's after each."""
    dev = dra.Config.DEVICE
    orc = E.filled_oracle(cap, cap)
    tree = _device_tree(dra, orc.tree, cap)
    try:
        hi, lo = float(orc.tree[cap - 1:].max()), float(orc.tree[cap - 1:].min())
        stat = _t(np.asarray([hi, lo]), dev)
        for k, (leaves, prio) in enumerate(E.fallback_rounds(cap)):
            hi, lo = max(hi, float(prio.max())), min(lo, float(prio.min()))
            E.oracle_updates(orc, leaves, prio.astype(np.float64))
            tree.commit_f32(_t(leaves, dev), _t(np.arange(len(leaves), dtype=np.int32), dev), _t(prio, dev), stat)
            assert np.array_equal(_tree_bits(tree), _bits(orc.tree)), "round %d" % k
        assert stat.cpu().tolist() == [hi, lo] and not E.exact_regime(cap, hi, lo)
        assert not np.array_equal(orc.tree, orc.rebuilt())
        orc.write = 0
        orc.add(hi)
        tree.set(cap - 1, hi)
        assert np.array_equal(_tree_bits(tree), _bits(orc.tree)), "set"
        orc.add(hi)
        tree.set_from(cap, stat)
        assert np.array_equal(_tree_bits(tree), _bits(orc.tree)), "set_from"
        write0, n = E.fallback_many_add(cap)
        orc.write = write0
        for _ in range(n):
            orc.add(hi)
        tree.set_many_from(write0, n, stat, stat=stat)
        assert np.array_equal(_tree_bits(tree), _bits(orc.tree)), "set_many_from"
    finally:
        tree.close()


def test_tree_sample_edges(dra):
    """Batches 1 / 63 / 64 / 65 / 1024 with u = 0 and nextafter(1, 0) in every stratum, ties s == tree[left] (all-ones trees
    with batch = capacity and u = 0, integer-aimed strata on a 1000-leaf one), zero-priority leaves, an all-zero tree."""
    dev = dra.Config.DEVICE
    trees = E.sample_trees()
    for name, heap in sorted(trees.items()):
        cap = (len(heap) + 1) // 2
        tree = _device_tree(dra, heap, cap)
        try:
            if name.startswith("ones_cap"):
                plans = [(b, {"boundary": E.boundary_us(heap[0], b)}) for b in (63, 65)]
            elif name.startswith("ones"):
                plans = [(cap, E.sample_us(cap, 2))]
            else:
                plans = [(b, E.sample_us(b, 2)) for b in E.SAMPLE_BATCHES]
            for b, us in plans:
                for kind, u in us.items():
                    want = E.ref_sample(heap, u)
                    idx, p, total = tree.sample(_t(u, dev))
                    what = "%s batch %d u %s" % (name, b, kind)
                    assert np.array_equal(idx.cpu().numpy(), want["idx"]), what
                    assert np.array_equal(_bits(p.cpu().numpy()), _bits(want["p"])), what
                    assert _bits(total.cpu().numpy())[0] == _bits(np.asarray([want["total"]]))[0], what
        finally:
            tree.close()


# ================================================================================================ the device draw
@pytest.mark.parametrize("case", E.PER_CASES, ids=_ids(E.PER_CASES))
def test_per_chain2_edges(dra, case):
    """The stand-alone dra_sumtree_per_chain2 launch, round after round, with the assertions of tests/test_gpu_per_chain2.py."""
    d = dra
    from deeprl_amd._lib import lib
    ops = d.ops
    dev = d.Config.DEVICE
    cap, batch = case["cap"], case["batch"]
    run = E.PerRun(case)
    tree = _device_tree(d, run.ref.orc.tree, cap)
    tree_t = tree.as_tensor()
    stat = torch.tensor([run.ref.max_p, run.ref.min_p], dtype=torch.float64, device=dev)
    sb = ctypes.c_int64()
    lib.dra_sumtree_per_chain2_state_bytes(ctypes.byref(sb))
    state = torch.zeros(sb.value, dtype=torch.uint8, device=dev)
    io_t = torch.zeros(ctypes.sizeof(ops.PerChain2IO), dtype=torch.uint8).pin_memory()
    io = ops.PerChain2IO.from_address(io_t.data_ptr())
    words_t = torch.zeros(ops.PER_RNG_WORDS, dtype=torch.int32).pin_memory()
    words_t.numpy().view(np.uint32)[:run.n_words] = run.words
    idx_out = torch.zeros(1024, dtype=torch.int64, device=dev)
    samp = torch.zeros(batch + 1, dtype=torch.float32, device=dev)
    weights = torch.zeros(batch, dtype=torch.float32, device=dev)
    prio_out = torch.zeros(batch, dtype=torch.float32, device=dev)
    lib.dra_sumtree_per_chain2_state_set(ctypes.c_void_p(state.data_ptr()), 0, 0,
                                         np.asarray(run.cur_idx, dtype=np.int64).ctypes.data_as(ctypes.c_void_p), batch)
    stream = torch.cuda.current_stream()
    worst_prio = worst_w = 0.0
    try:
        for r in range(case["rounds"]):
            inp = run.begin()
            loss_t = torch.from_numpy(inp["loss"]).to(dev)
            io.add_n, io.batch, io.next_batch, io.force_ordered = inp["add_n"], batch, batch, 0
            io.history, io.n_step, io.add_write0, io.memory_size = case["history"], case["n_step"], inp["write0"], cap
            io.pos_after, io.size_after, io.rng_produced, io.beta_next = inp["pos_after"], inp["size_after"], inp["rng_produced"], inp["beta"]
            lib.dra_sumtree_per_chain2(tree.h, ctypes.c_void_p(io_t.data_ptr()), ops.ptr(loss_t), case["eps"], case["alpha"], ops.ptr(prio_out),
                                       ops.ptr(stat), ctypes.c_void_p(state.data_ptr()), ctypes.c_void_p(words_t.data_ptr()), ops.ptr(idx_out),
                                       ops.ptr(samp), ops.ptr(weights), batch, ctypes.c_void_p(stream.cuda_stream))
            torch.cuda.synchronize()
            msg = "%s round %d" % (case["name"], r)
            prio = E.ref_priorities(inp["loss"], case["eps"], case["alpha"])
            got_prio = prio_out.cpu().numpy()
            if case["alpha"] == 0.5:
                assert np.array_equal(_bits(got_prio), _bits(prio)), msg
            else:       # powf: rtol 1e-6; the oracle goes on from the device's priorities
                worst_prio = max(worst_prio, float(np.abs(got_prio.astype(np.float64) / prio.astype(np.float64) - 1.0).max()))
                np.testing.assert_allclose(got_prio, prio, rtol=E.POW_RTOL, err_msg=msg)
                prio = got_prio
            want = run.finish(prio)
            final = run.final
            assert io.out_seq == want["seq"], msg
            assert (io.out_flags & 2) == (want["flags"] & 2) and (io.out_flags & 1) == (want["flags"] & 1), (msg, io.out_flags)
            assert np.array_equal(_bits(tree_t.cpu().numpy()), _bits(want["tree"])), msg + ": tree"
            assert stat.cpu().tolist() == want["stat"], msg
            assert list(io.out_raw_idx[:batch]) == want["raw"], msg
            assert io.out_n_valid == want["n_valid"], msg
            assert list(io.out_idx[:batch]) == want["idx"] and list(io.out_p[:batch]) == want["p"] and io.out_total == want["total"], msg
            assert np.array_equal(idx_out[:batch].cpu().numpy(), np.asarray(want["idx"]) - (cap - 1)), msg
            assert 0 <= int(idx_out[:batch].min()) and int(idx_out[:batch].max()) < cap, msg
            want_sp = (np.asarray(want["p"]) / want["total"]).astype(np.float32)
            got = samp.cpu().numpy()
            assert np.array_equal(_bits(got[:batch]), _bits(want_sp)) and got[batch] == np.float32(want["beta"]), msg
            want_w = E.ref_weights(want_sp, batch, want["beta"])
            got_w = weights.cpu().numpy()
            worst_w = max(worst_w, float(np.abs(got_w.astype(np.float64) / want_w.astype(np.float64) - 1.0).max()))
            np.testing.assert_allclose(got_w, want_w, rtol=E.POW_RTOL, err_msg=msg)
            used = int(io.out_rng_cursor) - run.consumed
            if final == "dry":
                assert used == 2 * batch, msg
            else:       # words consumed == what python's generator consumed for this draw
                random.setstate(want["before"])
                if used:
                    random.getrandbits(32 * used)
                assert random.getstate() == want["after"], msg + ": %d words" % used
                random.setstate(want["after"])
            run.consumed = int(io.out_rng_cursor)
        errs = dict(weights_rel=worst_w)
        if case["alpha"] != 0.5:        # (sqrt priorities are compared bit for bit: no figure to record)
            errs["powf_prio_rel"] = worst_prio
        record_parity("replay_edges_per_chain2_" + case["name"], **errs)
    finally:
        tree.close()
