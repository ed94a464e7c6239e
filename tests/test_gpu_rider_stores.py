"""The riders of the update's chained forward launch step fc4's deferred optimizer segment and store what they produce
THROUGH the L2 (csrc/common.h fc4_rider_run<true>, DRA_EXP_RIDER_WT: 16-byte raw-buffer stores behind a 32-bit offset, which the
hardware does not bounds-check); the flush kernel runs the same code with plain stores (fc4_rider_run<false>).  Whatever the form
of the stores, the arithmetic is the same: same bits, nothing outside the segment touched, nothing written when nothing is
pending.  Kernel test: the two forms as launches of their own (dra_fc4_rider_test) at sizes around one rider workgroup's 768
float4s; pipeline test: the benchmarked pipeline at batch 17 with DRA_VAR_DEFER_FC4 set and cleared (the actor reads the copy
the riders write through: ring frames and actions depend on it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of a fixed bit pattern in front of and behind the segment, in every buffer
GUARD_BITS = -0x21524111        # 0xDEADBEEF as int32 (a NaN as f32: any arithmetic on it would show)
WG4 = 768                       # float4s of one rider workgroup (256 threads x kRiderNV)
LR, ALPHA, EPS = 0.00025, 0.95, 0.01


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


def _buffers(begin4, count4, seed):
    """p, g, s1, s2, copy as int32 views of f32 device buffers: GUARD floats | 4 * begin4 floats | segment | GUARD floats | tail.
    The base handed to the kernel is element GUARD (16-byte aligned); the GUARD floats on either side of the SEGMENT carry the
    pattern (with begin4 = 3 the front guard covers the 12 floats in front of the segment and reaches below the base)."""
    rng = np.random.RandomState(seed)
    n = GUARD + 4 * (begin4 + count4) + GUARD + 16
    lo, hi = GUARD + 4 * begin4, GUARD + 4 * (begin4 + count4)
    out = {}
    for k in ("p", "g", "s1", "s2", "copy"):
        x = rng.standard_normal(n).astype(np.float32) * (0.1 if k != "p" else 1.0)
        out[k] = x
    out["s1"] = (out["s2"] * out["s2"] + rng.uniform(0.005, 0.015, n)).astype(np.float32)   # centered RMSprop: s1 - s2^2 >= 0.005
    for k, x in out.items():
        xi = x.view(np.int32)
        xi[lo - GUARD:lo] = GUARD_BITS
        xi[hi:hi + GUARD] = GUARD_BITS
    return out, lo, hi


def _launch(ops, host, begin4, count4, centered, with_copy, pending, write_through):
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in host.items()}
    coef = torch.tensor([0.37], dtype=torch.float32, device="cuda")
    pend = torch.tensor([pending], dtype=torch.int32, device="cuda")
    ops.fc4_rider_step(dev["p"][GUARD:], dev["g"][GUARD:], dev["s1"][GUARD:], dev["s2"][GUARD:],
                       dev["copy"][GUARD:] if with_copy else None, begin4, count4, coef, pend, LR, ALPHA, EPS, centered,
                       write_through)
    torch.cuda.synchronize()
    assert int(pend.item()) == pending                     # the rider code reads the word; its launch lowers it, not the rider
    return {k: v.cpu().numpy().view(np.int32) for k, v in dev.items()}


@pytest.mark.parametrize("begin4", [0, 3])
@pytest.mark.parametrize("count4", [1, 255, WG4 - 1, WG4, WG4 + 1, 3 * WG4 + 5])
def test_write_through_rider_matches_plain_rider(dra, count4, begin4):
    from deeprl_amd import ops
    host, lo, hi = _buffers(begin4, count4, 1000 * begin4 + count4)
    init = {k: v.view(np.int32) for k, v in host.items()}
    for centered in (True, False):
        for with_copy in (True, False):
            case = (count4, begin4, centered, with_copy)
            plain = _launch(ops, host, begin4, count4, centered, with_copy, 1, False)
            wt = _launch(ops, host, begin4, count4, centered, with_copy, 1, True)
            for k in ("p", "s1", "s2", "copy", "g"):
                assert np.array_equal(wt[k], plain[k]), (case, k, "write-through vs plain")
                for got in (wt[k], plain[k]):
                    # guards and everything else outside the segment: untouched
                    assert np.all(got[lo - GUARD:lo] == GUARD_BITS) and np.all(got[hi:hi + GUARD] == GUARD_BITS), (case, k, "guard")
                    assert np.array_equal(got[:lo], init[k][:lo]) and np.array_equal(got[hi:], init[k][hi:]), (case, k, "outside")
            # the step happened, and only where it should
            changed = lambda k: np.count_nonzero(wt[k][lo:hi] != init[k][lo:hi]) >= 0.75 * (hi - lo)   # (a tiny g moves p by < 1 ulp)
            assert changed("p") and changed("s1"), case
            assert np.array_equal(wt["g"], init["g"]), case
            if centered:
                assert changed("s2"), case
            else:
                assert np.array_equal(wt["s2"], init["s2"]), case
            if with_copy:
                assert np.array_equal(wt["copy"][lo:hi], wt["p"][lo:hi]), case
            else:
                assert np.array_equal(wt["copy"], init["copy"]), case
            # against the arithmetic of torch.optim.RMSprop in fp64 (that the plain form is a sound reference)
            f = lambda k, a: a[k].view(np.float32).astype(np.float64)
            gk = f("g", init)[lo:hi] * np.float64(np.float32(0.37))
            s = f("s1", init)[lo:hi] * np.float32(ALPHA) + (1.0 - np.float64(np.float32(ALPHA))) * gk * gk
            a = f("s2", init)[lo:hi] * np.float32(ALPHA) + (1.0 - np.float64(np.float32(ALPHA))) * gk
            avg = np.sqrt(np.maximum(s - a * a, 0.0) if centered else s) + EPS
            want = f("p", init)[lo:hi] - LR * gk / avg
            # (|p| < 8: one fp32 ulp is <= 4.8e-7; the step itself is < 1e-3 with a relative error of ~1e-5: var >= 4.7e-3 here)
            np.testing.assert_allclose(f("p", wt)[lo:hi], want, rtol=0, atol=5e-7)
            # nothing pending: nothing is written at all, in either form
            for write_through in (False, True):
                idle = _launch(ops, host, begin4, count4, centered, with_copy, 0, write_through)
                for k in idle:
                    assert np.array_equal(idle[k], init[k]), (case, k, "pending = 0", write_through)


def test_rider_launcher_refuses_what_the_16_byte_stores_cannot_address(dra):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, ptr, stream_ptr
    count4 = 5
    host, lo, hi = _buffers(0, count4, 7)
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in host.items()}
    coef = torch.tensor([0.37], dtype=torch.float32, device="cuda")
    pend = torch.tensor([1], dtype=torch.int32, device="cuda")

    def call(bases, begin4, write_through):
        return lib.dra_fc4_rider_test.raw(ptr(bases["p"]), ptr(bases["g"]), ptr(bases["s1"]), ptr(bases["s2"]), ptr(bases["copy"]),
                                          begin4, count4, ptr(coef), ptr(pend), LR, ALPHA, EPS, 1, write_through, stream_ptr())

    good = {k: v[GUARD:] for k, v in dev.items()}
    for write_through in (1, 0):
        for k in good:                                     # one base 4 bytes off a 16-byte boundary
            bad = dict(good)
            bad[k] = dev[k][GUARD + 1:]
            assert call(bad, 0, write_through) == -22, (k, write_through)
    # 4 * (begin4 + count4) floats = 2^29: the first offset a 32-bit byte offset no longer reaches
    assert call(good, (1 << 27) - count4, 1) == -22
    assert call(good, (1 << 27), 1) == -22 and call(good, -1, 1) == -22
    with pytest.raises(ops.DraError):
        ops.fc4_rider_step(good["p"], good["g"], good["s1"], good["s2"], good["copy"], (1 << 27) - count4, count4, coef, pend,
                           LR, ALPHA, EPS, True, True)
    torch.cuda.synchronize()
    for k, v in dev.items():                               # refused BEFORE any launch
        assert np.array_equal(v.cpu().numpy().view(np.int32), host[k].view(np.int32)), k
    assert call(good, 0, 1) == 0                           # (and the same buffers pass with a reachable offset)
    torch.cuda.synchronize()
    assert not np.array_equal(dev["p"].cpu().numpy().view(np.int32), host["p"].view(np.int32))


def _run(d, batch, variant):
    from deeprl_amd.learner import DQNLearnerBench
    np.random.seed(41)
    torch.manual_seed(42)
    b = DQNLearnerBench(ring_capacity=4096, batch=batch, seed=43, actor=True, async_actor=True, variant=variant)
    L = b.learner
    for t in range(24):
        b.step()               # (a bounded in-launch wait that gave up makes the call raise: DRA_ETIMEDOUT)
        if t == 11:
            L.sync_target()
        if t == 17:
            L.synchronize()
    L.synchronize()
    frames = d.ops._wrap_device_pointer(b.ring.pointers()[0], 200 * 7056, torch.uint8).cpu().numpy().copy()
    acts = d.ops._wrap_device_pointer(b.ring.pointers()[1], 200, torch.int64).cpu().numpy().copy()
    out = dict(p=L.flat.flat.detach().cpu().numpy().copy(), s1=L.state1.detach().cpu().numpy().copy(),
               s2=L.state2.detach().cpu().numpy().copy(), pt=L.target_flat.flat.detach().cpu().numpy().copy(),
               q=L.q.detach().cpu().numpy().copy(), delta=L.delta.detach().cpu().numpy().copy(),
               norm=L.norm.detach().cpu().numpy().copy(), frames=frames, acts=acts)
    L.close()
    b.ring.close()
    return out


def test_pipeline_with_riding_fc4_step_is_bit_identical_at_batch_17(dra):
    """Batch 17 is the smallest batch that takes the chained launches; fc4's segment is 1 605 632 / 4 float4s = 522 full rider
    workgroups and one of 512 float4s, at every batch."""
    from deeprl_amd import ops
    default = ops.get_tuning()
    assert default & ops.VAR_DEFER_FC4 and default & ops.VAR_FWD_CHAIN, "the library default lets the riders ride in the forward chain"
    assert (3136 * 512 // 4) % WG4 == 512
    got = _run(dra, 17, default)
    want = _run(dra, 17, default & ~ops.VAR_DEFER_FC4)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert float(np.abs(got["p"]).max()) > 0 and float(np.abs(got["delta"]).max()) > 0 and float(got["norm"][0]) > 0
    assert not np.array_equal(got["p"], got["pt"])       # (updates ran after the target sync)
