"""The update's chained launches hand activations, gradients and weight-gradient slabs from workgroup to workgroup INSIDE a
launch (csrc/common.h mega_st / mega_st4 / mega_ld4: write-through stores, arrival counters, agent-scope loads).  Whatever the
width of those accesses, a chained launch does the arithmetic of the per-layer launches in the same order: the pipeline with
DRA_VAR_FWD_CHAIN | DRA_VAR_BWD_CHAIN set (the default) and cleared must end on the same bits.  tests/test_gpu_agents.py holds
that at batch 32; here at the smallest batch that takes the chains (17, odd: csrc/learner.hip `fchain` / `bchain`) and at 24
(neither a full minibatch nor a multiple of the 8 XCDs' sample groups), so that partial sample groups, the natural-order
remainder of xcd_order and slab counts that are no multiple of the folds' four groups are covered."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


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
    out = dict(p=L.flat.flat.detach().cpu().numpy().copy(), s1=L.state1.detach().cpu().numpy().copy(),
               s2=L.state2.detach().cpu().numpy().copy(), pt=L.target_flat.flat.detach().cpu().numpy().copy(),
               q=L.q.detach().cpu().numpy().copy(), delta=L.delta.detach().cpu().numpy().copy(),
               norm=L.norm.detach().cpu().numpy().copy())
    L.close()
    b.ring.close()
    return out


@pytest.mark.parametrize("batch", [17, 24])
def test_chained_launches_are_bit_identical_at_partial_batches(dra, batch):
    from deeprl_amd import ops
    default = ops.get_tuning()
    chains = ops.VAR_FWD_CHAIN | ops.VAR_BWD_CHAIN
    assert default & chains == chains, "the library default carries both chained launches"
    got = _run(dra, batch, default)
    want = _run(dra, batch, default & ~chains)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (batch, k)
    assert float(np.abs(got["p"]).max()) > 0 and float(np.abs(got["delta"]).max()) > 0 and float(got["norm"][0]) > 0
    assert not np.array_equal(got["p"], got["pt"])       # (updates ran after the target sync)
