"""The update's chained launches (DRA_VAR_FWD_CHAIN | DRA_VAR_BWD_CHAIN, batches 17..32) hand activations, gradients and
weight-gradient slabs between workgroups of one launch through 32-bit arrival counters that are never reset: a consumer waits for
(updates so far + 1) x (arrivals per update), and counter and product wrap modulo 2^32 (csrc/common.h chain_reached; the predicate
itself is held on the CPU by tests/test_chain_counter_wrap_host.py).  No run of the suite reaches update 14.9 M, where the first
counter wraps, so here the counters are PUT next to each wrap (DQNLearner.chain_set_epoch: every counter at its level state for a
given number of updates) and the learner must carry on exactly as its twin at update 0 does: same loss and gradient norm after
every update, same parameters, optimiser state, target, q and TD errors at the end, to the bit -- the chains are deterministic
(tests/test_gpu_chain_handover.py, tests/test_gpu_learner_edges.py).  A consumer let through early reads the previous update's
activations or slabs, which shows as different bits; a wait that never ends gives up after 50 ms and surfaces as DRA_ETIMEDOUT.

Batch 17 is the smallest (and an odd) batch that takes the chains, 153 and 68 arrivals on the weight-gradient counters; batch 32
the full minibatch, 128 arrivals on conv2's weight-gradient counter being the power-of-two case (its target wraps to exactly 0);
DRA_VAR_BWD_CHAIN_FC adds the one fc4 input-gradient counter that 98 producers and several hundred consumers share;
DRA_VAR_TARGET_AHEAD the target net's own forward chains, with a counter set and an epoch word per update parity, run for 16 steps
so that both sets pass their wrap.  The last test starts the persistent actor's 32-bit step word just before its two wraps."""
import numpy as np
import pytest
import torch

from parity_log import record_parity
from test_chain_counter_wrap_host import ARRIVALS

pytestmark = pytest.mark.gpu

STEPS = 6          # from 3 updates before the wrap: crosses it for both epoch biases
# The target-ahead chains (DRA_VAR_TARGET_AHEAD: the target net's forward chain of the NEXT update on a third stream, one set of
# counters and one epoch word per update parity) start in the event-free lane, from the fifth step on, and each set is used every
# other step: its third use -- the one whose target wraps -- comes in the eighth step.  16 steps leave room for a later lane entry.
AHEAD_STEPS = 16
# name -> (batch, DRA_VAR_BWD_CHAIN_FC, DRA_VAR_TARGET_AHEAD, steps); the arrival counts per counter class the library must report
# are the hand-written table of the host test, by batch
CONFIGS = {"B17": (17, False, False, STEPS), "B32": (32, False, False, STEPS), "B32-fc": (32, True, False, STEPS),
           "B32-ahead": (32, False, True, AHEAD_STEPS)}


def _expected(batch, fc):
    pick = lambda v: v[0] if len(v) == 1 else v[{17: 0, 32: 1}[batch]]
    return {k: pick(v) for k, v in ARRIVALS.items() if fc or k != "bwd_fc4_dgrad"}


CASES = [(name, t) for name, (batch, fc, ahead, _) in CONFIGS.items() for t in sorted(set(_expected(batch, fc).values()))
         if not ahead or t in ARRIVALS["fwd_conv1_to_conv2"] + ARRIVALS["fwd_conv2_to_conv3"]]     # (the ahead chains are forward chains)


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


def _bits(t):
    return t.detach().cpu().contiguous().numpy().copy()


def _variant(fc, ahead=False):
    from deeprl_amd import ops
    default = ops.get_tuning()
    chains = ops.VAR_FWD_CHAIN | ops.VAR_BWD_CHAIN
    assert default & chains == chains, "the library default carries both chained launches"
    v = (default | ops.VAR_BWD_CHAIN_FC) if fc else (default & ~ops.VAR_BWD_CHAIN_FC)
    return (v | ops.VAR_TARGET_AHEAD) if ahead else (v & ~ops.VAR_TARGET_AHEAD)


def _run(batch, fc, ahead, steps, epoch):
    """`steps` steps of the benchmarked pipeline from a fresh bench whose chains were put at `epoch`.  -> (report of the aid, results)"""
    from deeprl_amd.learner import DQNLearnerBench
    np.random.seed(41)
    torch.manual_seed(42)
    b = DQNLearnerBench(ring_capacity=4096, batch=batch, seed=43, actor=True, async_actor=True, variant=_variant(fc, ahead))
    L = b.learner
    try:
        report = L.chain_set_epoch(epoch)
        per_step = []
        for _ in range(steps):
            b.step()               # (a bounded in-launch wait that gave up makes the next call raise: DRA_ETIMEDOUT)
            torch.cuda.synchronize()
            per_step.append((_bits(L.loss.reshape(1)).view(np.uint32)[0], _bits(L.norm).view(np.uint32)[0]))
        ahead_stats = L.ahead_stats()
        L.synchronize()
        out = dict(p=_bits(L.flat.flat), s1=_bits(L.state1), s2=_bits(L.state2), pt=_bits(L.target_flat.flat), q=_bits(L.q),
                   delta=_bits(L.delta), norm=_bits(L.norm))
        return report, dict(per_step=per_step, flags=L.path_flags(), ahead=ahead_stats, out=out)
    finally:
        L.close()
        b.ring.close()


_TWINS = {}


def _twin(name):
    """The same run with the chains at update 0 (through the aid, so that both runs take the same calls): once per configuration."""
    if name not in _TWINS:
        batch, fc, ahead, steps = CONFIGS[name]
        report, res = _run(batch, fc, ahead, steps, 0)
        horizons = sorted((t, k) for k, t in report.items() if k != "target_ahead")
        for t, k in horizons:
            wrap = -(-(1 << 32) // t)
            print("chain counter wrap [%s] %-20s T = %3d  wraps in update %d" % (name, k, t, wrap))
            record_parity("chain_counter_wrap[%s] %s" % (name, k), arrivals_per_update=t, wrap_update=wrap)
        _TWINS[name] = (report, res)
    return _TWINS[name]


def test_a_learner_without_chained_launches_refuses_the_aid(dra):
    from deeprl_amd._lib import DraError
    from deeprl_amd.learner import DQNLearnerBench
    b = DQNLearnerBench(ring_capacity=4096, batch=16, seed=43, actor=True, async_actor=True)       # (the chains start at batch 17)
    try:
        flags = b.learner.path_flags()
        assert not flags["fchain"] and not flags["bchain"]
        with pytest.raises(DraError, match="-22"):
            b.learner.chain_set_epoch(5)
    finally:
        b.learner.close()
        b.ring.close()


# ---- the persistent actor's 32-bit step word ------------------------------------------------------------------------------------
RESUME_STEPS = 160
_RESUME = {}


def _new_bench():
    from deeprl_amd.learner import DQNLearnerBench
    np.random.seed(41)
    torch.manual_seed(42)
    return DQNLearnerBench(ring_capacity=4096, batch=32, seed=43, actor=True, async_actor=True, variant=_variant(False))


_BENCH_HOST = ("counter", "pos", "size", "updates", "_primed", "_ring_pushed", "_ring_issued", "_fed_steps", "_pos0", "_size0")


def _resume_source():
    """Everything of a bench after 4 steps that a fresh bench needs to continue it: the learner's resume state, the replay ring's
    arrays, the bench's host bookkeeping and the two random streams."""
    import ctypes
    if "src" not in _RESUME:
        b = _new_bench()
        L = b.learner
        try:
            for _ in range(4):
                b.step()
            st = L.resume_state()                  # (synchronises, a pending fc4 segment flushed)
            _RESUME["src"] = dict(learner=st, ring=[a.cpu().clone() for a in b.ring.arrays()], host={k: getattr(b, k) for k in _BENCH_HOST},
                                  actor_rs=b.actor_rs.get_state(), np_random=np.random.get_state(),
                                  params=ctypes.string_at(ctypes.addressof(L.params), ctypes.sizeof(L.params)))
        finally:
            L.close()
            b.ring.close()
    return _RESUME["src"]


def _resumed_run(shift):
    """A fresh bench continued from the source with the actor's step counters -- host (aring_pushed, aring_issued) and device
    (aring_seq) -- moved on by `shift`, then RESUME_STEPS steps."""
    import copy
    import ctypes
    src = _resume_source()
    st = copy.deepcopy(src["learner"])
    assert shift % 64 == 0
    assert st["counters"][11] == 0        # (aprm_seq counts the launches of the staged-block actor, which the ring actor never issues)
    st["counters"][3] += shift            # aring_pushed
    st["counters"][4] += shift            # aring_issued
    seq = st["buffers"]["aring_seq"].numpy().view(np.uint32)
    assert seq.shape == (1,) and int(seq[0]) == src["learner"]["counters"][4]      # (device and host count agree at a step boundary)
    seq[0] = np.uint32((int(seq[0]) + shift) & 0xffffffff)
    b = _new_bench()
    L = b.learner
    try:
        for dst, a in zip(b.ring.arrays(), src["ring"]):
            dst.copy_(a)
        L.load_resume_state(st)
        for k, v in src["host"].items():
            setattr(b, k, v)
        b.actor_rs.set_state(src["actor_rs"])
        np.random.set_state(src["np_random"])
        ctypes.memmove(ctypes.addressof(L.params), src["params"], ctypes.sizeof(L.params))
        per_step = []
        for _ in range(RESUME_STEPS):
            b.step()
            torch.cuda.synchronize()
            per_step.append((_bits(L.loss.reshape(1)).view(np.uint32)[0], _bits(L.norm).view(np.uint32)[0]))
        L.synchronize()
        torch.cuda.synchronize()
        _, actions, rewards, masks = b.ring.arrays()
        out = dict(p=_bits(L.flat.flat), s1=_bits(L.state1), s2=_bits(L.state2), pt=_bits(L.target_flat.flat), q=_bits(L.q),
                   delta=_bits(L.delta), norm=_bits(L.norm), actions=_bits(actions), rewards=_bits(rewards), masks=_bits(masks))
        seq_end = int(dict(L._resume_buffers())["aring_seq"].cpu().numpy().view(np.uint32)[0])
        return dict(per_step=per_step, flags=L.path_flags(), lane=L.lane_stats(), out=out, seq_end=seq_end)
    finally:
        L.close()
        b.ring.close()


@pytest.mark.parametrize("shift,boundary", [((1 << 29) - 64, 1 << 29), ((1 << 32) - 64, 1 << 32)], ids=["tag-wrap", "word-wrap"])
def test_the_actor_step_word_wraps_without_a_trace(dra, shift, boundary):
    """The persistent actor counts agent steps in a 32-bit device word (aring_seq) and derives its hand-over tags as
    seq * 8 + e + 1 (csrc/actor_persist.h): the tags wrap at 2^29 agent steps, the word at 2^32, the host's counts are 64-bit.
    Through the resume interface a fresh learner starts just before either point: the state of a bench after 4 steps is loaded
    into two fresh benches, once as it is and once with the actor's step counters -- aring_pushed, aring_issued (host) and
    aring_seq (device) -- moved on by one common offset, and both run 160 steps; everything the twins compute is equal to the bit,
    the replay ring's actions, rewards and masks included.

    The offsets are multiples of 64, 2^29 - 64 and 2^32 - 64, so that the parameter-ring entry seq % 64, the slot of the
    pinned `need` ring and the step parity stay what the saved ring entries were written for (with the actor 5 steps in, the tag
    base seq * 8 passes 2^32 / the word passes 2^32 at the 59th step of the run).  Nothing else had to stay behind: the blocks
    in the parameter ring carry replay-ring slots and frame counters, no step number; aprm_seq is the staged-block actor's
    launch count, zero under the ring actor."""
    twin = _RESUME.get("twin")
    if twin is None:
        twin = _RESUME["twin"] = _resumed_run(0)
    got = _resumed_run(shift)
    first_seq = _resume_source()["learner"]["counters"][4]
    assert twin["seq_end"] == first_seq + RESUME_STEPS
    assert got["seq_end"] == (first_seq + shift + RESUME_STEPS) & 0xffffffff
    assert first_seq + shift < boundary <= first_seq + shift + RESUME_STEPS        # (the step count passes the wrap inside the run)
    for who, r in (("twin", twin), ("shifted", got)):
        assert not r["flags"]["timed_out"], who
        assert r["flags"]["fchain"] and r["flags"]["bchain"] and r["flags"]["fs"], who
        assert r["lane"]["steps"] >= RESUME_STEPS - 32, (who, r["lane"])     # (the persistent actor ran: the lane carried the run)
    assert got["per_step"] == twin["per_step"], "loss / norm after every update"
    for k, want in twin["out"].items():
        a, w = got["out"][k], want
        assert a.shape == w.shape and a.dtype == w.dtype and np.array_equal(a.view(np.uint8), w.view(np.uint8)), (shift, k)
    assert float(np.abs(twin["out"]["delta"]).max()) > 0 and float(twin["out"]["norm"][0]) > 0


@pytest.mark.parametrize("name,t", CASES, ids=["%s-T%d" % c for c in CASES])
def test_a_learner_next_to_a_counter_wrap_equals_its_twin_bit_for_bit(dra, name, t):
    batch, fc, ahead, steps = CONFIGS[name]
    twin_report, twin = _twin(name)
    want_report = dict(_expected(batch, fc), target_ahead=ahead)
    assert twin_report == want_report, "the library's arrival counts against the table of tests/test_chain_counter_wrap_host.py"
    wrap = -(-(1 << 32) // t)                       # the update in which (updates + 1) x T first reaches 2^32
    report, got = _run(batch, fc, ahead, steps, wrap - 3)
    assert report == want_report
    for who, r in (("twin", twin), ("wrap", got)):
        assert not r["flags"]["timed_out"], who
        assert r["flags"]["fchain"] and r["flags"]["bchain"], who
        assert r["flags"]["ah"] == ahead, who
        if ahead:       # six uses or more of the ahead chains (in line or consumed from the stash): each parity set three times
            assert r["ahead"]["active"] and r["ahead"]["in_line"] >= 1 and r["ahead"]["from_stash"] + r["ahead"]["in_line"] >= 6, (who, r["ahead"])
    for i, (a, b) in enumerate(zip(got["per_step"], twin["per_step"])):
        print("T %d update %d (chains at %d): loss bits %08x / %08x  norm bits %08x / %08x" % (t, i, wrap - 3 + i, a[0], b[0], a[1], b[1]))
    assert got["per_step"] == twin["per_step"], (name, t, "loss / norm after every update")
    for k, want in twin["out"].items():
        assert got["out"][k].shape == want.shape and np.array_equal(got["out"][k].view(np.uint32), want.view(np.uint32)), (name, t, k)
    for r in (twin, got):
        assert float(np.abs(r["out"]["delta"]).max()) > 0 and float(r["out"]["norm"][0]) > 0
        assert not np.array_equal(r["out"]["p"], r["out"]["pt"])        # (updates really ran)
