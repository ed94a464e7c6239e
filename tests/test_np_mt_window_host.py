"""dra_np_mt_draw_window_host (csrc/np_mt.hip, csrc/np_mt.h): one lane's step of the device draws over an n-step window as plain
host code, against np.random.RandomState itself driven through support.plan_actor_epsilon_greedy and
replay.draw_uniform_indices(..., n_step=n) -- the indices, the flags, the actions and the generator's key and pos afterwards.  No GPU
is touched.

The ring is tests/test_gpu_dqn_lanes_agent.py's (24 slots, minibatches of 10, 4 transitions per step) in the states of
np_mt_window_cases.rings: either range of valid indices empty, exactly one valid slot, both populated; the generator starts one
word before the twist, on it and mid-key.  Every state is one numpy alone walks through in far fewer words than the entry's
budget of 4096, which the test counts before it compares."""
import numpy as np
import pytest

import np_mt_cases as C
import np_mt_window_cases as W

STEPS = 40
WORD_BOUND = 1024      # a quarter of kNpMtBudget: what "far fewer" means below


def _cases():
    return [(n, name, ring, start) for n in W.N_STEPS for name, ring in W.rings(n) for start in W.STARTS]


def _case_id(case):
    n, name, ring, start = case
    return "n%d-%s-ring%dat%d-%s" % (n, name, ring[0], ring[1], "_".join(str(x) for x in start))


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_window_host_entry_draws_numpys_stream(case):
    n, name, ring, start = case
    size, pos = ring
    count = len([i for i in range(size) if W.valid(i, pos, size, n)])
    assert count == (1 if name == "one_valid" else count) and count > 0
    rs = C.start_state(start)
    lane = W.WindowLane(rs, W.K, W.BATCH, W.N_ACTIONS, n)
    regenerated = 0
    for step in range(STEPS):
        learn = step % 5 != 1
        before = rs.get_state()[2]
        want = W.numpy_step(rs, 0.37, W.K, W.BATCH, W.N_ACTIONS, ring, n, learn, limit=WORD_BOUND)
        assert want["words"] < WORD_BOUND, (step, want["words"])      # numpy alone, counted on the raw stream
        stale = lane.idx().copy()
        lane.step(want["eps"], want["slot0"], ring, learn)
        assert lane.err.value == 0, (step, lane.err.value)
        assert np.array_equal(lane.rand(), want["rand"]), step
        assert np.array_equal(lane.flags(), want["explore"]), step
        assert lane.slot0() == want["slot0"]
        assert np.array_equal(lane.idx(), want["idx"] if learn else stale), step
        if learn:
            assert all(W.valid(int(i), pos, size, n) for i in lane.idx()), step
        _, key, mt_pos, has_gauss, _ = rs.get_state()
        assert lane.pos() == mt_pos and np.array_equal(lane.key(), key) and has_gauss == 0, step
        regenerated += mt_pos < before
    assert regenerated >= 1, regenerated


@pytest.mark.parametrize("start", W.STARTS, ids=lambda s: "_".join(str(x) for x in s))
def test_window_of_one_is_the_one_step_entry(start):
    """At n_step 1 the window entry's state and block equal dra_np_mt_draw_host's byte for byte, step after step."""
    for name, ring in W.rings(1):
        old = C.HostLane(C.start_state(start), W.K, W.BATCH, W.N_ACTIONS)
        new = W.WindowLane(C.start_state(start), W.K, W.BATCH, W.N_ACTIONS, 1)
        for step in range(STEPS):
            learn = step % 5 != 1
            eps = [0.9, 0.0, 0.37, 1.0]
            old.step(eps, step % ring[0], ring, learn)
            new.step(eps, step % ring[0], ring, learn)
            assert old.block.tobytes() == new.block.tobytes() and old.words.tobytes() == new.words.tobytes(), (name, step)
            assert old.err.value == new.err.value == 0


def test_a_ring_without_a_window_valid_index_is_refused():
    """DRA_EINVAL before any word is drawn for a ring state whose window-valid count is 0 -- fewer rows than a window, and a
    full ring is never one: capacity >= n_step + 1 --, for an n_step outside 1..8; a step that does not learn is taken."""
    from deeprl_amd import seed_batch
    for n, ring in ((3, (3, 3)), (3, (2, 2)), (8, (8, 8)), (2, (1, 1)), (8, (4, 4))):
        assert seed_batch.valid_index_count(ring[1], ring[0], n) == 0
        lane = W.WindowLane(C.start_state(("seed", 0)), W.K, W.BATCH, W.N_ACTIONS, n)
        before = lane.words.copy()
        assert lane.step_raw([0.5] * W.K, 0, ring, True) == -22
        assert np.array_equal(lane.words, before)
        assert lane.step_raw([0.5] * W.K, 0, ring, False) == 0
    for n in (0, 9, -1):
        lane = W.WindowLane(C.start_state(("seed", 0)), W.K, W.BATCH, W.N_ACTIONS, n)
        assert lane.step_raw([0.5] * W.K, 0, (24, 11), False) == -22


def test_valid_index_count_is_the_replays():
    """valid_index_count(pos, size, n) against len(compute_valid_indices()) of a UniformReplay, over every (pos, size) a ring of
    12 slots passes through (size < 12: pos == size; full: every pos) and the states a checkpoint could hold besides, n 1..8;
    the default n is 1."""
    from deeprl_amd import seed_batch
    from deeprl_amd.replay import UniformReplay
    for n in range(1, 9):
        rp = UniformReplay(memory_size=12, batch_size=4, n_step=n, discount=0.99, history_length=1)
        seen = 0
        for size in range(0, 13):
            for pos in range(0, 12):
                if pos > size:
                    continue
                rp.pos = pos
                rp.size = lambda size=size: size
                want = len(rp.compute_valid_indices())
                assert seed_batch.valid_index_count(pos, size, n) == want, (n, pos, size)
                assert want == len([i for i in range(size) if rp.valid_index(i)])
                seen += 1
        assert seen > 80
    assert seed_batch.valid_index_count(5, 12) == seed_batch.valid_index_count(5, 12, 1) == 4 + 6


def test_window_lanes_supported_limits():
    from deeprl_amd._lib import lib
    ok = lib.dra_np_mt_window_lanes_supported.raw
    assert ok(1, 1, 1, 1, 2, 1) == 0 and ok(64, 8, 256, 6, 2 ** 32 - 1, 8) == 0 and ok(3, 4, 10, 2, 9, 8) == 0
    for bad in ((0, 4, 10, 2, 24, 3), (65, 4, 10, 2, 24, 3), (3, 0, 10, 2, 24, 3), (3, 9, 10, 2, 24, 3), (3, 4, 0, 2, 24, 3),
                (3, 4, 257, 2, 24, 3), (3, 4, 10, 0, 24, 3), (3, 4, 10, 2, 2 ** 32, 3), (3, 4, 10, 2, 24, 0), (3, 4, 10, 2, 24, 9),
                (3, 4, 10, 2, 8, 8), (3, 4, 10, 2, 3, 3)):
        assert ok(*bad) == -22, bad
    for dims in ((3, 4, 10, 2, 24), (3, 4, 10, 2, 1), (65, 4, 10, 2, 24)):      # n_step 1 is the 1-step table
        assert ok(*dims, 1) == lib.dra_np_mt_lanes_supported.raw(*dims)
