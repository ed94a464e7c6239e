"""dra_np_mt_draw_host (csrc/np_mt.hip, csrc/np_mt.h): one lane's step of the seed lanes' device draws as plain host code, against
np.random.RandomState itself driven through support.plan_actor_epsilon_greedy and replay.draw_uniform_indices -- the values, the
flags, and the generator's key and pos afterwards, step after step.  No GPU is touched.

The grid (np_mt_cases.py, shared with the kernel's test): every starting state with every ring state, and every (n_actions, k,
batch, epsilon) combination, the other dimensions cycling through their values so that each appears everywhere; 300 consecutive
steps per case (about 10 to 70 words per step: the key regenerates several to dozens of times)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import np_mt_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 300


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_host_entry_draws_numpys_stream(case):
    start, n_actions, k, batch, ring, eps_kind = case
    rs = C.start_state(start)
    lane = C.HostLane(rs, k, batch, n_actions)
    schedule = C.make_schedule(eps_kind)
    regenerated = 0
    for step in range(STEPS):
        learn = step % 5 != 1      # (a step that does not learn draws no index and leaves idx alone)
        before = rs.get_state()[2]
        want = C.numpy_step(rs, schedule, k, batch, n_actions, ring, learn)
        stale = lane.idx().copy()
        lane.step(want["eps"], want["slot0"], ring, learn)
        assert lane.err.value == 0, (step, lane.err.value)
        assert np.array_equal(lane.rand(), want["rand"]), step
        assert np.array_equal(lane.flags(), want["explore"]), step
        assert lane.slot0() == want["slot0"]
        assert np.array_equal(lane.idx(), want["idx"] if learn else stale), step
        _, key, pos, has_gauss, _ = rs.get_state()
        assert lane.pos() == pos and np.array_equal(lane.key(), key) and has_gauss == 0, step
        regenerated += pos < before
    assert regenerated >= (3 if batch >= 10 else 1), regenerated      # (240 minibatches of 10 alone are 2400 words)


def test_words_straddle_the_regeneration():
    """pos 623 in front of a rand(1) (one action: randint takes no word), and pos 622 in front of randint, then rand: the second
    word of the rand is the first of the regenerated key, and the key is regenerated no earlier."""
    for pos, n_actions in ((623, 1), (622, 2)):
        rs = C.start_state(("pos", 5, pos))
        lane = C.HostLane(rs, 1, 1, n_actions)
        old = lane.key().copy()
        want = C.numpy_step(rs, lambda: 0.5, 1, 1, n_actions, (24, 7), False)
        lane.step(want["eps"], 7, (24, 7), False)
        assert lane.pos() == 1 == rs.get_state()[2] and not np.array_equal(lane.key(), old)
        assert np.array_equal(lane.key(), rs.get_state()[1])
        assert np.array_equal(lane.rand(), want["rand"]) and np.array_equal(lane.flags(), want["explore"])


def test_a_ring_without_a_valid_index_is_refused():
    """A ring of one slot (either cursor) admits no index: DRA_EINVAL from the entry before any word is drawn, a ValueError from
    the host check seed_batch makes ahead of a step; a step that does not learn is taken."""
    from deeprl_amd import seed_batch
    for ring in ((1, 1), (1, 0)):
        assert seed_batch.valid_index_count(ring[1], ring[0]) == 0
        rs = C.start_state(("seed", 0))
        lane = C.HostLane(rs, 1, 4, 2)
        before = lane.words.copy()
        assert lane.step_raw([0.5], 0, ring, True) == -22
        assert np.array_equal(lane.words, before)
        assert lane.step_raw([0.5], 0, ring, False) == 0
    for size, pos in C.RINGS:
        assert seed_batch.valid_index_count(pos, size) == len([i for i in range(size) if C.valid(i, pos, size)]) > 0
    assert seed_batch.ring_after(22, 22, 24, 4) == (2, 24) and seed_batch.ring_after(5, 24, 24, 4) == (9, 24)
    assert seed_batch.ring_after(0, 0, 24, 4) == (4, 4)


def test_the_word_budget_ends_a_lane_that_finds_nothing():
    """An all-zero key (no state numpy ever holds: the twist keeps it zero) yields the index 0 for ever, which a ring of 3 at pos 1
    does not accept: the entry stops after its budget of 4096 words instead of spinning, fills the indices with a slot inside the
    ring and sets DRA_NP_MT_ERR_BUDGET in the err word; the acting draws of the same step (0 is a valid action) are made."""
    from deeprl_amd import seed_batch
    rs = np.random.RandomState(0)
    lane = C.HostLane(rs, 2, 10, 3)
    lane.words[:] = 0
    lane.idx()[:] = -1
    assert lane.step_raw([1.0, 0.0], 1, (3, 1), True) == 0
    assert lane.err.value == seed_batch.NP_MT_ERR_BUDGET == 1 << 30
    assert np.array_equal(lane.idx(), np.zeros(10, dtype=np.int64)) and np.array_equal(lane.rand(), [0, 0])
    assert lane.flags().tolist() == [True, False]
    # 2 x (randint + two words of rand) = 6 words, then attempts while at most 4096 have been taken: 4097 in all
    assert lane.pos() == 4097 % 624 and not lane.key().any()


def test_lanes_supported_limits():
    from deeprl_amd._lib import lib
    ok = lib.dra_np_mt_lanes_supported.raw
    assert ok(1, 1, 1, 1, 2) == 0 and ok(64, 8, 256, 6, 2 ** 32 - 1) == 0
    for bad in ((0, 4, 10, 2, 24), (65, 4, 10, 2, 24), (3, 0, 10, 2, 24), (3, 9, 10, 2, 24), (3, 4, 0, 2, 24), (3, 4, 257, 2, 24),
                (3, 4, 10, 0, 24), (3, 4, 10, 2, 1), (3, 4, 10, 2, 2 ** 32)):
        assert ok(*bad) == -22, bad


def test_state_words_round_trip_and_refuse_a_cached_gaussian():
    from deeprl_amd import seed_batch
    rs = np.random.RandomState(12)
    rs.randint(5, size=7)
    words = seed_batch.np_mt_words(rs)
    assert words.dtype == np.uint32 and words.shape == (seed_batch.NP_MT_STATE_WORDS,) and words[624] == rs.get_state()[2]
    twin = seed_batch.np_mt_restore(np.random.RandomState(), words)
    assert np.array_equal(twin.randint(0, 1 << 30, size=5), rs.randint(0, 1 << 30, size=5))
    rs.standard_normal()
    with pytest.raises(ValueError, match="cached Gaussian"):
        seed_batch.np_mt_words(rs)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_np_mt_common", "dra_np_mt_state"])
def test_np_mt_struct_mirrors_match_the_header(tmp_path, which):
    """tests/test_struct_layouts.py's probe over the two np_mt structs, and the header's constants against the Python side's."""
    from deeprl_amd import seed_batch
    mirror = dict(dra_np_mt_common=seed_batch.NpMtCommon, dra_np_mt_state=seed_batch.NpMtState)[which]
    names = [f[0] for f in mirror._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "include/deeprl_amd.h"', 'int main(void) {',
           '  printf("%%zu\\n", sizeof(%s));' % which]
    src += ['  printf("%%zu\\n", offsetof(%s, %s));' % (which, f) for f in names]
    src += ['  printf("%d\\n%d\\n", DRA_NP_MT_STATE_WORDS, DRA_NP_MT_ERR_BUDGET);', '  return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", str(c), "-I", ROOT, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(mirror) and got[1:-2] == [getattr(mirror, n).offset for n in names]
    assert got[-2:] == [seed_batch.NP_MT_STATE_WORDS, seed_batch.NP_MT_ERR_BUDGET]
    assert ctypes.sizeof(seed_batch.NpMtState) % 16 == 0
