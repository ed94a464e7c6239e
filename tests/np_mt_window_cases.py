"""The ring states and the numpy oracle of the np_mt window tests (test_np_mt_window_host.py: the host entry;
test_gpu_dqn_replay_lanes_kernels.py: the kernel): np_mt_cases.py's lane and oracle over an n-step window.  The oracle is
np.random.RandomState itself, driven through support.plan_actor_epsilon_greedy and replay.draw_uniform_indices(..., n_step=n)."""
import ctypes

import numpy as np

import np_mt_cases as C

CAPACITY, BATCH, K, N_ACTIONS = 24, 10, 4, 2
N_STEPS = (1, 2, 3, 8)
# the generator's pos at the step's start: one word before the twist, on it (a fresh seed stands there), and mid-key
STARTS = (("pos", 21, 623), ("seed", 5), ("pos", 22, 300))


def rings(n):
    """(name, (size, pos)) of a ring of CAPACITY slots under a window of n: the low range [0, pos - n) empty in a full ring (at
    its edge pos == n, and at pos 0); the high range [pos, size - n) empty in a full ring (at its edge) and in one that has not
    wrapped (size == pos); exactly ONE valid slot (n + 1 rows, not wrapped: slot 0); both ranges populated."""
    return (("low_empty", (CAPACITY, n)), ("low_empty_pos0", (CAPACITY, 0)), ("high_empty", (CAPACITY, CAPACITY - n)),
            ("high_empty_unwrapped", (17, 17)), ("one_valid", (n + 1, n + 1)), ("both", (CAPACITY, 11)))


def valid(i, pos, size, n):
    """UniformReplay.valid_index at history_length = 1."""
    return (i >= 0 and i + n < pos) or (i >= pos and i + n < size)


def count_words(before, k, n_actions, size, idx, limit):
    """How many 32-bit words numpy took for one lane step that started at get_state() `before` and drew the indices `idx` (None:
    the step did not learn), counted on the raw stream: a copy of the generator hands out `limit` raw words (randint over the full
    uint32 range takes exactly one each), and the step is walked over them -- per transition randint's masked attempts, then rand's
    two words; then one word per attempt of randint(0, size), the accepted ones in order being numpy's candidates, of which the
    valid ones are `idx` in order.  The walk checks itself: the accepted candidates must contain `idx` as it goes, and the last
    word taken is the one that gave idx[-1]."""
    copy = np.random.RandomState()
    copy.set_state(before)
    raw = copy.randint(0, 2 ** 32, size=limit, dtype=np.uint32)
    at = 0

    def below(n):
        nonlocal at
        if n == 1:
            return 0
        mask = (1 << int(n - 1).bit_length()) - 1
        while True:
            v = int(raw[at]) & mask
            at += 1
            if v <= n - 1:
                return v
    for _ in range(k):
        below(n_actions)
        at += 2
    have = 0
    while idx is not None and have < len(idx):
        if below(size) == idx[have]:      # (an invalid candidate never equals the next kept index: that one is valid)
            have += 1
    return at


def numpy_step(rs, eps, k, batch, n_actions, ring, n, learn=True, limit=4096):
    """One lane step drawn by numpy from `rs` with constant epsilon `eps` -> np_mt_cases.numpy_step's dict plus `words`: how many
    32-bit words numpy alone took for it (count_words; an IndexError there means more than `limit`)."""
    from deeprl_amd.replay import draw_uniform_indices
    from deeprl_amd.support import plan_actor_epsilon_greedy
    size, pos = ring
    before = rs.get_state()
    explore, rand = plan_actor_epsilon_greedy(lambda: eps, k, n_actions, 0, 0, rng=rs)
    idx = draw_uniform_indices(size, pos, batch, 1, n, rng=rs) if learn else None
    words = count_words(before, k, n_actions, size, idx, limit)
    assert (rs.get_state()[2] - before[2]) % 624 == words % 624      # (the walk ended where numpy's generator stands)
    return dict(explore=explore, rand=rand, idx=idx, eps=[eps] * k, slot0=(pos - k) % size, words=words)


class WindowLane(C.HostLane):
    """np_mt_cases.HostLane stepped by dra_np_mt_draw_window_host."""

    def __init__(self, rs, k, batch, n_actions, n_step):
        C.HostLane.__init__(self, rs, k, batch, n_actions)
        self.n_step = n_step

    def step_raw(self, eps, slot0, ring, learn):
        from deeprl_amd._lib import lib
        C.fill_common(self.common, eps, slot0, ring)
        lay = self.lay
        return lib.dra_np_mt_draw_window_host.raw(self.words.ctypes.data, self.block.ctypes.data, ctypes.byref(self.common),
                                                  ctypes.byref(self.err), self.k, self.batch, self.n_actions, int(learn), lay['idx'],
                                                  lay['rand'], lay['flag'], self.n_step)
