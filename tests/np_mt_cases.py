"""The case grid and the numpy oracle of the np_mt tests (test_np_mt_host.py: the host entry; test_gpu_np_mt_draws.py: the kernel).
The oracle is np.random.RandomState itself, driven through the two functions the seed lanes draw with."""
import ctypes
import itertools

import numpy as np

# starting states: fresh seeds (pos == 624), and the key of a seed with pos set by hand -- 0, 1, 300; 623 and 622 put the
# regeneration between the words of the first draws
STARTS = (("seed", 0), ("seed", 3), ("seed", 12345), ("pos", 7, 0), ("pos", 8, 1), ("pos", 9, 300), ("pos", 10, 623), ("pos", 11, 622))
N_ACTIONS = (1, 2, 3, 6)          # 1 takes no word; 3 and 6 reject past the mask
KS = (1, 4)
BATCHES = (1, 10, 64)
# (size, pos), capacity = size where full: one valid slot | full at the seam | full | not full | 2^5 + 1: the worst mask rejection
# | 2^5: none | large
RINGS = ((2, 2), (24, 0), (24, 7), (17, 17), (33, 5), (32, 31), (10000, 1234))
EPSILONS = ("one", "zero", "0.37", "linear")      # the int 1 (always explore), 0.0 (never), a constant, a LinearSchedule run


def _cycle(values, i):
    return values[i % len(values)]


def _grid():
    cases = []
    for i, (start, ring) in enumerate(itertools.product(STARTS, RINGS)):
        cases.append((start, _cycle(N_ACTIONS, i), _cycle(KS, i // 2), _cycle(BATCHES, i // 3), ring, _cycle(EPSILONS, i // 5)))
    for i, (n_actions, k, batch, eps) in enumerate(itertools.product(N_ACTIONS, KS, BATCHES, EPSILONS)):
        cases.append((_cycle(STARTS, i), n_actions, k, batch, _cycle(RINGS, i // 3), eps))
    return cases


CASES = _grid()


def case_id(case):
    start, n_actions, k, batch, ring, eps = case
    return "%s-a%d-k%d-b%d-ring%dat%d-eps_%s" % ("_".join(str(x) for x in start), n_actions, k, batch, ring[0], ring[1], eps)


def start_state(start):
    rs = np.random.RandomState(start[1])
    if start[0] == "pos":
        kind, key, _, _, _ = rs.get_state()
        rs.set_state((kind, key, start[2], 0, 0.0))
    return rs


def make_schedule(kind):
    from deeprl_amd.support import LinearSchedule
    if kind == "linear":
        return LinearSchedule(0.9, 0.05, 700)
    value = dict(one=1, zero=0.0)[kind] if kind in ("one", "zero") else float(kind)
    return lambda: value


def valid(i, pos, size):
    """UniformReplay.valid_index at history_length = n_step = 1."""
    return (i >= 0 and i + 1 < pos) or (i >= pos and i + 1 < size)


def numpy_step(rs, schedule, k, batch, n_actions, ring, learn):
    """One lane step drawn by numpy from `rs`: the reference of every comparison."""
    from deeprl_amd.replay import draw_uniform_indices
    from deeprl_amd.support import plan_actor_epsilon_greedy
    size, pos = ring
    eps = []

    def recorded():
        eps.append(schedule())
        return eps[-1]
    explore, rand = plan_actor_epsilon_greedy(recorded, k, n_actions, 0, 0, rng=rs)
    idx = draw_uniform_indices(size, pos, batch, 1, 1, rng=rs) if learn else None
    return dict(explore=explore, rand=rand, idx=idx, eps=eps, slot0=(pos - k) % size)


def layout(k, batch):
    from deeprl_amd.seed_batch import lane_layout
    return lane_layout(k, batch)


def fill_common(c, eps, slot0, ring):
    c.slot0, c.ring_size, c.ring_pos = slot0, ring[0], ring[1]
    for t, e in enumerate(eps):
        c.eps[t] = e


class HostLane:
    """One lane's state and block in host memory, stepped by dra_np_mt_draw_host."""

    def __init__(self, rs, k, batch, n_actions):
        from deeprl_amd import seed_batch
        self.k, self.batch, self.n_actions = k, batch, n_actions
        self.lay = layout(k, batch)
        self.words = seed_batch.np_mt_words(rs)
        self.block = np.zeros(self.lay['stride'], dtype=np.uint8)
        self.common = seed_batch.NpMtCommon()
        self.err = ctypes.c_int(0)

    def step_raw(self, eps, slot0, ring, learn):
        from deeprl_amd._lib import lib
        fill_common(self.common, eps, slot0, ring)
        lay = self.lay
        return lib.dra_np_mt_draw_host.raw(self.words.ctypes.data, self.block.ctypes.data, ctypes.byref(self.common), ctypes.byref(self.err),
                                           self.k, self.batch, self.n_actions, int(learn), lay['idx'], lay['rand'], lay['flag'])

    def step(self, eps, slot0, ring, learn):
        assert self.step_raw(eps, slot0, ring, learn) == 0

    def key(self):
        return self.words[:624]

    def pos(self):
        return int(self.words[624])

    def slot0(self):
        return int(self.block[:8].view(np.int64)[0])

    def idx(self):
        return self.block[self.lay['idx']:self.lay['rand']].view(np.int64)

    def rand(self):
        return self.block[self.lay['rand']:self.lay['flag']].view(np.int64)

    def flags(self):
        return self.block[self.lay['flag']:self.lay['flag'] + self.k].astype(np.bool_)
