"""Edge-shape cases and references for the replay data path: csrc/ring.hip (put / put_host / put_rows, the frame-stack +
n-step gather in its two output forms, the uint8 -> float32 table kernels, dra_gather_rows), csrc/sumtree.hip (update, the
three adds, commit_f32, sample) and the stand-alone launch of csrc/per_chain2.h.  NOT a test file: pure numpy on the CPU,
imported by tests/test_replay_edge_cases_host.py (which proves on the CPU that every case reaches the path it is named for,
that the references agree with the reference project's own classes and that the inputs tell a subtly wrong kernel from a
right one) and by tests/test_gpu_replay_edges.py (which holds the kernels to them); tests/test_gpu_per_chain2.py shares the
restatement of the device draw.

References
  ring      a plain numpy record of what was put (RingContents); gather = slices of it (replay.py:112-134)
  fold      the Python loop cum = r + (m * gamma) * cum in float64, mask `cum_m and m` (replay.py:135-139)
  trees     oracle/sumtree_oracle.py (add, update with pending gating, get)
  draw      replay.py:164-196 spelled out over that oracle (DrawRef)
Everything is compared BIT FOR BIT except priorities that went through powf (alpha != 0.5) and the importance weights:
rtol 1e-6 against float64 pow rounded to float32 (POW_RTOL, the bar tests/test_gpu_per_chain2.py has always used); the
oracle is then fed the device's own priorities so that tree, leaves, totals and probabilities stay bit-exact.

The dispatch conditions of the launchers are restated here (gather_dispatch, lut_blocks, ...) so that the host test can
assert, case by case, which kernel variant, how many loop trips and which branch a case reaches."""
import random

import numpy as np

from oracle.sumtree_oracle import SumTreeOracle

POW_RTOL = 1e-6
SLACK = 64            # bytes of 0xA5 behind every gather output
SLACK_BYTE = 0xA5
RING_CAP = 48         # every ring case: capacity <= 64 slots
WG = 256              # workgroup size of the ring kernels
STREAM_BYTES = 256 << 20
LUT_GRID_CAP = 2048
LUT_ROWS_GRID_CAP = 4096
GATHER_CHUNK = 4096
K_TOP_NODES = 2047    # per_chain2.h kTopNodes
NT = 1024             # threads of the stand-alone per_chain2 launch
F = np.float32


# ================================================================================================ ring contents and gather
class RingContents:
    """What a ring of `capacity` slots holds after slot s was put frame / action / reward / mask [s]."""

    def __init__(self, capacity, frame_bytes, action_bytes, seed, rewards=None, masks=None):
        rs = np.random.RandomState(seed)
        self.capacity, self.frame_bytes, self.action_bytes = capacity, frame_bytes, action_bytes
        self.frames = rs.randint(0, 256, size=(capacity, frame_bytes)).astype(np.uint8)
        self.actions = rs.randint(0, 256, size=(capacity, action_bytes)).astype(np.uint8)
        # float64 rewards with all 52 mantissa bits in use: none is float32-representable
        self.rewards = rs.uniform(-2, 2, size=capacity) if rewards is None else np.asarray(rewards, dtype=np.float64)
        self.masks = (rs.rand(capacity) > 0.25).astype(np.int32) if masks is None else np.asarray(masks, dtype=np.int32)


def fold(rewards, masks, i, n, discount):
    """replay.py:135-139 for index i, in Python floats (float64), association (m * gamma) * cum."""
    cum_r, cum_m = 0.0, 1
    for k in range(n - 1, -1, -1):
        m = int(masks[i + k])
        cum_r = float(rewards[i + k]) + (m * float(discount)) * cum_r
        cum_m = cum_m and m
    return cum_r, cum_m


def ref_gather(c, idx, history, n_step, discount):
    """replay.py:112-140 for a batch of indices: state = frames [i - H + 1, i], next_state the same run n later; block = the
    whole run of H + n frames once (state = block[:, :H], next_state = block[:, n:])."""
    idx = np.asarray(idx, dtype=np.int64)
    run = idx[:, None] - history + 1 + np.arange(history + n_step)[None, :]
    block = c.frames[run]
    rm = [fold(c.rewards, c.masks, int(i), n_step, discount) for i in idx]
    reward = np.asarray([r for r, _ in rm], dtype=np.float64)
    mask = np.asarray([m for _, m in rm], dtype=np.int32)
    with np.errstate(over="ignore"):
        reward_f32 = reward.astype(np.float32)
    return dict(block=block, state=block[:, :history], next_state=block[:, n_step:], action=c.actions[idx], reward=reward, mask=mask,
                reward_f32=reward_f32, mask_f32=mask.astype(np.float32))


def index_range(capacity, history, n_step):
    """Indices whose whole run [i - H + 1, i + n] lies inside the ring (what the gather kernel dereferences)."""
    return history - 1, capacity - 1 - n_step


def gather_indices(capacity, history, n_step, batch, seed):
    """`batch` in-range indices: both ends of the range first, then seeded draws (repeats once batch > the range)."""
    lo, hi = index_range(capacity, history, n_step)
    rs = np.random.RandomState(seed)
    idx = rs.randint(lo, hi + 1, size=batch).astype(np.int64)
    idx[0] = hi
    if batch > 1:
        idx[1] = lo
    return idx


def gather_dispatch(frame_bytes, history, n_step, batch, block, out_aligned=True):
    """ring_gather_launch + the copy loop of ring_gather_kernel, restated.  Returns path ('vec' / 'byte'), stream (the
    nontemporal-store variant), trips (of the longest lane), second (the set of values the guard `t + 256 < nv` takes
    over every lane and trip) and byte_trips."""
    vec = frame_bytes % 16 == 0 and out_aligned
    out_bytes = batch * ((history + n_step) if block else 2 * history) * frame_bytes
    d = dict(path="vec" if vec else "byte", stream=bool(vec and out_bytes >= STREAM_BYTES), out_bytes=out_bytes, trips=0, second=set(),
             byte_trips=0)
    if vec:
        nv = frame_bytes >> 4
        for lane in range(WG):
            trips, t = 0, lane
            while t < nv:
                d["second"].add(t + WG < nv)
                t += 2 * WG
                trips += 1
            d["trips"] = max(d["trips"], trips)
    else:
        d["byte_trips"] = -(-frame_bytes // WG)
    return d


_PAIRS = [(1, 1), (4, 1), (4, 3), (3, 3), (2, 5)]
VEC_NV = [1, 255, 256, 257, 511, 512, 513, 1025]
BYTE_SIZES = [1, 15, 17, 255, 257, 513]
# nv -> (trips, guard seen True, guard seen False), written down by hand from the loop: lane t moves vectors t and t + 256
# of every 512
VEC_EXPECT = {1: (1, False, True), 255: (1, False, True), 256: (1, False, True), 257: (1, True, True), 511: (1, True, True),
              512: (1, True, False), 513: (2, True, True), 1025: (3, True, True)}


def _gather_cases():
    cases = []
    k = 0
    for nv in VEC_NV:
        h, n = _PAIRS[k % len(_PAIRS)]
        cases.append(dict(name="vec_nv%d_h%dn%d" % (nv, h, n), frame_bytes=16 * nv, history=h, n_step=n, batch=1 if k % 3 == 0 else 5,
                          misaligned=False))
        k += 1
    for fb in BYTE_SIZES:
        h, n = _PAIRS[k % len(_PAIRS)]
        cases.append(dict(name="byte_%d_h%dn%d" % (fb, h, n), frame_bytes=fb, history=h, n_step=n, batch=1 if k % 3 == 0 else 5,
                          misaligned=False))
        k += 1
    # every (history, n_step) pair on both paths, with a batch larger than the capacity (repeated indices)
    for h, n in _PAIRS:
        cases.append(dict(name="pairs_vec_h%dn%d" % (h, n), frame_bytes=48, history=h, n_step=n, batch=RING_CAP + 22, misaligned=False))
        cases.append(dict(name="pairs_byte_h%dn%d" % (h, n), frame_bytes=33, history=h, n_step=n, batch=RING_CAP + 22, misaligned=False))
    cases.append(dict(name="byte_by_misalignment_4096", frame_bytes=4096, history=4, n_step=1, batch=3, misaligned=True))
    for c in cases:
        c.update(capacity=RING_CAP, action_bytes=8, discount=0.99, seed=100 + len(c["name"]) + c["frame_bytes"])
    return cases


GATHER_CASES = _gather_cases()
STREAM_CASES = [
    dict(name="stream_two_2048", frame_bytes=16400, history=4, n_step=1, batch=2048, block=False, stream=True),
    dict(name="stream_two_2046_below", frame_bytes=16400, history=4, n_step=1, batch=2046, block=False, stream=False),
    dict(name="stream_block_3274", frame_bytes=16400, history=4, n_step=1, batch=3274, block=True, stream=True),
]
for _c in STREAM_CASES:
    _c.update(capacity=RING_CAP, action_bytes=8, discount=0.99, seed=7)


# ------------------------------------------------------------------------------------------------ fold
FOLD_DISCOUNTS = [0.0, 1.0, 0.99]


def fold_case(n, discount, wide_masks=False):
    """A 16-byte-frame ring whose masks put a terminal at every position of an n-step run and at none: mask[j] = 0 iff
    j % (n + 1) == n.  Rewards: full-mantissa float64, with -0.0 and +-1e300 planted.  wide_masks: masks 2 and 3 among the
    ones -- the ring multiplies by the int32 it stores, and only a factor other than 0 / 1 tells (m * gamma) * cum from
    m * (gamma * cum) (with m in {0, 1} both products are exact)."""
    cap = RING_CAP
    rs = np.random.RandomState(1000 * n + int(100 * discount) + (7 if wide_masks else 0))
    rewards = rs.uniform(-3, 3, size=cap)
    rewards[rs.permutation(cap)[:9]] = [-0.0, -0.0, 1e300, -1e300, 1e300, -0.0, -1e300, 0.1, 1.0 / 3.0]
    masks = np.ones(cap, dtype=np.int32)
    if wide_masks:
        masks[:] = rs.randint(1, 4, size=cap)
    masks[np.arange(cap) % (n + 1) == n] = 0
    lo, hi = index_range(cap, 1, n)
    return dict(name="fold_n%d_g%s%s" % (n, discount, "_wide" if wide_masks else ""), capacity=cap, frame_bytes=16, action_bytes=8,
                history=1, n_step=n, discount=discount, seed=n, rewards=rewards, masks=masks,
                idx=np.arange(lo, hi + 1, dtype=np.int64))


FOLD_CASES = [fold_case(n, g) for n in range(1, 6) for g in FOLD_DISCOUNTS] + [fold_case(n, 0.99, True) for n in range(2, 6)]


def terminal_positions(case):
    """For every index of a fold case: the first position k of its run with mask 0, or -1."""
    out = []
    for i in case["idx"]:
        z = [k for k in range(case["n_step"]) if case["masks"][i + k] == 0]
        out.append(z[0] if z else -1)
    return out


# ------------------------------------------------------------------------------------------------ put
PUT_ACTION_BYTES = [1, 4, 8, 48, 256, 264]
PUT_COUNTS = [1, 7, 16]     # the last one is the put ring's whole capacity
PUT_CAP = 16
PUT_HOST_FEEDS = 130        # of 7056-byte frames into a 64-slot ring: its 64-slot staging ring wraps twice
PUT_HOST_FRAME = 7056
STAGE_SLOTS = 64


def action_from_value(value, action_bytes):
    """ring_put_kernel's by-value action: the little-endian bytes of the int64, zeros beyond 8."""
    b = np.zeros(action_bytes, dtype=np.uint8)
    raw = np.asarray([value], dtype="<i8").view(np.uint8)
    b[:min(8, action_bytes)] = raw[:min(8, action_bytes)]
    return b


# ------------------------------------------------------------------------------------------------ table kernels, row gather
LUT_N = [1, 15, 16, 17, 4097, 16 * (LUT_GRID_CAP * WG) + 16 + 5]
LUT_ROWS = [dict(rows=1030, elems=16384, stride=16400), dict(rows=3, elems=16, stride=16)]


def lut_blocks(n):
    """dra_u8_to_f32_lut's grid and what a case makes of it: blocks, vector trips of the busiest lane, tail elements."""
    n16 = n >> 4
    blocks = min(max((n16 + WG - 1) // WG, 1), LUT_GRID_CAP)
    return dict(blocks=blocks, trips=-(-n16 // (blocks * WG)) if n16 else 0, tail=n - 16 * n16, capped=(n16 + WG - 1) // WG > LUT_GRID_CAP)


def lut_rows_blocks(rows, elems):
    total = rows * (elems >> 4)
    blocks = min((total + WG - 1) // WG, LUT_ROWS_GRID_CAP)
    return dict(blocks=blocks, trips=-(-total // (blocks * WG)), capped=(total + WG - 1) // WG > LUT_ROWS_GRID_CAP, vectors=total)


def lut_input(n, seed=3):
    """n bytes in which every byte value occurs once n >= 256 (the first 256 are a permutation)."""
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 256, size=n).astype(np.uint8)
    if n >= 256:
        x[:256] = rs.permutation(256).astype(np.uint8)
    return x


GATHER_ROWS_BYTES = [4096, 4097, 4112, 8192]
GATHER_ROWS_SRC = 11        # source rows
GATHER_ROWS_IDX = [-GATHER_ROWS_SRC, GATHER_ROWS_SRC - 1, 0, 5, -1, 5]


def gather_rows_dispatch(row_bytes, aligned=True):
    """gather_rows_kernel: chunks per row, 16-byte or byte path, trips of the byte loop in the fullest chunk."""
    vec = row_bytes % 16 == 0 and aligned
    return dict(chunks=-(-row_bytes // GATHER_CHUNK), vec=vec, byte_trips=0 if vec else -(-min(row_bytes, GATHER_CHUNK) // WG))


# ================================================================================================ sum tree
TREE_CAPS = [1, 2, 3, 5, 7, 8, 9, 1000, 1023, 1024, 1025]


class TreeRef(SumTreeOracle):
    """oracle/sumtree_oracle.py with one change: the walk to the root stops AT the root, so that a one-leaf tree (whose
    only leaf is the root; the reference's own _propagate recurses for ever there) has a reference too.  Identical for
    every capacity >= 2 (the host test compares)."""

    def update(self, idx, p):
        idx = int(idx)
        if idx not in self.pending:
            return False
        self.pending.remove(idx)
        delta_add(self.tree, idx, p)
        return True


def leaf_depths(capacity):
    """The set of depths the leaves of a `capacity`-leaf heap live on (root = 0)."""
    depths = set()
    for leaf in range(capacity - 1, 2 * capacity - 1):
        d, node = 0, leaf
        while node > 0:
            node = (node - 1) // 2
            d += 1
        depths.add(d)
    return depths


def f32_priorities(rs, n, lo_exp=-3, hi_exp=2):
    """float32-valued priorities 2^[lo_exp, hi_exp) with full 24-bit mantissas, as float64."""
    return (np.exp2(rs.uniform(lo_exp, hi_exp, size=n)) * rs.uniform(1.0, 1.5, size=n)).astype(np.float32).astype(np.float64)


def exact_regime(capacity, hi, lo):
    """The bound dra_sumtree_commit_f32 / per_chain2 / set_many_from check: True = the level-parallel update is exact."""
    if not (lo > 0.0) or not np.isfinite(hi):
        return False
    ilogb = int(np.frexp(lo)[1]) - 1
    return not (float(capacity) * hi > np.ldexp(1.0, 53 + ilogb - 23))


def filled_oracle(capacity, seed, lo_exp=-3, hi_exp=2):
    """An oracle whose `capacity` leaves were added at seeded float32-valued priorities."""
    rs = np.random.RandomState(seed)
    orc = TreeRef(capacity)
    for p in f32_priorities(rs, capacity, lo_exp, hi_exp):
        orc.add(float(p))
    return orc


def update_cases():
    """(capacity, n): every leaf in one launch for capacities <= 1024; a second wave and all 16 waves on 1025."""
    return [(c, c) for c in TREE_CAPS if c <= 1024] + [(1025, 65), (1025, 1024)]


def update_inputs(capacity, n, ordered, seed=0):
    """n unique leaves in a seeded order and their new priorities: float32-valued for the parallel mode, arbitrary float64
    spanning 2^-40 .. 2^20 for the ordered one (where only the reference's own order of additions gives its bits)."""
    rs = np.random.RandomState(31 * capacity + n + seed)
    leaves = (rs.permutation(capacity)[:n] + capacity - 1).astype(np.int64)
    prio = f32_priorities(rs, n) if not ordered else np.exp2(rs.uniform(-40, 20, size=n)) * rs.uniform(1.0, 2.0, size=n)
    return leaves, prio


def oracle_updates(orc, leaves, prio):
    for leaf, p in zip(leaves, prio):
        orc.pending.add(int(leaf))
        orc.update(int(leaf), float(p))


def delta_add(tree, leaf, p):
    """sum_tree.py:39-60 on a bare heap array: add is update, tree[ancestor] += (p - old)."""
    change = p - tree[leaf]
    tree[leaf] = p
    node = leaf
    while node > 0:
        node = (node - 1) // 2
        tree[node] += change


def recompute_add(tree, leaf, p):
    """The WRONG add outside the exactness regime: every ancestor recomputed as left + right."""
    tree[leaf] = p
    node = leaf
    while node > 0:
        node = (node - 1) // 2
        tree[node] = tree[2 * node + 1] + tree[2 * node + 2]


def many_add_plan(capacity):
    """(write0, n) of the set_many_from launch of a capacity: 64 leaves (all of them below 64), wrapping at the capacity."""
    n = min(64, capacity)
    return (capacity - 1 if capacity > 1 else 0), n


FALLBACK_CAPS = [13, 4096]
FALLBACK_ROUNDS = 6


def fallback_many_add(capacity):
    """(write0, n) of the set_many_from launch after the fall-back rounds: five adds that wrap (not every leaf: a tree
    whose leaves are all equal has exact sums again)."""
    return capacity - 2, 5


def fallback_rounds(capacity, seed=6):
    """Rounds of commit_f32 whose float32 priorities span 2^-40 .. 2^20: (leaves, prio_f32) per round, unique leaves."""
    rs = np.random.RandomState(seed + capacity)
    out = []
    for _ in range(FALLBACK_ROUNDS):
        n = min(capacity, 32)
        leaves = (rs.permutation(capacity)[:n] + capacity - 1).astype(np.int64)
        prio = (np.exp2(rs.uniform(-40, 20, size=n)) * rs.uniform(1.0, 2.0, size=n)).astype(np.float32)
        out.append((leaves, prio))
    return out


# ------------------------------------------------------------------------------------------------ sample
SAMPLE_BATCHES = [1, 63, 64, 65, 1024]
U_TOP = float(np.nextafter(1.0, 0.0))


def descend(tree, s, strict=False):
    """sum_tree.py:23-33 on a bare heap; returns (leaf, ties): ties = descents steps that met s == tree[left].
    strict: the WRONG comparison `s < left`."""
    idx, ties, n = 0, 0, len(tree)
    while True:
        left = 2 * idx + 1
        if left >= n:
            break
        lv = tree[left]
        ties += int(s == lv)
        if (s < lv) if strict else (s <= lv):
            idx = left
        else:
            idx = left + 1
            s = s - lv
    return idx, ties


def strata(total, batch, u, wrong=False):
    """s_i = a + (b - a) * u_i with a = seg * i, b = seg * (i + 1), seg = total / batch (python's random.uniform).
    wrong: seg * (i + u)."""
    seg = np.float64(total) / np.float64(batch)
    i = np.arange(batch, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    if wrong:
        return seg * (i + u)
    a, b = seg * i, seg * (i + 1.0)
    return a + (b - a) * u


def ref_sample(tree, u, strict=False, wrong_strata=False):
    batch = len(u)
    s = strata(tree[0], batch, u, wrong_strata)
    leaves, ties = [], 0
    for x in s:
        leaf, t = descend(tree, float(x), strict)
        leaves.append(leaf)
        ties += t
    leaves = np.asarray(leaves, dtype=np.int64)
    return dict(idx=leaves, p=tree[leaves].copy(), total=np.float64(tree[0]), ties=ties)


def sample_us(batch, seed):
    """u = 0 and nextafter(1, 0) in every stratum (two vectors), plus a seeded mix of both with interior draws."""
    rs = np.random.RandomState(seed + batch)
    mix = rs.rand(batch)
    mix[rs.rand(batch) < 0.2] = 0.0
    mix[rs.rand(batch) < 0.2] = U_TOP
    return dict(zero=np.zeros(batch), top=np.full(batch, U_TOP), mix=mix)


def boundary_us(total, batch):
    """For an all-ones tree (every integer is a left-subtree boundary somewhere): u_i that aims stratum i at an integer
    inside it.  total / batch is inexact here, so whether s lands on, below or above the integer depends on the order
    of the roundings: a + (b - a) * u and seg * (i + u) part ways."""
    seg = np.float64(total) / np.float64(batch)
    u = np.full(batch, 0.5)
    for i in range(batch):
        a, b = seg * i, seg * (i + 1.0)
        k = np.ceil(a) + 1.0
        if a < k < b:
            u[i] = min((k - a) / (b - a), U_TOP)
    return u


def sample_trees():
    """name -> heap array.  ones<B>: all-ones leaves, drawn with batch = capacity and u = 0: every s = i sits exactly on a
    left-subtree sum somewhere on its way down."""
    trees = {}
    for cap in (1000, 1025):
        trees["random%d" % cap] = filled_oracle(cap, 77).tree
        orc = TreeRef(cap)
        p = f32_priorities(np.random.RandomState(cap), cap)
        p[::2] = 0.0
        for v in p:
            orc.add(float(v))
        trees["zeros_interleaved%d" % cap] = orc.tree
    trees["all_zero9"] = np.zeros(17)
    orc = TreeRef(1000)
    for _ in range(1000):
        orc.add(1.0)
    trees["ones_cap1000"] = orc.tree
    for b in SAMPLE_BATCHES:
        orc = TreeRef(b)
        for _ in range(b):
            orc.add(1.0)
        trees["ones%d" % b] = orc.tree
    return trees


# ================================================================================================ the device draw (per_chain2)
def valid_index(di, pos, size, h, n):
    """replay.py:122-127"""
    return (di - h + 1 >= 0 and di + n < pos) or (di - h + 1 >= pos and di + n < size)


def mt_words(n_words):
    """The next n_words 32-bit outputs of python's `random`, exactly as replay.DeviceDraw produces them; the generator is
    left where it was."""
    st0 = random.getstate()
    w = np.frombuffer(random.getrandbits(32 * n_words).to_bytes(4 * n_words, "little"), dtype="<u4").copy()
    random.setstate(st0)
    return w


def pow_f32(base_f32, exponent_f32):
    """float64 pow of float32 operands, rounded to float32: the reference the device's powf is held to at POW_RTOL."""
    return np.power(np.asarray(base_f32, dtype=np.float32).astype(np.float64), float(F(exponent_f32))).astype(np.float32)


def ref_priorities(loss_f32, eps, alpha):
    """DQN_agent.py:121-123 in float32: (|loss| + eps) ^ alpha; sqrt (correctly rounded: bit-exact) when alpha == 0.5."""
    ad = np.abs(np.asarray(loss_f32, dtype=np.float32)) + F(eps)
    return np.sqrt(ad).astype(np.float32) if F(alpha) == F(0.5) else pow_f32(ad, alpha)


def ref_weights(samp_prob_f32, batch, beta):
    """DQN_agent.py:124-126: (P * B + 1e-6) ^ -beta over their max."""
    w = pow_f32(np.asarray(samp_prob_f32, dtype=np.float32) * F(batch) + F(1e-6), -F(beta))
    return w / w.max()


class DrawRef:
    """replay.py:164-196 over the oracle tree, one agent step at a time, in the reference's order update_priorities ->
    feed x add_n -> sample; python's `random` is the uniform source."""

    def __init__(self, capacity, batch, history, n_step, size0=None):
        self.cap, self.batch, self.h, self.n = capacity, batch, history, n_step
        self.orc = TreeRef(capacity)
        size0 = min(capacity, 3 * capacity // 4 + 7) if size0 is None else size0
        for _ in range(size0):
            self.orc.add(1.0)
        self.pos, self.size, self.max_p, self.min_p = size0 % capacity, size0, 1.0, 1.0

    def commit(self, cur_idx, prio, last_writer=False):
        """last_writer: the WRONG gating (the last occurrence of a leaf in the minibatch wins)."""
        pairs = list(zip(cur_idx, prio))
        for idx, p in (reversed(pairs) if last_writer else pairs):
            self.max_p = max(self.max_p, float(p))
            self.min_p = min(self.min_p, float(p))
            self.orc.update(idx, float(p))

    def adds(self, add_n, recompute=False):
        """recompute: the WRONG add outside the exactness regime (ancestors rebuilt as left + right)."""
        for _ in range(add_n):
            if recompute:
                orc = self.orc
                leaf = orc.write + self.cap - 1
                orc.pending.discard(leaf)
                recompute_add(orc.tree, leaf, self.max_p)
                orc.write = (orc.write + 1) % self.cap
            else:
                self.orc.add(self.max_p)
            if self.pos >= self.size:
                self.size += 1
            self.pos = (self.pos + 1) % self.cap

    def draw(self, u=None):
        """Returns raw leaves, the padded minibatch's leaves and priorities, total, n_valid.  u: fixed uniforms instead of
        `random` (a dry word ring makes the kernel draw with u = 0 and pad with its first valid draw)."""
        orc, batch = self.orc, self.batch
        total = orc.total()
        seg = total / batch
        picked, raw = [], []
        for i in range(batch):
            a, b = seg * i, seg * (i + 1)
            s = random.uniform(a, b) if u is None else a + (b - a) * u[i]
            idx, p, di = orc.get(s)
            raw.append(idx)
            if valid_index(di, self.pos, self.size, self.h, self.n):
                picked.append((idx, p))
        n_valid = len(picked)
        if n_valid == 0:     # the reference would loop forever; the kernel reports flag 2 and keeps the indices in range
            picked = [(self.cap - 1 + self.h, 0.0)] * batch
        while len(picked) < batch:
            picked.append(random.choice(picked) if u is None else picked[0])
        return raw, [t[0] for t in picked], [t[1] for t in picked], total, n_valid


PER_CASES = [
    # name, capacity, batch, add_n, history, n_step, alpha, eps, loss kind, rounds
    dict(name="cap300_b1_a1", cap=300, batch=1, add_n=1),
    dict(name="cap300_b8_a0", cap=300, batch=8, add_n=0),
    dict(name="cap300_b9_a4", cap=300, batch=9, add_n=4),
    dict(name="cap8_b32_a2_duplicates", cap=8, batch=32, add_n=2, history=2),
    dict(name="cap1024_b64_a8_top_exact", cap=1024, batch=64, add_n=8),
    dict(name="cap1025_b64_a8_top_plus2", cap=1025, batch=64, add_n=8),
    dict(name="cap4096_b1024_a0", cap=4096, batch=1024, add_n=0, rounds=6),
    dict(name="cap4096_b1024_a8_level_by_level", cap=4096, batch=1024, add_n=8, rounds=6),
    dict(name="cap300_b32_a4_add_hits_committed_leaf", cap=300, batch=32, add_n=4, collide=True),
    dict(name="cap300_b32_a4_alpha07", cap=300, batch=32, add_n=4, alpha=0.7),
    dict(name="cap300_b32_a4_unforced_ordered", cap=300, batch=32, add_n=4, eps=0.0, loss="wide"),
    dict(name="cap4096_b64_a8_unforced_ordered", cap=4096, batch=64, add_n=8, eps=0.0, loss="wide"),
    dict(name="cap300_b32_a4_word_ring_dry", cap=300, batch=32, add_n=4, rounds=6, final="dry"),
    dict(name="cap300_b32_a4_no_valid_leaf", cap=300, batch=32, add_n=4, rounds=6, final="no_valid"),
]
for _c in PER_CASES:
    for _k, _v in dict(history=4, n_step=1, alpha=0.5, eps=0.01, loss="normal", rounds=8, collide=False).items():
        _c.setdefault(_k, _v)


def per_losses(case, rs, r):
    """The float32 loss vector of round r.  'wide': magnitudes 1e-30 .. 1e6 in ONE minibatch (with eps = 0 the priorities
    span 1e-15 .. 1e3: outside the exactness bound for every capacity here)."""
    b = case["batch"]
    if case["loss"] == "wide":
        mag = np.power(10.0, rs.uniform(-30, 6, size=b))
        if b >= 2:
            i = rs.randint(b)
            mag[i], mag[(i + 1 + rs.randint(b - 1)) % b] = 1e-30, 1e6
        return (mag * rs.choice([-1.0, 1.0], size=b)).astype(np.float32)
    return (rs.randn(b) * (3.0 if r % 3 else 0.05)).astype(np.float32)


class PerRun:
    """The rounds of one per_chain2 case, shared by the host test (which checks what the rounds reach) and the GPU test (which
    holds the kernel to them): begin() gives a round's inputs, finish(prio) applies the reference's update_priorities ->
    feed x add_n -> sample with the priorities given (the reference's own, or the device's where they went through powf)
    and returns everything the launch must have produced.  final: 'dry' / 'no_valid' turn the LAST round into the word
    ring running dry (flag 1) / a ring state without one valid index (flag 2).  recompute_adds / last_writer: mutants."""

    def __init__(self, case, n_words=40000, recompute_adds=False, last_writer=False):
        self.case, self.n_words = case, n_words
        self.recompute_adds, self.last_writer = recompute_adds, last_writer
        cap, batch = case["cap"], case["batch"]
        self.rs = np.random.RandomState(cap + batch)
        self.ref = DrawRef(cap, batch, case["history"], case["n_step"])
        random.seed(cap)
        _, self.cur_idx, _, _, _ = self.ref.draw()
        self.words = mt_words(n_words)
        self.write = self.ref.orc.write
        self.beta, self.r, self.consumed = 0.4, 0, 0

    def begin(self):
        case, ref = self.case, self.ref
        cap, add_n = case["cap"], case["add_n"]
        last = self.r == case["rounds"] - 1
        self.final = case.get("final") if last else None
        if case["collide"] and self.r % 2 == 1:
            # the write cursor onto the first leaf of the minibatch being committed: the add's value must stand
            di = int(self.cur_idx[0]) - (cap - 1)
            ref.orc.write = ref.pos = self.write = di
        pos, size = ref.pos, ref.size
        for _ in range(add_n):
            if pos >= size:
                size += 1
            pos = (pos + 1) % cap
        if self.final == "no_valid":
            pos, size = 0, 0
        self.pos_after, self.size_after = pos, size
        self.loss = per_losses(case, self.rs, self.r)
        return dict(loss=self.loss, add_n=add_n, write0=self.write, pos_after=pos, size_after=size, beta=self.beta,
                    rng_produced=self.consumed if self.final == "dry" else self.n_words)

    def finish(self, prio):
        case, ref = self.case, self.ref
        cap, batch, add_n = case["cap"], case["batch"], case["add_n"]
        adds = [(self.write + i) % cap + cap - 1 for i in range(add_n)]
        collisions = sorted(set(adds) & set(int(i) for i in self.cur_idx))
        duplicates = batch - len(set(int(i) for i in self.cur_idx))
        ref.commit(self.cur_idx, prio, self.last_writer)
        ordered = not exact_regime(cap, ref.max_p, ref.min_p)
        ref.adds(add_n, self.recompute_adds)
        ref.pos, ref.size = self.pos_after, self.size_after
        self.write = (self.write + add_n) % cap
        before = random.getstate()
        raw, idx, p, total, n_valid = ref.draw(np.zeros(batch) if self.final == "dry" else None)
        after = random.getstate()
        flags = (1 if self.final == "dry" else 0) | (2 if n_valid == 0 else 0)
        out = dict(tree=ref.orc.tree.copy(), stat=[ref.max_p, ref.min_p], raw=raw, idx=idx, p=p, total=total, n_valid=n_valid, flags=flags,
                   before=before, after=after, beta=self.beta, ordered=ordered, branch=per_branch(case, ordered), collisions=collisions,
                   duplicates=duplicates, seq=self.r + 1)
        self.cur_idx = idx
        self.beta = min(1.0, self.beta + 0.05)
        self.r += 1
        return out


def per_branch(case, ordered):
    """Which commit / add branch of per_chain2_body a round takes."""
    if ordered:
        return "ordered"
    return "atomic" if case["batch"] + case["add_n"] <= NT else "level"
