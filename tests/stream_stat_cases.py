"""Cases, statistics, bars and negative controls for the device-drawn random streams (csrc/gumbel_noise.h, csrc/cont_env.h,
csrc/actor_env.h + csrc/ring.hip).  NOT a test file and no product import: plain numpy in float64, imported by
tests/test_stream_stats_host.py (which proves on the CPU that the restatements below meet the bars with margin, that every negative
control fails the bar it is aimed at, and that the product's host statements draw what the restatements draw) and by
tests/test_gpu_stream_stats.py (which draws the same cases through the kernels).

Every stream is a counter hash mix64(key(seed, stream) + position), position = counter * stride + component.  The restatements
here are written from the header comments, with the PRE-MIX word of every position exposed (`*_words`), so that the stride / cap
sets can be computed from the same code the draws go through.

Bars (derived, not tuned; the cases are deterministic, so they are conditions and not measurements):
  Z_BAR   5.0  every z-type statistic (moments, correlations, Wilson-Hilferty chi-square, Bernoulli rates): two-sided p = 5.7e-7,
               about 300 statistics in this module -> a correct stream fails with probability < 2e-4
  KS_BAR  2.8  Kolmogorov-Smirnov D sqrt(n): 2 exp(-2 2.8^2) = 3.1e-7
  Z_HOST 4.0 / KS_HOST 2.4  what the restatement alone must meet on the CPU: the margin absorbs the last-bit differences of logf /
               cosf between device and host in the two float streams.  A seed or length that fails it is replaced and noted here:
               (none rejected so far)
Every expected count of a chi-square is >= 20 (smaller cells are merged).

Known overlap, recorded and not changed (the streams and the committed fixtures stay): synthetic Atari keys its frames with
`seed`, its reward with `seed + 1` and its terminal with `seed + 2`, and envs.py gives neighbouring environments consecutive seeds.
So the terminal word of environment i at counter c IS the reward word of environment i + 1 at counter c, and both are frame word
c mod 882 of frame c // 882 of environment i + 2.  The distinctness assertion of this family is therefore scoped to one seed, and
the cross statistic `terminal of i against reward and |reward| of i + 1` is held to the same bar: the terminal reads the word
modulo done_period, the reward reads its high half modulo 10."""
import math

import numpy as np

Z_BAR, KS_BAR = 5.0, 2.8
Z_HOST, KS_HOST = 4.0, 2.4
SCORE_GAP = 1e-5          # loss_edge_cases.SCORE_GAP: a Gumbel decision under this margin may differ from float64's
EXEMPT_CAP = 0.01         # ... in at most this fraction of a case's rows
GAUSS_ABS = 1e-5          # the absolute bar of dra_gauss_sample (ppo_mlp_edge_cases: "sample")
MIN_EXPECTED = 20.0

M64 = (1 << 64) - 1
_GOLD = np.uint64(0x9E3779B97F4A7C15)
_EULER = 0.5772156649015329


def u64(x):
    """A python integer (negative or past 2^64 included) as the uint64 a C caller passes: x mod 2^64."""
    return np.uint64(int(x) & M64)


def u64s(xs):
    return np.asarray([int(x) & M64 for x in np.asarray(xs, dtype=object).reshape(-1)], dtype=np.uint64)


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


# ------------------------------------------------------------------------------------------------------------ statistics
def _flat(x):
    return np.asarray(x, dtype=np.float64).reshape(-1)


def z_mean(x, mu, var):
    x = _flat(x)
    return float((x.mean() - mu) / math.sqrt(var / x.size))


def z_moment(x, mu, k, m_k, m_2k):
    """z of the k-th central sample moment about the law's own mean: its variance is (m_2k - m_k^2) / n."""
    x = _flat(x) - mu
    return float(((x ** k).mean() - m_k) / math.sqrt((m_2k - m_k * m_k) / x.size))


def z_corr(a, b, mu_a, sd_a, mu_b, sd_b):
    """sum of products of two samples standardised by their laws' own moments, over sqrt(n): N(0, 1) if they are independent."""
    a, b = _flat(a), _flat(b)
    assert a.size == b.size and a.size > 0
    return float(np.dot(a - mu_a, b - mu_b) / (sd_a * sd_b * math.sqrt(a.size)))


def z_lag(x, axis, mu, sd):
    """lag-1 correlation along one index of a stream."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[axis]
    return z_corr(np.take(x, np.arange(n - 1), axis=axis), np.take(x, np.arange(1, n), axis=axis), mu, sd, mu, sd)


def z_rate(k, n, p):
    return float((k - n * p) / math.sqrt(n * p * (1.0 - p)))


def merge_cells(counts, expected):
    """Cells in order of their expected counts, the smallest merged until every cell expects >= MIN_EXPECTED."""
    counts, expected = _flat(counts), _flat(expected)
    order = np.argsort(expected, kind="stable")
    c, e, out_c, out_e = 0.0, 0.0, [], []
    for i in order:
        c, e = c + counts[i], e + expected[i]
        if e >= MIN_EXPECTED:
            out_c.append(c), out_e.append(e)
            c, e = 0.0, 0.0
    if e > 0.0:           # a remainder under the bar joins the last cell
        assert out_e, "chi-square: the whole sample expects fewer than %g counts" % MIN_EXPECTED
        out_c[-1] += c
        out_e[-1] += e
    return np.asarray(out_c), np.asarray(out_e)


def chi2_z(counts, expected):
    """Pearson chi-square of counts against expected counts as the Wilson-Hilferty z: (X2 / df)^(1/3) is close to normal with mean
    1 - 2 / (9 df) and variance 2 / (9 df)."""
    c, e = merge_cells(counts, expected)
    assert abs(c.sum() - e.sum()) <= 1e-6 * e.sum() and e.min() >= MIN_EXPECTED and c.size >= 2
    df = c.size - 1
    x2 = float(((c - e) ** 2 / e).sum())
    return float(((x2 / df) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * df))) / math.sqrt(2.0 / (9.0 * df)))


def ks_stat(x, cdf):
    """D sqrt(n) of a sample against a continuous CDF (a vectorised callable)."""
    x = np.sort(_flat(x))
    n = x.size
    f = cdf(x)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - f).max(), (f - (i - 1) / n).max()) * math.sqrt(n))


_erf = np.vectorize(math.erf, otypes=[np.float64])


def normal_cdf(x):
    return 0.5 * (1.0 + _erf(np.asarray(x, dtype=np.float64) / math.sqrt(2.0)))


def gumbel_cdf(x):
    return np.exp(-np.exp(-np.asarray(x, dtype=np.float64)))


def uniform_cdf(lo, hi):
    return lambda x: np.clip((np.asarray(x, dtype=np.float64) - lo) / (hi - lo), 0.0, 1.0)


def sum_moments(m, n):
    """Raw moments [0..K] of the sum of n independent copies of a variable with raw moments m[0..K] (binomial convolution)."""
    k_max = len(m) - 1
    out = list(m)
    for _ in range(n - 1):
        out = [sum(math.comb(k, j) * out[j] * m[k - j] for j in range(k + 1)) for k in range(k_max + 1)]
    return out


def uniform_central_moments(half, k_max=8):
    """E x^k of the uniform law on [-half, half)."""
    return [0.0 if k % 2 else half ** k / (k + 1) for k in range(k_max + 1)]


_UNI_NOISE = uniform_central_moments(0.02)                 # the state increment's noise
_UNI_RESET = uniform_central_moments(0.05)                 # a reset component
_SQRT3 = 1.7320508075688772
_REWARD = [mk * _SQRT3 ** k for k, mk in enumerate(sum_moments(uniform_central_moments(0.5), 4))]   # var 1, m4 2.7


def worst(stats, bars=(Z_BAR, KS_BAR)):
    """(name, |value| / bar) of the statistic closest to (or furthest past) its bar; stats = [(name, kind, value)]."""
    fr = [(n, abs(v) / (bars[1] if kind == "ks" else bars[0])) for n, kind, v in stats]
    return max(fr, key=lambda t: t[1])


def failures(stats, bars=(Z_BAR, KS_BAR)):
    return [(n, v) for n, kind, v in stats if not abs(v) <= (bars[1] if kind == "ks" else bars[0])]


# ---------------------------------------------------------------------------------------------------------------- gumbel
# gumbel_noise.h: base = mix64(seed GOLD + step); word(row, a) = base + row * 64 + a; u = ((mix64(word) >> 41) + 0.5) 2^-23 in fp32
# (23 bits: strictly inside (0, 1)); score = logit - log(-log u).
GUMBEL_STRIDE, GUMBEL_CAP = 64, 64


def gumbel_words(seed, step, rows, n_actions, row_stride=GUMBEL_STRIDE):
    """Pre-mix words [len(rows), n_actions] of sampler step `step` for GLOBAL rows `rows`."""
    with np.errstate(over="ignore"):
        base = mix64(u64(seed) * _GOLD + u64(step))
        return base + u64s(rows)[:, None] * np.uint64(row_stride) + np.arange(n_actions, dtype=np.uint64)[None, :]


def gumbel_uniform_of_hash(h, bits=23):
    """The kernel's float32 arithmetic on a hashed word.  bits = 24 is the formula the header's comment records as wrong: k + 0.5
    is not a float32 number for k >= 2^23, the largest k rounds to 2^24 and u == 1."""
    k = (np.asarray(h, dtype=np.uint64) >> np.uint64(64 - bits)).astype(np.float32)
    return ((k + np.float32(0.5)) * np.float32(2.0 ** -bits)).astype(np.float64)


def gumbel_noise_of_u(u):
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(u))


def gumbel_draw(logits, seed, step, lo, row_stride=GUMBEL_STRIDE, bits=23):
    """(action [n], top-two score gap [n], noise [n, A]) of one launch over rows lo .. lo + n, scores in float64."""
    logits = np.asarray(logits, dtype=np.float64)
    n, a = logits.shape
    rows = [int(lo) + i for i in range(n)]
    noise = gumbel_noise_of_u(gumbel_uniform_of_hash(mix64(gumbel_words(seed, step, rows, a, row_stride)), bits))
    score = logits + noise
    if a > 1:
        s = np.sort(score, axis=1)
        with np.errstate(invalid="ignore"):
            gap = s[:, -1] - s[:, -2]
    else:
        gap = np.full(n, np.inf)
    return score.argmax(axis=1).astype(np.int64), gap, noise


def _peaked(a):
    """One logit vector with probabilities spread over three decades (float32 values, as the kernel reads them)."""
    return (2.5 * np.cos(1.7 * np.arange(a) + 0.3) - 0.04 * np.arange(a)).astype(np.float32)


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


# name, A, rows, steps, logits, seed, second seed, first sampler step, lo
_GUMBEL_GRID = (
    (2, 1000, 200, "flat", 20240611, 20240612, 0, 0), (2, 1000, 200, "peaked", 7, 8, 100000, 64),
    (6, 1000, 200, "flat", (1 << 40) + 3, (1 << 40) + 4, 5, 3), (6, 1000, 200, "peaked", 911, 3, 17, 1000),
    (18, 1000, 100, "flat", 31337, 31338, 1 << 20, 0), (18, 1000, 100, "peaked", 5, 6, 0, 7),
    (64, 1000, 100, "flat", 99, 100, 42, 0), (64, 1000, 100, "peaked", 123456789, 1, 9, 129))


def gumbel_cases():
    out = []
    for a, rows, steps, kind, seed, seed2, step0, lo in _GUMBEL_GRID:
        vec = np.zeros(a, dtype=np.float32) if kind == "flat" else _peaked(a)
        out.append(dict(name="a%d_%s" % (a, kind), A=a, rows=rows, steps=steps, seed=seed, seed2=seed2, step0=step0, lo=lo,
                        logit_vec=vec, logits=np.ascontiguousarray(np.broadcast_to(vec, (rows, a)))))
    return out


def gumbel_sample(c, seed=None, noise=False, **variant):
    """The restatement's draws of a case: actions [steps, rows], gaps [steps, rows] (and the noise [steps, rows, A])."""
    seed = c["seed"] if seed is None else seed
    acts, gaps, ns = [], [], []
    for k in range(c["steps"]):
        a, g, nz = gumbel_draw(c["logits"], seed, c["step0"] + k, c["lo"], **variant)
        acts.append(a), gaps.append(g)
        if noise:
            ns.append(nz)
    return (np.stack(acts), np.stack(gaps)) + ((np.stack(ns),) if noise else ())


def gumbel_action_stats(c, actions, actions2):
    """What can be asked of the ACTIONS alone (all a kernel returns): frequencies against the float64 softmax of the logits, and
    independence of the action index along rows, along steps and between two seeds."""
    p = softmax64(c["logit_vec"])
    idx = np.arange(c["A"], dtype=np.float64)
    mu = float((p * idx).sum())
    sd = math.sqrt(float((p * (idx - mu) ** 2).sum()))
    actions = np.asarray(actions)
    assert actions.shape == (c["steps"], c["rows"]) and actions.min() >= 0 and actions.max() < c["A"]
    counts = np.bincount(actions.reshape(-1), minlength=c["A"])
    return [("freq_chi2", "z", chi2_z(counts, p * actions.size)),
            ("lag_row", "z", z_lag(actions, 1, mu, sd)), ("lag_step", "z", z_lag(actions, 0, mu, sd)),
            ("two_seeds", "z", z_corr(actions, actions2, mu, sd, mu, sd))]


def gumbel_noise_stats(noise, noise2):
    """The per-element noise (score minus logit) of the restatement: Gumbel by KS against exp(-exp(-x)); moments; independence
    along action, row, step and between two seeds."""
    sd = math.pi / math.sqrt(6.0)
    with np.errstate(invalid="ignore"):
        finite = bool(np.isfinite(noise).all())
    out = [("noise_finite", "z", 0.0 if finite else np.inf)]
    if not finite:
        return out
    out += [("noise_ks", "ks", ks_stat(noise, gumbel_cdf)), ("noise_mean", "z", z_mean(noise, _EULER, sd * sd)),
            ("noise_lag_row", "z", z_lag(noise, 1, _EULER, sd)), ("noise_lag_step", "z", z_lag(noise, 0, _EULER, sd)),
            ("noise_two_seeds", "z", z_corr(noise, noise2, _EULER, sd, _EULER, sd))]
    if noise.shape[2] > 1:
        out.append(("noise_lag_action", "z", z_lag(noise, 2, _EULER, sd)))
    return out


# The uniform's range.  No sample of 1e5 draws meets the largest 24-bit word (2^-24 per draw), so the range is tested where it is
# reached: GUMBEL_EXTREME is a position of the real stream whose hashed word has its top 24 bits all set (found by a search over
# sampler steps of seed 1, rows 0 .. 1023, 64 actions: tests/test_stream_stats_host.py checks that it still is one).  With the
# 23-bit formula its noise is -log(-log(1 - 2^-24)) = 16.6 and an action 30 below the rest cannot win; with the 24-bit formula
# u == 1, the noise is +inf and it wins whatever the logits.
GUMBEL_EXTREME = dict(seed=1, step=73, row=517, action=14, lo=512, rows=8, A=18)      # hashed word 0xffffffeaa42a0bca
GUMBEL_EXTREME_LOGIT = -30.0


def gumbel_extreme_logits(n_rows, n_actions, action):
    x = np.zeros((n_rows, n_actions), dtype=np.float32)
    x[:, action] = GUMBEL_EXTREME_LOGIT
    return x


GUMBEL_CONTROLS = (       # (name, variant of gumbel_draw, the statistic it must fail)
    ("row_stride_1", dict(row_stride=1), "lag_row"),
    ("uniform_24_bits", dict(bits=24), "noise_finite"))     # at GUMBEL_EXTREME: no sample reaches it


# ----------------------------------------------------------------------------------------------------------------- gauss
# cont_env.h gauss_noise: word = (seed 8 + 6) GOLD + (t n_global + i) 64 + 2 d; u1 = ((mix64(word) >> 40) + 1) 2^-24 in (0, 1],
# u2 = (mix64(word + 1) >> 40) 2^-24 in [0, 1); z = sqrt(-2 log u1) cos(2 pi u2), all in fp32.
GAUSS_STRIDE, GAUSS_CAP, GAUSS_STREAM = 64, 32, 6


def gauss_words(seed, t, n_global, envs, a_dim, d_step=2):
    """Pre-mix words [len(envs), a_dim] of u1 (u2's word is the next one)."""
    with np.errstate(over="ignore"):
        pos = u64(t) * u64(n_global) + u64s(envs)[:, None]
        return (u64(seed) * np.uint64(8) + np.uint64(GAUSS_STREAM)) * _GOLD + pos * np.uint64(GAUSS_STRIDE) + \
            np.uint64(d_step) * np.arange(a_dim, dtype=np.uint64)[None, :]


def gauss_draw(seed, t, n_global, envs, a_dim, d_step=2, one_word=False):
    """float32 standard normals [len(envs), a_dim] of sampler step t for GLOBAL environments `envs`."""
    w = gauss_words(seed, t, n_global, envs, a_dim, d_step)
    with np.errstate(over="ignore"):
        h1 = mix64(w)
        h2 = h1 if one_word else mix64(w + np.uint64(1))
    f = np.float32
    u1 = ((h1 >> np.uint64(40)).astype(np.uint32) + np.uint32(1)).astype(f) * f(5.9604644775390625e-8)
    u2 = (h2 >> np.uint64(40)).astype(f) * f(5.9604644775390625e-8)
    return (np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(6.2831853071795865) * u2)).astype(f)


# name, a_dim, rows, steps, seed, second seed, first step, n_global, env0
_GAUSS_GRID = ((1, 64, 256, 12345, 12346, 0, 64, 0), (6, 64, 256, 12345, 12346, 11, 200, 100),
               (16, 64, 256, 12345, 12346, 0, 64, 0), (32, 64, 256, (1 << 33) + 9, 2, 1 << 16, 64, 0))


def gauss_cases():
    return [dict(name="a%d" % a, A=a, rows=n, steps=t, seed=s, seed2=s2, step0=t0, n_global=ng, env0=e0)
            for a, n, t, s, s2, t0, ng, e0 in _GAUSS_GRID]


def gauss_sample(c, seed=None, **variant):
    seed = c["seed"] if seed is None else seed
    envs = [c["env0"] + i for i in range(c["rows"])]
    return np.stack([gauss_draw(seed, c["step0"] + k, c["n_global"], envs, c["A"], **variant) for k in range(c["steps"])])


def gauss_stats(z, z2):
    """z [steps, rows, A] and the same positions of a second seed: standard normal by moments and KS; independence along
    dimension (the two halves of Box-Muller: linear AND in the squares -- sharing a word between neighbouring dimensions leaves
    the linear correlation at zero because cos(2 pi u) has mean zero), row, step and seed."""
    z, z2 = np.asarray(z, dtype=np.float64), np.asarray(z2, dtype=np.float64)
    sq, sq_sd = z * z, math.sqrt(2.0)
    out = [("mean", "z", z_mean(z, 0.0, 1.0)), ("var", "z", z_moment(z, 0.0, 2, 1.0, 3.0)),
           ("m4", "z", z_moment(z, 0.0, 4, 3.0, 105.0)), ("ks", "ks", ks_stat(z, normal_cdf)),
           ("lag_row", "z", z_lag(z, 1, 0.0, 1.0)), ("lag_step", "z", z_lag(z, 0, 0.0, 1.0)),
           ("sq_lag_row", "z", z_lag(sq, 1, 1.0, sq_sd)), ("sq_lag_step", "z", z_lag(sq, 0, 1.0, sq_sd)),
           ("two_seeds", "z", z_corr(z, z2, 0.0, 1.0, 0.0, 1.0))]
    if z.shape[2] > 1:
        out += [("lag_dim", "z", z_lag(z, 2, 0.0, 1.0)), ("sq_lag_dim", "z", z_lag(sq, 2, 1.0, sq_sd))]
    return out


GAUSS_CONTROLS = (("one_word", dict(one_word=True), "ks"), ("d_step_1", dict(d_step=1), "sq_lag_dim"))


# ------------------------------------------------------------------------------------------------ continuous environment
# cont_env.h: hash(seed, stream, c, j) = mix64((seed 8 + stream + 1) GOLD + c 64 + j); U = (hash >> 11) 2^-53.
#   step: c += 1; m = mean of the clipped fp32 actions, summed left to right in fp64; s_j = (s_j + 0.01 m) + (-0.02 + 0.04 U(0, c, j))
#   reward = (((U(1,c,0) + U(1,c,1)) + (U(1,c,2) + U(1,c,3))) - 2) sqrt(3);  done = hash(2, c, 0) mod horizon == 0
#   done -> s_j = -0.05 + 0.1 U(3, c, j)       (also cartpole_env.h's and pendulum_env.h's reset)
CENV_STRIDE, CENV_CAP, CENV_STREAMS = 64, 64, 4


def cenv_words(seeds, stream, c, j, with_stream=True):
    """Pre-mix words, broadcast over seeds / counters / components (uint64 arrays or python integers)."""
    as_u = lambda x: x if isinstance(x, np.ndarray) and x.dtype == np.uint64 else u64s(x).reshape(np.shape(x))
    with np.errstate(over="ignore"):
        key = as_u(seeds) * np.uint64(8) + np.uint64(stream + 1 if with_stream else 1)
        return key * _GOLD + as_u(c) * np.uint64(CENV_STRIDE) + as_u(j)


def cenv_hash(seeds, stream, c, j, with_stream=True):
    return mix64(cenv_words(seeds, stream, c, j, with_stream))


def cenv_u(seeds, stream, c, j, with_stream=True):
    return (cenv_hash(seeds, stream, c, j, with_stream) >> np.uint64(11)).astype(np.float64) * 1.1102230246251565e-16


def cenv_reset(seeds, c, s_dim, with_stream=True):
    """Reset states [n, s_dim] of environments `seeds` [n] at counters c [n]."""
    seeds, c = u64s(seeds), u64s(c)
    return -0.05 + 0.1 * cenv_u(seeds[:, None], 3, c[:, None], np.arange(s_dim, dtype=np.uint64)[None, :], with_stream)


def cenv_mean_action(action):
    """[..., A] float32 actions -> the fp64 mean of their clipped values, summed left to right."""
    a = np.clip(np.asarray(action, dtype=np.float32), np.float32(-1.0), np.float32(1.0)).astype(np.float64)
    return np.cumsum(a, axis=-1)[..., -1] / float(a.shape[-1])


def cenv_rollout(seeds, s_dim, actions, horizon, c0=0, state0=None, with_stream=True, reward_terms=4):
    """T steps of n environments from counters c0 (int or [n]) and states state0 (default: the reset at c0).
    -> dict(states [T + 1, n, S] fp64, reward [T, n], done [T, n] bool, mean_a [T, n], counters [n] python integers)."""
    seeds = u64s(seeds)
    n, t_len = seeds.size, actions.shape[0]
    c_start = [int(c0)] * n if np.ndim(c0) == 0 else [int(x) for x in c0]
    s = cenv_reset(seeds, c_start, s_dim, with_stream) if state0 is None else np.array(state0, dtype=np.float64)
    mean_a = cenv_mean_action(actions)
    with np.errstate(over="ignore"):        # counters of every (step, environment), advanced before the step's draws
        c = (u64s(c_start)[None, :] + np.arange(1, t_len + 1, dtype=np.uint64)[:, None])[:, :, None]
    sd, j = seeds[None, :, None], np.arange(s_dim, dtype=np.uint64)[None, None, :]
    step_noise = -0.02 + 0.04 * cenv_u(sd, 0, c, j, with_stream)
    resets = -0.05 + 0.1 * cenv_u(sd, 3, c, j, with_stream)
    ur = cenv_u(sd, 1, c, np.arange(4, dtype=np.uint64)[None, None, :], with_stream)
    if reward_terms == 3:       # negative control: the fourth uniform replaced by its mean
        ur[:, :, 3] = 0.5
    reward = (((ur[:, :, 0] + ur[:, :, 1]) + (ur[:, :, 2] + ur[:, :, 3])) - 2.0) * _SQRT3
    done = (cenv_hash(sd, 2, c, np.uint64(0), with_stream)[:, :, 0] % np.uint64(horizon)) == 0
    states = np.empty((t_len + 1, n, s_dim), dtype=np.float64)
    states[0] = s
    for t in range(t_len):
        s = np.where(done[t][:, None], resets[t], (s + 0.01 * mean_a[t][:, None]) + step_noise[t])
        states[t + 1] = s
    return dict(states=states, reward=reward, done=done, mean_a=mean_a, counters=[x + t_len for x in c_start])


# name, s_dim, horizon, first seed (64 environments with consecutive seeds), steps, a_dim
_CENV_GRID = ((1, 7, 40, 2048, 3), (17, 7, 1 << 20, 2048, 6), (64, 7, 77, 2048, 2),
              (1, 1000, 3, 2048, 6), (17, 1000, 40, 2048, 3), (64, 1000, (1 << 35) + 1, 2048, 1))
CENV_ENVS = 64


def cenv_cases():
    return [dict(name="s%d_h%d" % (s, h), S=s, horizon=h, seeds=[sd + i for i in range(CENV_ENVS)], steps=t, A=a)
            for s, h, sd, t, a in _CENV_GRID]


def cenv_actions(c):
    """[steps, n, A] float32, a fifth of them outside [-1, 1] (the clip is part of the drift)."""
    rs = np.random.RandomState(c["S"] * 1000 + c["horizon"])
    return (rs.standard_normal((c["steps"], len(c["seeds"]), c["A"])) * 0.8).astype(np.float32)


def cenv_stats(c, states, reward, done, mean_a):
    """The laws of one trajectory (states [T + 1, n, S], reward [T, n], done [T, n], mean_a [T, n]):
    increment minus drift uniform on [-0.02, 0.02); reward mean 0, variance 1, fourth moment of a four-uniform sum; terminal rate
    1 / horizon; resets uniform on [-0.05, 0.05); streams 0 (noise), 1 (reward) and 3 (reset) uncorrelated at equal (seed, counter);
    neighbouring seeds uncorrelated; no lag correlation along step or component."""
    states, reward, done = np.asarray(states, dtype=np.float64), np.asarray(reward, dtype=np.float64), np.asarray(done).astype(bool)
    t_len, n = reward.shape
    h = c["horizon"]
    p_done = float(((1 << 64) + h - 1) // h) / 2.0 ** 64          # multiples of the horizon among 2^64 words
    noise_all = states[1:] - (states[:-1] + 0.01 * np.asarray(mean_a, dtype=np.float64)[:, :, None])
    live = ~done
    noise, reset = noise_all[live], states[1:][done]                # [k, S] each
    m, r, rm = _UNI_NOISE, _UNI_RESET, _REWARD
    sd_n, sd_r = math.sqrt(m[2]), math.sqrt(r[2])
    out = [("noise_ks", "ks", ks_stat(noise, uniform_cdf(-0.02, 0.02))), ("noise_mean", "z", z_mean(noise, 0.0, m[2])),
           ("noise_var", "z", z_moment(noise, 0.0, 2, m[2], m[4])), ("noise_m4", "z", z_moment(noise, 0.0, 4, m[4], m[8])),
           ("reward_mean", "z", z_mean(reward, 0.0, 1.0)), ("reward_var", "z", z_moment(reward, 0.0, 2, rm[2], rm[4])),
           ("reward_m4", "z", z_moment(reward, 0.0, 4, rm[4], rm[8])),
           ("done_rate", "z", z_rate(int(done.sum()), done.size, p_done)),
           ("reward_lag_step", "z", z_lag(reward, 0, 0.0, 1.0)), ("reward_lag_env", "z", z_lag(reward, 1, 0.0, 1.0))]
    # pairs of consecutive live steps / neighbouring live environments of the noise
    both_t, both_e = live[:-1] & live[1:], live[:, :-1] & live[:, 1:]
    out += [("noise_lag_step", "z", z_corr(noise_all[:-1][both_t], noise_all[1:][both_t], 0.0, sd_n, 0.0, sd_n)),
            ("noise_lag_env", "z", z_corr(noise_all[:, :-1][both_e], noise_all[:, 1:][both_e], 0.0, sd_n, 0.0, sd_n))]
    k4 = min(4, c["S"])
    out.append(("noise_vs_reward", "z", z_corr(noise_all[:, :, :k4].sum(axis=2)[live], reward[live], 0.0, sd_n * math.sqrt(k4), 0.0, 1.0)))
    if c["S"] > 1:
        out.append(("noise_lag_comp", "z", z_lag(noise, 1, 0.0, sd_n)))
    if h > 1:
        out.append(("done_lag_step", "z", z_lag(done, 0, p_done, math.sqrt(p_done * (1 - p_done)))))
        out.append(("done_vs_reward", "z", z_corr(done, reward, p_done, math.sqrt(p_done * (1 - p_done)), 0.0, 1.0)))
    if reset.size:
        out += [("reset_ks", "ks", ks_stat(reset, uniform_cdf(-0.05, 0.05))), ("reset_mean", "z", z_mean(reset, 0.0, r[2])),
                ("reset_vs_reward", "z", z_corr(reset[:, :k4].sum(axis=1), reward[done], 0.0, sd_r * math.sqrt(k4), 0.0, 1.0))]
        if reset.size >= 64 * MIN_EXPECTED:
            cells = np.clip(((reset.reshape(-1) + 0.05) * 320.0).astype(np.int64), 0, 31)
            out.append(("reset_chi2", "z", chi2_z(np.bincount(cells, minlength=32), np.full(32, reset.size / 32.0))))
        if c["S"] > 1:
            out.append(("reset_lag_comp", "z", z_lag(reset, 1, 0.0, sd_r)))
    return out


def cenv_stream_stats(seeds, counters, with_stream=True):
    """Streams 0 .. 3 at equal (seed, counter, component 0): the six pairwise correlations of their uniforms (restatement only:
    a kernel shows stream 3 only where stream 2 says done)."""
    u = [cenv_u(u64s(seeds)[:, None], s, u64s(counters)[None, :], np.uint64(0), with_stream) for s in range(CENV_STREAMS)]
    sd = math.sqrt(1.0 / 12.0)
    return [("streams_%d_%d" % (a, b), "z", z_corr(u[a], u[b], 0.5, sd, 0.5, sd)) for a in range(4) for b in range(a + 1, 4)]


CENV_CONTROLS = (("no_stream_term", dict(with_stream=False), "noise_vs_reward"), ("reward_3_uniforms", dict(reward_terms=3), "reward_var"))

# cart-pole resets (cartpole_env.h): with horizon 1 every step ends its episode, and the state after step k of an environment that
# started at counter c0 is the reset at counter c0 + k
CARTPOLE_CASE = dict(name="cartpole_h1", S=4, seeds=[50 + i for i in range(64)], steps=1024)


def cartpole_resets(seeds, c0, steps):
    """[steps, n, 4]: the states dra_cartpole_step leaves at horizon 1."""
    return np.stack([cenv_reset(seeds, [int(c0) + k + 1] * len(seeds), 4) for k in range(steps)])


def reset_stats(x):
    """x [steps, n, S] reset states: uniform on [-0.05, 0.05) by KS, chi-square and moments; independent along every index."""
    r, sd = _UNI_RESET, math.sqrt(_UNI_RESET[2])
    x = np.asarray(x, dtype=np.float64)
    cells = np.clip(((x.reshape(-1) + 0.05) * 640.0).astype(np.int64), 0, 63)
    return [("ks", "ks", ks_stat(x, uniform_cdf(-0.05, 0.05))), ("chi2", "z", chi2_z(np.bincount(cells, minlength=64), np.full(64, x.size / 64.0))),
            ("mean", "z", z_mean(x, 0.0, r[2])), ("var", "z", z_moment(x, 0.0, 2, r[2], r[4])), ("m4", "z", z_moment(x, 0.0, 4, r[4], r[8])),
            ("lag_step", "z", z_lag(x, 0, 0.0, sd)), ("lag_env", "z", z_lag(x, 1, 0.0, sd)), ("lag_comp", "z", z_lag(x, 2, 0.0, sd))]


# ------------------------------------------------------------------------------------------------------- synthetic Atari
# actor_env.h / ring.hip: frame word w of frame `counter` = mix64(seed GOLD + counter words + w) (882 words of 8 bytes for 84 x 84);
# reward from (mix64((seed + 1) GOLD + counter) >> 32) mod 10: 0 -> -1, 9 -> +1, else 0; terminal: mix64((seed + 2) GOLD + counter)
# mod done_period == 0 (mask = 1 - terminal).
ATARI_WORDS = 882


def atari_frame_words(seed, counters, n_words=ATARI_WORDS, frame_words=ATARI_WORDS):
    """Pre-mix words [len(counters), n_words]; frame_words is the stride (the frame's size in words)."""
    with np.errstate(over="ignore"):
        return u64(seed) * _GOLD + u64s(counters)[:, None] * np.uint64(frame_words) + np.arange(n_words, dtype=np.uint64)[None, :]


def atari_reward_words(seeds, counters):
    with np.errstate(over="ignore"):
        return (u64s(seeds)[:, None] + np.uint64(1)) * _GOLD + u64s(counters)[None, :]


def atari_mask_words(seeds, counters):
    with np.errstate(over="ignore"):
        return (u64s(seeds)[:, None] + np.uint64(2)) * _GOLD + u64s(counters)[None, :]


def atari_frames(seed, counters, frame_bytes=7056):
    w = frame_bytes // 8
    return mix64(atari_frame_words(seed, counters, w, w)).astype("<u8").view(np.uint8).reshape(len(counters), frame_bytes)


def atari_reward_done(seeds, counters, done_period):
    """(reward f64 [n_seeds, n_counters], done bool [n_seeds, n_counters])."""
    u = (mix64(atari_reward_words(seeds, counters)) >> np.uint64(32)) % np.uint64(10)
    done = (mix64(atari_mask_words(seeds, counters)) % np.uint64(done_period)) == 0
    return np.where(u == 0, -1.0, np.where(u == 9, 1.0, 0.0)), done


ATARI_CASES = tuple(dict(name="period%d" % p, done_period=p, seeds=[s + i for i in range(8)], counter0=c0, count=32768)
                    for p, s, c0 in ((3, 11, 0), (37, 1, 5), (800, (1 << 32) + 1000, 1 << 20)))
ATARI_FRAME_CASE = dict(name="frames", seed=11, counter0=3, count=256, frame_bytes=7056)


def atari_stats(c, reward, done):
    """reward / done [n_seeds, count] of environments with consecutive seeds: p = 0.1 / 0.8 / 0.1, terminal rate 1 / period,
    independence along the counter and across neighbouring seeds, and the cross statistic of the recorded overlap."""
    reward, done = np.asarray(reward, dtype=np.float64), np.asarray(done).astype(bool)
    p = c["done_period"]
    pd = float(((1 << 64) + p - 1) // p) / 2.0 ** 64
    sd_d, sd_r = math.sqrt(pd * (1 - pd)), math.sqrt(0.2)
    ab, sd_ab = np.abs(reward), math.sqrt(0.2 * 0.8)
    counts = np.asarray([(reward == v).sum() for v in (-1.0, 0.0, 1.0)])
    assert counts.sum() == reward.size
    return [("reward_chi2", "z", chi2_z(counts, np.asarray([0.1, 0.8, 0.1]) * reward.size)),
            ("done_rate", "z", z_rate(int(done.sum()), done.size, pd)),
            ("reward_lag_counter", "z", z_lag(reward, 1, 0.0, sd_r)), ("done_lag_counter", "z", z_lag(done, 1, pd, sd_d)),
            ("reward_lag_seed", "z", z_lag(reward, 0, 0.0, sd_r)), ("done_lag_seed", "z", z_lag(done, 0, pd, sd_d)),
            ("done_vs_own_reward", "z", z_corr(done, reward, pd, sd_d, 0.0, sd_r)),
            ("done_vs_next_seed_reward", "z", z_corr(done[:-1], reward[1:], pd, sd_d, 0.0, sd_r)),
            ("done_vs_next_seed_abs_reward", "z", z_corr(done[:-1], ab[1:], pd, sd_d, 0.2, sd_ab))]


def frame_stats(frames):
    """uint8 [count, frame_bytes]: the byte histogram, and neighbouring bytes / neighbouring frames uncorrelated."""
    f = np.asarray(frames)
    mu, sd = 127.5, math.sqrt((256.0 ** 2 - 1.0) / 12.0)
    return [("byte_chi2", "z", chi2_z(np.bincount(f.reshape(-1), minlength=256), np.full(256, f.size / 256.0))),
            ("byte_mean", "z", z_mean(f, mu, sd * sd)), ("lag_byte", "z", z_lag(f, 1, mu, sd)), ("lag_frame", "z", z_lag(f, 0, mu, sd))]


# --------------------------------------------------------------------------------------------------------- stride and cap
def collisions(words):
    """Number of repeated values among pre-mix words (mix64 is a bijection: equal words are the only way to equal draws)."""
    w = np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in words])
    return int(w.size - np.unique(w).size)


def gumbel_position_words(seed, step, n_rows, n_actions):
    return [gumbel_words(seed, step, list(range(n_rows)), n_actions)]


def gauss_position_words(seed, t, n_rows, a_dim):
    w = gauss_words(seed, t, n_rows, list(range(n_rows)), a_dim)
    return [w, w + np.uint64(1)]


def cenv_position_words(seed, n_counters, s_dim, t=0, n_rows=8):
    """The four environment streams over counters 0 .. n_counters and s_dim components, plus the noise stream of the same seed."""
    c = np.arange(n_counters, dtype=np.uint64)[:, None]
    j = np.arange(s_dim, dtype=np.uint64)[None, :]
    return [cenv_words(u64(seed), s, c, j) for s in range(CENV_STREAMS)] + gauss_position_words(seed, t, n_rows, GAUSS_CAP)


def atari_position_words(seed, n_counters, n_words):
    c = list(range(n_counters))
    return [atari_frame_words(seed, c, n_words), atari_reward_words([seed], c), atari_mask_words([seed], c)]


# ----------------------------------------------------------------------------------------------------------- far counters
FAR_POINTS = (1 << 31, 1 << 32, 1 << 40)       # three steps across each: P - 1, P, P + 1
FAR_SEEDS = ((1 << 31) - 1, (1 << 32) + 5, (1 << 63) + 7, -3)   # the last read as uint64 by every kernel


def as_i64(x):
    """The int64 a uint64 seed travels as in a device array of seeds."""
    x = int(x) & M64
    return x - (1 << 64) if x >> 63 else x


def far_logits(n, a, key):
    return (np.random.RandomState(key).standard_normal((n, a)) * 2).astype(np.float32)


# rows x actions of the far-counter gumbel launches, and (step, lo, seed) of each: one input far, the others small
FAR_GUMBEL_SHAPE = (65, 6)
FAR_GUMBEL = tuple([(p - 1, 3, 77) for p in FAR_POINTS] + [(5, p - 33, 77) for p in FAR_POINTS] + [(9, 4, s) for s in FAR_SEEDS])
# (step, n_global, env0, seed) of the far-counter gauss launches over 33 rows x 5 dims
FAR_GAUSS_SHAPE = (33, 5)
FAR_GAUSS = tuple([(p - 1, 40, 2, 77) for p in FAR_POINTS] + [(2, p - 1, 3, 77) for p in FAR_POINTS] +
                  [(2, p + 100, p - 17, 77) for p in FAR_POINTS] + [(4, 64, 1, s) for s in FAR_SEEDS])
# first counter of the environments' far launches (three steps each) and of fill_synthetic (4 transitions each)
FAR_COUNTERS = tuple(p - 2 for p in FAR_POINTS)

