"""Edge-shape cases, float64 references and bars for csrc/a2c_mlp.hip: the one-launch Gaussian rollout (dra_a2c_mlp_rollout) and the
Gaussian head kernels (dra_gauss_head_fwd / _bwd).  NOT a test file: CPU only, no product code imported.
tests/test_a2c_mlp_edge_cases_host.py proves on the CPU that every case reaches the path it is named for and that its inputs carry
the bars; tests/test_gpu_a2c_mlp_edges.py holds the kernels to it.

References
  rollout  a2c_mlp_restatement.rollout in float64 over the oracle's environments, normaliser and hashed noise.  Every case runs with
           reward_coef 0.1 and environment i stepped i % 3 times (zero actions) before the start is recorded, so that the step
           counters differ from one environment to the next.
  head     a2c_mlp_restatement.head / head_grads in float64 on head_case(n, a_dim).

Bars (those of tests/test_gpu_a2c_continuous.py, not tuned to the kernels)
  rollout  state, action, v, cur_state: 1e-5 x max(max |want|, 1)
  raw      the raw environment state after the rollout: rtol 1e-6 / atol 1e-8
  stats    updated observation statistics: rtol 1e-7 (mean: atol 1e-9 besides); the count exact
  head     mean, log_pi_a, entropy, dz, dstd: 1e-5 x max(max |want|, 1)
  exact    rewards, masks, counters, sampler position
BAR_OVERRIDES is where a tensor whose INPUTS cannot carry its bar would get a wider one, with the float32 CPU run's figure beside
it.  It is empty: every case's float32 CPU run of the same reference stays within 0.3 x every bar."""
import functools

import numpy as np
import torch

import a2c_mlp_restatement as R

# (case id, group) -> (bar as a multiple of the group's bar, float32-CPU-run error as a multiple of the group's bar)
BAR_OVERRIDES = {}
BAR_GROUPS = ("rollout", "raw", "stats", "head")
HOST_FRACTION = 0.3          # the float32 CPU run of the reference must stay within this fraction of every bar

K_MAX_S, K_MAX_A, K_MAX_N, K_RB = 64, 16, 64, 8          # kMaxS, kMaxA, kMaxN, kRB of csrc/a2c_mlp.hip
K_HEAD_MAX_A = 64                                        # kHeadMaxA
LDS_BYTES_MAX = 160 * 1024
GATE_CODES = {"relu": 1, "tanh": 2}                      # ops.ACT

WARM_ROWS = 40              # rows the mean / std normaliser has seen before the rollout starts
NOISE_SEED, SAMPLER0, ENV_SEED0 = 4, 3, 70
ENV0_EXTRA = 2              # the rollout's environments are GLOBAL environments 2 .. 2 + n of n + 3 (the noise stream's indexing)
REWARD_COEF = 0.1
PRE_STEP_PERIOD = 3         # environment i starts with its counter at i % 3

# (n_env, t_len, state_dim, action_dim, hidden, gate, normaliser, horizon, rms_clip) and the path each is named for
ROLLOUT_CASES = (
    # corner of the supported range (158 692 B of LDS); <64, tanh>; power-of-two fold; all 64 feature lanes fold
    (64, 2, 64, 16, 64, "tanh", "meanstd-update", 2, 10.0),
    # <32, relu>; five row blocks over four row groups, the last block one row live; A = 1; the clip reached
    (33, 3, 3, 1, 32, "relu", "meanstd-readonly", 2, 0.5),
    # S = 1; horizon 1 (every mask 0); two row blocks, the second one row live
    (9, 2, 1, 16, 64, "tanh", "identity", 1, float("inf")),
    # N one short of the maximum and no power of two (the fold's division path); T = 1; the clip on a just-updated statistic
    (63, 1, 64, 1, 32, "tanh", "meanstd-update", 5, 0.5),
    # one environment (batch variance 0 in every fold); T N A = 640 > 256 in the noise loop; 41 folds
    (1, 40, 2, 16, 32, "relu", "meanstd-update", 3, 10.0),
    # odd N, three row blocks; S and A at their maxima with H = 32; clip 1.0
    (17, 6, 64, 16, 32, "relu", "meanstd-update", 3, 1.0),
)
HEAD_CASES = ((257, 3), (320, 6), (1000, 64), (300, 1))     # (n, a_dim): a second workgroup forward, a second trip backward


def case_id(c):
    return "n%d_t%d_s%d_a%d_h%d_%s_%s_hz%d_clip%g" % tuple(c)


# ------------------------------------------------------------------------------------------------ shapes
def round_up8(n):
    return (n + 7) & ~7


def rollout_lds_floats(S, A, H, N):
    """rollout_lds_floats of csrc/a2c_mlp.hip."""
    NP = round_up8(N)
    return 2 * (3 * S + 2) + 2 * S * H + 2 * H * H + 4 * H + A * (H + 1) + H + (A + 1) + A + S * NP + 4 * H * NP + N * A


def rollout_lds_bytes(S, A, H, N):
    """What launch_rollout asks dra_grant_lds for."""
    return (rollout_lds_floats(S, A, H, N) + 4) * 4


def supported(S, A, H, N, gate):
    """dra_a2c_mlp_supported's conditions."""
    return 1 <= S <= K_MAX_S and 1 <= A <= K_MAX_A and H in (32, 64) and 1 <= N <= K_MAX_N and gate in (1, 2) and \
        rollout_lds_bytes(S, A, H, N) <= LDS_BYTES_MAX


def rollout_shape(c):
    """What the launcher and the kernel derive from a case's sizes."""
    n, t_len, S, A, H, gate, kind, horizon, clip = c
    blocks, groups = round_up8(n) // K_RB, 128 // H
    return dict(N=n, T=t_len, S=S, A=A, H=H, gate=gate, kind=kind, horizon=horizon, clip=clip, instantiation=(H, gate),
                blocks=blocks, groups=groups, passes=(blocks + groups - 1) // groups, live_last=n - (blocks - 1) * K_RB,
                pow2=n & (n - 1) == 0, folds=(t_len + 1) if kind == "meanstd-update" else 0, noise=t_len * n * A,
                lds=rollout_lds_bytes(S, A, H, n))


# ------------------------------------------------------------------------------------------------ rollout reference
def run_rollout(case, dtype=torch.float64):
    """The restatement's rollout of a case with both forwards in `dtype` -> (want, environments and normaliser AFTER the rollout,
    what the rollout started from: params, raw, rms, seeds, counters)."""
    n, t_len, S, A, H, gate, kind, horizon, clip = case
    params = R.init_params(S, A, H, seed=12 + n)
    envs, raw = R.start_envs([ENV_SEED0 + i for i in range(n)], S, A, horizon, pre_steps=[i % PRE_STEP_PERIOD for i in range(n)])
    norm, rms0 = R.warm_normalizer(kind, S, WARM_ROWS, clip=clip)
    start = dict(params=params, raw=raw.copy(), rms=rms0.copy(), seeds=[e.seed for e in envs], counters=[e.c for e in envs])
    want = R.rollout(params, envs, raw, norm, t_len, NOISE_SEED, SAMPLER0, gate=gate, n_global=n + ENV0_EXTRA + 1, env0=ENV0_EXTRA,
                     reward_coef=REWARD_COEF, dtype=dtype)
    return want, envs, norm, start


@functools.lru_cache(maxsize=None)
def _reference(case):
    return run_rollout(case)


def rollout_reference(case):
    """The float64 reference of a rollout case, computed once and shared.  Do not modify."""
    return _reference(tuple(case))


def final_stats(norm, start):
    """The statistics [2 S + 1] the kernel must leave behind."""
    if norm is None:
        return start["rms"]
    return np.concatenate([norm.rms.mean.reshape(-1), norm.rms.var.reshape(-1), [norm.rms.count]])


def clip_census(case):
    """(elements equal to +clip, elements equal to -clip) over every normalised observation of the float64 reference, the
    bootstrap observation included."""
    want = rollout_reference(case)[0]
    x = np.concatenate([want["state"].reshape(-1), want["cur_state"].reshape(-1)])
    clip = np.float32(case[8])
    return int((x == clip).sum()), int((x == -clip).sum())


# ------------------------------------------------------------------------------------------------ head cases
STD_VALUES = (-8.0, 0.0, 3.0, 19.9, 20.1, 30.0)       # both sides of softplus's threshold; scale from 3e-4 to 30


def head_case(n, a):
    rs = np.random.RandomState(100 * n + a)
    std = np.asarray([STD_VALUES[(i + n) % len(STD_VALUES)] for i in range(a)], dtype=np.float32)
    z = rs.randn(n, a) * 1.5
    sat = rs.rand(n, a) < 0.4                           # means near +-1: the tanh saturates
    z = np.where(sat, np.sign(z) * rs.uniform(3.0, 9.0, size=(n, a)), z).astype(np.float32)
    scale = R.softplus(torch.tensor(std, dtype=torch.float64)).numpy()
    k = rs.uniform(-6.0, 6.0, size=(n, a))
    k.flat[0], k.flat[-1] = 6.0, -6.0                   # up to 6 sigma from the mean
    action = (np.tanh(z.astype(np.float64)) + k * scale).astype(np.float32)
    g_lp, g_ent = rs.randn(n, 1).astype(np.float32), rs.randn(n, 1).astype(np.float32)
    return z, std, action, g_lp, g_ent


@functools.lru_cache(maxsize=None)
def head_reference(n, a):
    """The float64 restatement of a head case: dict(mean, log_pi_a, entropy, dz, dstd).  Computed once; do not modify."""
    z, std, action, g_lp, g_ent = head_case(n, a)
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)
    mean, lp, ent = R.head(t64(z), t64(std), t64(action))
    dz, dstd = R.head_grads(z, std, action, g_lp, g_ent)
    return dict(mean=mean.numpy(), log_pi_a=lp.numpy(), entropy=ent.numpy(), dz=dz, dstd=dstd)


# ------------------------------------------------------------------------------------------------ bars
def fraction(kind, got, want):
    """The error of `got` against `want` as a multiple of the bar of its kind (<= 1 passes)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float("inf")
    if not got.size:
        return 0.0
    err = np.abs(got - want)
    if kind in ("rollout", "head"):
        return float(err.max()) / (1e-5 * max(float(np.abs(want).max()), 1.0))
    rtol, atol = dict(raw=(1e-6, 1e-8), rms_mean=(1e-7, 1e-9), rms_var=(1e-7, 0.0))[kind]
    tol = atol + rtol * np.abs(want)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0.0, tol, np.finfo(np.float64).tiny))))


def bar(case, group):
    """1, or the entry of BAR_OVERRIDES: the multiple of the group's bar a case's measured fraction may reach."""
    assert group in BAR_GROUPS, group
    return BAR_OVERRIDES.get((case, group), (1.0, 0.0))[0]


ROLLOUT_KEYS = ("state", "action", "v", "cur_state")


def compare_rollout(got, want):
    """{key: fraction of the rollout bar} for the four float32 outputs."""
    return {k: fraction("rollout", got[k], want[k]) for k in ROLLOUT_KEYS}


def compare_stats(got, want, S):
    """(fraction of the mean's bar, fraction of the variance's bar, the counts are equal) for statistics [2 S + 1]."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return fraction("rms_mean", got[:S], want[:S]), fraction("rms_var", got[S:2 * S], want[S:2 * S]), bool(got[2 * S] == want[2 * S])
