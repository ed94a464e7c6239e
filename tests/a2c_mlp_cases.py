"""The rollout cases of tests/test_gpu_a2c_continuous.py and their fp64 restatement (tests/a2c_mlp_restatement.py), computed
once per case and shared: the CPU suite checks what the cases cover (terminals inside the short-horizon case), the GPU suite
compares dra_a2c_mlp_rollout with them."""
import functools

import numpy as np

import a2c_mlp_restatement as R
from oracle.numerics_oracle import RunningMeanStdOracle

# (n_env, t_len, state_dim, action_dim, hidden, gate, normaliser, horizon): one environment and one step; an odd everything with
# tanh, updated statistics and a horizon short enough for several episodes to end inside 7 steps; the a2c_continuous shape; the
# largest environment count (8 row blocks per thread group) with read-only statistics
ROLLOUT_CASES = ((1, 1, 17, 6, 64, "relu", "identity", 4),
                 (5, 7, 5, 2, 32, "tanh", "meanstd-update", 3),
                 (16, 5, 17, 6, 64, "relu", "identity", 4),
                 (64, 3, 17, 6, 64, "relu", "meanstd-readonly", 4))
WARM_ROWS = 40              # rows the mean / std normaliser has seen before the rollout starts
NOISE_SEED, SAMPLER0, ENV_SEED0 = 4, 3, 70
ENV0_EXTRA = 2              # the rollout's environments are GLOBAL environments 2 .. 2 + n of n + 3 (the noise stream's indexing)


def _setup(case):
    n, t_len, s_dim, a_dim, hidden, gate, kind, horizon = case
    params = R.init_params(s_dim, a_dim, hidden, seed=12 + n)
    envs = [R.ContinuousEnvOracle(ENV_SEED0 + i, s_dim, a_dim, horizon) for i in range(n)]
    raw = np.stack([e.reset() for e in envs])
    norm = None
    rms0 = np.concatenate([np.zeros(s_dim), np.ones(s_dim), [0.0]])
    if kind != "identity":
        norm = R.MeanStdNormalizerOracle()
        norm.rms = RunningMeanStdOracle(shape=(1, s_dim))
        norm(np.random.RandomState(5).randn(WARM_ROWS, s_dim) * 0.05 + 0.01)
        norm.read_only = kind == "meanstd-readonly"
        rms0 = np.concatenate([norm.rms.mean.reshape(-1), norm.rms.var.reshape(-1), [norm.rms.count]])
    return params, envs, raw, norm, rms0


@functools.lru_cache(maxsize=None)
def _restated(case):
    n, t_len, s_dim, a_dim, hidden, gate, kind, horizon = case
    params, envs, raw, norm, rms0 = _setup(case)
    start = dict(params=params, raw=raw.copy(), rms=rms0.copy(), seeds=[e.seed for e in envs])
    want = R.rollout(params, envs, raw, norm, t_len, NOISE_SEED, SAMPLER0, gate=gate, n_global=n + ENV0_EXTRA + 1, env0=ENV0_EXTRA)
    return want, envs, norm, start


def restated_rollout(case):
    """(the restatement's rollout, its environments and normaliser AFTER the rollout, what the rollout started from).  Computed
    once per case; callers leave it unchanged."""
    return _restated(tuple(case))
