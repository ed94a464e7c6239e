"""The case tables of tests/test_a2c_feature_host.py and tests/test_gpu_a2c_feature.py and their restatement
(tests/a2c_feature_restatement.py), computed once per case and shared: the CPU suite checks what the cases cover (terminals,
ring rows, the Gumbel margins the GPU action comparisons rest on), the GPU suite compares dra_cat_mlp_rollout and A2CAgent's
device path with them."""
import copy
import functools

import numpy as np
import torch

import a2c_feature_restatement as R

# (hidden, gate, n_env, t_len, horizon, padded parameter buffer, parameter seed): the a2c_feature shape; one environment and one
# step; the smallest width with relu, an odd environment count (three row blocks, the last one partial), more steps than a
# wave has lanes and a horizon that ends every episode every third step; the middle width at the largest environment count
# (every lane of the environment wave, 8 row blocks) with a horizon of 2; the largest everything with the parameters behind a
# leading gap and NaN padding between them
ROLLOUT_CASES = ((64, "tanh", 5, 5, 200, False, 31),
                 (64, "tanh", 1, 1, 200, False, 32),
                 (16, "relu", 17, 33, 3, False, 33),
                 (32, "tanh", 64, 3, 2, False, 34),
                 (64, "relu", 64, 5, 200, True, 35))
NOISE_SEED, SAMPLER0, ENV_SEED0 = 4, 3, 70
ENV0_EXTRA = 2              # the rollout's environments are GLOBAL environments 2 .. 2 + n of n + 3 (the noise stream's indexing)
RING_CAP, RING_COUNT0 = 64, 61      # the test's ring is short and starts near its end: the appended rows wrap
MARGIN = 1e-4               # the smallest gap between the two Gumbel-perturbed logits the action comparisons tolerate

# the closed-loop test: three seeds, the statistic and where its bar comes from (tests/golden/a2c_feature/)
LEARN_SEEDS = (1, 2, 3)
LAST_EPISODES = 100

# A2CAgent, device path against host-stepped path: 4 environments, rollouts of 5, episodes of at most 7 steps, 6 agent steps
AGENT = dict(n_env=4, t_len=5, horizon=7, steps=6, hidden=64, gate="tanh", param_seed=41, task_seed=3, noise_seed=11,
             discount=0.99, gae_tau=0.95, entropy_weight=0.01, value_loss_weight=1.0, gradient_clip=0.5, lr=0.001)


def case_id(c):
    return "h%d_%s_n%d_t%d_hz%d%s" % (c[0], c[1], c[2], c[3], c[4], "_padded" if c[5] else "")


def make_envs(n, seed0, horizon):
    from deeprl_amd.envs import CartPole
    envs = [CartPole(seed0 + i, horizon) for i in range(n)]
    raw = np.stack([e.reset() for e in envs])
    return envs, raw


@functools.lru_cache(maxsize=None)
def _restated(case):
    hidden, gate, n, t_len, horizon, padded, pseed = case
    params = R.init_params(hidden, pseed)
    envs, raw = make_envs(n, ENV_SEED0, horizon)
    start = dict(params=params, raw=raw.copy(), seeds=[e.seed for e in envs])
    envs32 = copy.deepcopy(envs)
    kw = dict(gate=gate, n_global=n + ENV0_EXTRA + 1, env0=ENV0_EXTRA)
    want = R.rollout(params, envs, raw, t_len, NOISE_SEED, SAMPLER0, **kw)
    want32 = R.rollout(params, envs32, raw, t_len, NOISE_SEED, SAMPLER0, dtype=torch.float32, **kw)
    want["fp32_same_actions"] = bool(np.array_equal(want["action"], want32["action"]))
    return want, envs, start


def restated_rollout(case):
    """(the restatement's rollout, its environments AFTER the rollout, what the rollout started from).  Computed once per case;
    callers leave it unchanged."""
    return _restated(tuple(case))


@functools.lru_cache(maxsize=None)
def restated_agent_run():
    """AGENT['steps'] agent steps (rollout, update, RMSprop's averages carried) in fp64 -> dict(actions, masks [steps, T, N],
    events [(sampler step, env, return)], margin, fp32_same_actions, params (after the last update), init (the start))."""
    a = AGENT
    params = R.init_params(a["hidden"], a["param_seed"])
    init = {k: v.copy() for k, v in params.items()}
    envs, raw = make_envs(a["n_env"], a["task_seed"], a["horizon"])
    sq, step0 = None, 0
    actions, masks, events, margin, same = [], [], [], float("inf"), True
    for _ in range(a["steps"]):
        r32 = R.rollout(params, copy.deepcopy(envs), raw, a["t_len"], a["noise_seed"], step0, gate=a["gate"], dtype=torch.float32)
        r = R.rollout(params, envs, raw, a["t_len"], a["noise_seed"], step0, gate=a["gate"])
        same = same and bool(np.array_equal(r["action"], r32["action"]))
        margin = min(margin, r["margin"])
        actions.append(r["action"]); masks.append(r["mask"]); events += r["events"]
        states = np.concatenate([r["state"], r["bootstrap_state"][None]])
        params, keep = R.a2c_update(params, states, r["action"], r["reward"][..., None], r["mask"][..., None], a["discount"],
                                    a["gae_tau"], a["entropy_weight"], a["value_loss_weight"], a["gradient_clip"], a["lr"],
                                    gate=a["gate"], square_avg=sq)
        sq, raw, step0 = keep["square_avg"], r["raw_states"], step0 + a["t_len"] + 1
    return dict(actions=np.stack(actions), masks=np.stack(masks), events=events, margin=margin, fp32_same_actions=same,
                params=params, init=init)


def random_policy_mean(episodes=2000, seed=0, env_seed=1):
    """Mean return of the uniformly random policy on envs.CartPole over `episodes` seeded episodes (the closed-loop test's bar is
    twice this)."""
    from deeprl_amd.envs import CartPole
    rs = np.random.RandomState(seed)
    e = CartPole(env_seed)
    total = 0.0
    for _ in range(episodes):
        e.reset()
        done = False
        while not done:
            _, _, done, info = e.step(rs.randint(2))
        total += info['episodic_return']
    return total / episodes
