"""The case tables of tests/test_option_critic_feature_host.py and tests/test_gpu_option_critic_feature.py and their restatement
(tests/option_critic_feature_restatement.py), computed once per case and shared: the CPU suite checks what the cases cover (both
option branches, terminals, ring rows, the decision margins the GPU option / action comparisons rest on, the relu pre-activation
margins the gradient comparisons rest on), the GPU suite compares dra_oc_mlp_rollout, dra_oc_mlp_update and OptionCriticAgent's
cart-pole device path with them."""
import copy
import functools

import numpy as np
import torch

import option_critic_feature_restatement as R
from nstep_feature_cases import (ENV_SEED0, MARGIN, PREACT_MARGIN, RING_CAP, RING_COUNT0, STEP0, UPDATE_CAP,      # noqa: F401
                                 epsilon_schedule, make_envs)

# (hidden, gate, n_env, t_len, horizon, options, padded parameter buffers, online seed, target seed, uniform seed): one
# environment and one step; the option_critic_feature shape; the smallest width with tanh, an odd environment count, more steps
# than a wave has lanes, a horizon that ends every episode every third step and an odd option count; the middle width at the
# largest environment count with a horizon of 2 and the largest option count (2048 head outputs a step: eight per thread); the
# largest everything with the parameters behind a leading gap and NaN padding between them
ROLLOUT_CASES = ((64, "relu", 1, 1, 200, 2, False, 51, 151, 251),
                 (64, "relu", 5, 5, 200, 2, False, 52, 152, 252),
                 (16, "tanh", 17, 33, 3, 3, False, 53, 153, 253),
                 (32, "relu", 64, 3, 2, 8, False, 54, 154, 254),
                 (64, "tanh", 64, 5, 200, 8, True, 55, 155, 256))
EPS_RANGE = (0.7, 0.3)      # the option epsilon of the kernel cases: from 0.7 at the first step down to 0.3 at the last

# (hidden, gate, n_env, t_len, horizon, options, every row the same option, online seed, target seed, uniform seed): one row; the
# example's 25 rows; 51 rows: odd, one partial row block, zero masks and init rows; 320 rows: five full blocks; the stated cap, 16
# blocks; one option only: the heads' other rows get exactly zero
UPDATE_CASES = ((64, "relu", 1, 1, 200, 2, False, 61, 161, 261),
                (64, "relu", 5, 5, 200, 2, False, 62, 162, 262),
                (16, "tanh", 17, 3, 2, 3, False, 63, 163, 263),
                (32, "relu", 64, 5, 200, 8, False, 64, 164, 264),
                (16, "tanh", 64, 16, 200, 8, False, 65, 165, 265),
                (64, "relu", 8, 4, 200, 4, True, 69, 166, 266))
FORCED_OPTION = 1           # the option (and prev_option) of every row of the last update case
DISCOUNT, TERM_REG, ENT_W = 0.99, 0.01, 0.01

# the closed-loop test: three seeds, the statistic and where its bar comes from (tests/golden/option_critic_feature/)
LEARN_SEEDS = (1, 2, 3)
LAST_EPISODES = 100

# OptionCriticAgent, device path against host-stepped path: 4 environments, rollouts of 5, episodes of at most 7 steps, 6 agent
# steps, 2 options, option epsilon from 1.0 to 0.1 over 100 steps, a target copy every 3 steps (inside and between rollouts)
AGENT = dict(n_env=4, t_len=5, horizon=7, steps=6, hidden=64, gate="relu", options=2, param_seed=71, task_seed=3, torch_seed=13,
             eps=(1.0, 0.1, 100), target_freq=3, discount=0.99, gradient_clip=5, lr=0.001, term_reg=0.01, ent_w=0.01)


def case_id(c):
    return "h%d_%s_n%d_t%d_hz%d_o%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "_padded" if c[6] else "")


def update_id(c):
    return "h%d_%s_n%d_t%d_hz%d_o%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "_one_option" if c[6] else "")


def draws(seed, t_len, n):
    """(eps [T] float32, uniform [T, N, 3] float32) of a kernel case."""
    rs = np.random.RandomState(seed)
    return np.linspace(EPS_RANGE[0], EPS_RANGE[1], t_len).astype(np.float32), rs.rand(t_len, n, 3).astype(np.float32)


def carried_start(n, n_opt):
    """A mixed carried state: every option as prev_option, every third environment initial."""
    return ((np.arange(n) * 3 + 1) % n_opt).astype(np.int64), (np.arange(n) % 3 == 0)


@functools.lru_cache(maxsize=None)
def _restated(case, force=False):
    hidden, gate, n, t_len, horizon, n_opt, _, pseed, tseed, useed = case
    params, target = R.init_params(hidden, pseed, n_opt), R.init_params(hidden, tseed, n_opt)
    envs, raw = make_envs(n, ENV_SEED0, horizon)
    eps, uniform = draws(useed, t_len, n)
    prev, init = carried_start(n, n_opt)
    kw = dict(gate=gate, step0=STEP0)
    if force:
        prev = np.full(n, FORCED_OPTION, dtype=np.int64)
        kw["force_option"] = FORCED_OPTION
    start = dict(params=params, target=target, raw=raw.copy(), seeds=[e.seed for e in envs], eps=eps, uniform=uniform,
                 prev_option=prev.copy(), is_initial=init.copy())
    envs32 = copy.deepcopy(envs)
    want = R.rollout(params, target, envs, raw, t_len, eps, uniform, prev, init, **kw)
    want32 = R.rollout(params, target, envs32, raw, t_len, eps, uniform, prev, init, dtype=torch.float32, **kw)
    want["fp32_same_decisions"] = bool(np.array_equal(want["option"], want32["option"]) and
                                       np.array_equal(want["action"], want32["action"]))
    return want, envs, start


def restated_rollout(case):
    """(the restatement's rollout, its environments AFTER the rollout, what the rollout started from).  Computed once per case;
    callers leave it unchanged."""
    return _restated(tuple(case))


UPDATE_INPUTS = ("state", "q", "beta", "logits", "option", "prev_option", "action", "init", "log_pi_a", "entropy", "reward", "mask",
                 "bootstrap")


@functools.lru_cache(maxsize=None)
def _restated_update(case):
    roll, _, start = _restated(tuple(case), bool(case[6]))
    f32 = lambda k: roll[k].astype(np.float32) if roll[k].dtype == np.float64 else roll[k]
    inputs = {k: f32(k) for k in UPDATE_INPUTS}
    out = R.loss_and_grads(start["params"], inputs, start["eps"], DISCOUNT, TERM_REG, ENT_W, case[1])
    out.update(inputs=inputs, params=start["params"], eps=start["eps"], events=roll["events"], margin=roll["margin"],
               fp32_same_decisions=roll["fp32_same_decisions"],
               min_preact=float(min(np.abs(out["z1"]).min(), np.abs(out["z2"]).min())))
    return out


def restated_update(case):
    """The update case's inputs (what a rollout of the restatement leaves, narrowed to float32 as the rollout kernel stores it)
    and the fp64 results on them: ret, adv, beta_adv, loss [4], grads, the smallest |pre-activation|.  Callers leave it unchanged."""
    return _restated_update(tuple(case))


def restated_agent_run(uniforms):
    """AGENT['steps'] agent steps in fp64 fed the uniforms [steps, T, N, 3] the device run drew (the option epsilon from the
    schedule in the reference's order, target copies where OptionCritic_agent.py:83-85 makes them, rollout, update, RMSprop's
    averages carried) -> dict(options, actions, masks [steps, T, N], events, margin, fp32_same_decisions, params (after the last
    update), init, epsilon (the schedule's value after the run), total)."""
    a = AGENT
    params = R.init_params(a["hidden"], a["param_seed"], a["options"])
    target = {k: v.copy() for k, v in params.items()}
    envs, raw = make_envs(a["n_env"], a["task_seed"], a["horizon"])
    eps = epsilon_schedule(*a["eps"])
    n, t_len = a["n_env"], a["t_len"]
    prev, init = np.ones(n, dtype=np.int64), np.ones(n, dtype=bool)
    sq, step0, total = None, 0, 0
    options, actions, masks, events, margin, same = [], [], [], [], float("inf"), True
    for s in range(a["steps"]):
        e, sync = np.empty(t_len, dtype=np.float32), False
        for t in range(t_len):
            e[t] = eps(n)
            total += n
            sync = sync or (total // n % a["target_freq"] == 0)
        if sync:
            target = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
        r32 = R.rollout(params, target, copy.deepcopy(envs), raw, t_len, e, uniforms[s], prev, init, gate=a["gate"], step0=step0,
                        dtype=torch.float32)
        r = R.rollout(params, target, envs, raw, t_len, e, uniforms[s], prev, init, gate=a["gate"], step0=step0)
        same = same and bool(np.array_equal(r["option"], r32["option"]) and np.array_equal(r["action"], r32["action"]))
        margin = min(margin, r["margin"])
        options.append(r["option"]); actions.append(r["action"]); masks.append(r["mask"]); events += r["events"]
        params, keep = R.oc_update(params, r, a["discount"], a["term_reg"], a["ent_w"], a["gradient_clip"], a["lr"], gate=a["gate"],
                                   square_avg=sq)
        sq, raw, step0, prev, init = keep["square_avg"], r["raw_states"], step0 + t_len, r["prev_option_out"], r["is_initial_out"]
    return dict(options=np.stack(options), actions=np.stack(actions), masks=np.stack(masks), events=events, margin=margin,
                fp32_same_decisions=same, params=params, epsilon=eps.state["current"], total=total, prev_option=prev, is_initial=init)


def agent_init_params():
    a = AGENT
    return R.init_params(a["hidden"], a["param_seed"], a["options"])


def random_policy_mean(episodes=2000, seed=0, env_seed=1):
    """a2c_feature_cases.random_policy_mean: the uniformly random policy's mean return on envs.CartPole."""
    import a2c_feature_cases
    return a2c_feature_cases.random_policy_mean(episodes, seed, env_seed)
