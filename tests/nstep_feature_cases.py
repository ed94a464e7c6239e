"""The case tables of tests/test_nstep_feature_host.py and tests/test_gpu_nstep_feature.py and their restatement
(tests/nstep_feature_restatement.py), computed once per case and shared: the CPU suite checks what the cases cover (terminals,
ring rows, exploring and greedy pairs, the Q margins the GPU action comparisons rest on, the relu pre-activation margins the
gradient comparisons rest on), the GPU suite compares dra_q_mlp_rollout, dra_q_mlp_update and NStepDQNAgent's device path with
them."""
import copy
import functools

import numpy as np
import torch

import nstep_feature_restatement as R

# (hidden, gate, n_env, t_len, horizon, padded parameter buffers, online seed, target seed, exploration seed): the
# n_step_dqn_feature shape; one environment and one step; the smallest width with tanh, an odd environment count (three row
# blocks, the last one partial), more steps than a wave has lanes and a horizon that ends every episode every third step; the
# middle width at the largest environment count (every lane of the environment wave) with a horizon of 2; the largest everything
# with the parameters behind a leading gap and NaN padding between them
ROLLOUT_CASES = ((64, "relu", 5, 5, 200, False, 51, 151, 251),
                 (64, "relu", 1, 1, 200, False, 52, 152, 252),
                 (16, "tanh", 17, 33, 3, False, 53, 153, 253),
                 (32, "relu", 64, 3, 2, False, 54, 154, 254),
                 (64, "tanh", 64, 5, 200, True, 55, 155, 255))
EPSILON = 0.5               # exploration of the kernel cases: explore = rand < 0.5 from a seeded RandomState
ENV_SEED0, STEP0 = 70, 9    # the environments' seeds start here; the device step counter's value before the rollout
RING_CAP, RING_COUNT0 = 64, 61      # the test's ring is short and starts near its end: the appended rows wrap
MARGIN = 1e-4               # the smallest |q_1 - q_0| at a non-exploring (step, environment) the action comparisons tolerate
PREACT_MARGIN = 1e-5        # the smallest |pre-activation| of a relu case: the derivative is the same in fp32 and fp64
UPDATE_CAP = 1024           # dra_q_mlp_update_supported's cap on rows

# (hidden, gate, n_env, t_len, horizon, every action forced to 0, online seed, target seed, exploration seed): one row; the
# example's 25 rows; 51 rows: odd, one partial row block, zero masks; 320 rows: five full blocks (every n_env the rollout takes at
# the example's rollout length); the stated cap, 16 blocks; one action only: the head's other row gets exactly zero
UPDATE_CASES = ((64, "relu", 1, 1, 200, False, 61, 161, 261),
                (64, "relu", 5, 5, 200, False, 62, 162, 262),
                (16, "tanh", 17, 3, 2, False, 63, 163, 263),
                (32, "relu", 64, 5, 200, False, 70, 164, 264),
                (16, "tanh", 64, 16, 3, False, 65, 165, 265),
                (64, "relu", 8, 4, 200, True, 66, 166, 266))
DISCOUNT = 0.99

# the closed-loop test: three seeds, the statistic and where its bar comes from (tests/golden/nstep_feature/)
LEARN_SEEDS = (1, 2, 3)
LAST_EPISODES = 100

# NStepDQNAgent, device path against host-stepped path: 4 environments, rollouts of 5, episodes of at most 7 steps, 6 agent
# steps, epsilon from 1.0 to 0.1 over 100 steps, a target copy every 3 steps (inside and between rollouts)
AGENT = dict(n_env=4, t_len=5, horizon=7, steps=6, hidden=64, gate="relu", param_seed=71, task_seed=3, np_seed=13,
             eps=(1.0, 0.1, 100), target_freq=3, discount=0.99, gradient_clip=5, lr=0.001)


def case_id(c):
    return "h%d_%s_n%d_t%d_hz%d%s" % (c[0], c[1], c[2], c[3], c[4], "_padded" if c[5] else "")


def update_id(c):
    return "h%d_%s_n%d_t%d_hz%d%s" % (c[0], c[1], c[2], c[3], c[4], "_action0" if c[5] else "")


def make_envs(n, seed0, horizon):
    from deeprl_amd.envs import CartPole
    envs = [CartPole(seed0 + i, horizon) for i in range(n)]
    raw = np.stack([e.reset() for e in envs])
    return envs, raw


def exploration(seed, t_len, n, force_zero=False):
    rs = np.random.RandomState(seed)
    explore = rs.rand(t_len, n) < EPSILON
    random_action = rs.randint(2, size=(t_len, n)).astype(np.int64)
    if force_zero:
        explore, random_action = np.ones((t_len, n), dtype=bool), np.zeros((t_len, n), dtype=np.int64)
    return explore, random_action


@functools.lru_cache(maxsize=None)
def _restated(case, force_zero=False):
    hidden, gate, n, t_len, horizon, _, pseed, tseed, xseed = case
    params, target = R.init_params(hidden, pseed), R.init_params(hidden, tseed)
    envs, raw = make_envs(n, ENV_SEED0, horizon)
    explore, rand = exploration(xseed, t_len, n, force_zero)
    start = dict(params=params, target=target, raw=raw.copy(), seeds=[e.seed for e in envs], explore=explore, random_action=rand)
    envs32 = copy.deepcopy(envs)
    want = R.rollout(params, target, envs, raw, t_len, explore, rand, gate=gate, step0=STEP0)
    want32 = R.rollout(params, target, envs32, raw, t_len, explore, rand, gate=gate, step0=STEP0, dtype=torch.float32)
    want["fp32_same_actions"] = bool(np.array_equal(want["action"], want32["action"]))
    return want, envs, start


def restated_rollout(case):
    """(the restatement's rollout, its environments AFTER the rollout, what the rollout started from).  Computed once per case;
    callers leave it unchanged."""
    return _restated(tuple(case))


@functools.lru_cache(maxsize=None)
def _restated_update(case):
    hidden, gate, n, t_len, horizon, force_zero, pseed, tseed, xseed = case
    roll, _, start = _restated(tuple(case), bool(force_zero))
    inputs = dict(state=roll["state"], action=roll["action"], reward=roll["reward"], mask=roll["mask"],
                  bootstrap=roll["bootstrap"].astype(np.float32))
    ret, loss, grads, q, pre = R.loss_and_grads(start["params"], inputs["state"], inputs["action"], inputs["reward"], inputs["mask"],
                                                inputs["bootstrap"], DISCOUNT, gate)
    min_pre = float(min(np.abs(pre["z1"]).min(), np.abs(pre["z2"]).min()))
    return dict(inputs=inputs, params=start["params"], ret=ret, loss=loss, grads=grads, q=q, min_preact=min_pre, events=roll["events"])


def restated_update(case):
    """The update case's inputs (what a rollout of the restatement leaves: float32 states, actions, rewards, masks, the float32
    bootstrap) and the fp64 results on them: ret, loss, grads, the smallest |pre-activation|.  Callers leave it unchanged."""
    return _restated_update(tuple(case))


def epsilon_schedule(start, end, steps):
    """support.LinearSchedule's arithmetic as a generator of (value before the call) for calls with `n` steps each."""
    inc = (end - start) / float(steps)
    state = dict(current=start)

    def call(n):
        v = state["current"]
        state["current"] = max(state["current"] + inc * n, end) if end < start else min(state["current"] + inc * n, end)
        return v
    call.state = state
    return call


@functools.lru_cache(maxsize=None)
def restated_agent_run():
    """AGENT['steps'] agent steps (exploration draws in the reference's order from RandomState(np_seed), target copies where
    NStepDQN_agent.py:48-50 makes them, rollout, update, RMSprop's averages carried) in fp64 -> dict(actions, masks [steps, T, N],
    events [(step counter, env, return)], margin, fp32_same_actions, explored / greedy counts, params (after the last update), init,
    rng_tail, epsilon (the schedule's value after the run))."""
    a = AGENT
    params = R.init_params(a["hidden"], a["param_seed"])
    init = {k: v.copy() for k, v in params.items()}
    target = {k: v.copy() for k, v in params.items()}
    envs, raw = make_envs(a["n_env"], a["task_seed"], a["horizon"])
    rs = np.random.RandomState(a["np_seed"])
    eps = epsilon_schedule(*a["eps"])
    n, t_len = a["n_env"], a["t_len"]
    sq, step0, total = None, 0, 0
    actions, masks, events, margin, same, explored, greedy = [], [], [], float("inf"), True, 0, 0
    for _ in range(a["steps"]):
        explore, rand = np.empty((t_len, n), dtype=bool), np.empty((t_len, n), dtype=np.int64)
        sync = False
        for t in range(t_len):
            e = eps(n)
            rand[t] = rs.randint(2, size=n)
            explore[t] = rs.rand(n) < e
            total += n
            sync = sync or (total // n % a["target_freq"] == 0)
        if sync:
            target = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
        r32 = R.rollout(params, target, copy.deepcopy(envs), raw, t_len, explore, rand, gate=a["gate"], step0=step0, dtype=torch.float32)
        r = R.rollout(params, target, envs, raw, t_len, explore, rand, gate=a["gate"], step0=step0)
        same = same and bool(np.array_equal(r["action"], r32["action"]))
        margin = min(margin, r["margin"])
        explored, greedy = explored + int(explore.sum()), greedy + int((~explore).sum())
        actions.append(r["action"]); masks.append(r["mask"]); events += r["events"]
        states = np.concatenate([r["state"], r["bootstrap_state"][None]])
        params, keep = R.nstep_update(params, target, states, r["action"], r["reward"], r["mask"], a["discount"], a["gradient_clip"],
                                      a["lr"], gate=a["gate"], square_avg=sq)
        sq, raw, step0 = keep["square_avg"], r["raw_states"], step0 + t_len
    return dict(actions=np.stack(actions), masks=np.stack(masks), events=events, margin=margin, fp32_same_actions=same,
                explored=explored, greedy=greedy, params=params, init=init, rng_tail=rs.randint(0, 1 << 30, size=3),
                epsilon=eps.state["current"], total=total)


def random_policy_mean(episodes=2000, seed=0, env_seed=1):
    """a2c_feature_cases.random_policy_mean: the uniformly random policy's mean return on envs.CartPole."""
    import a2c_feature_cases
    return a2c_feature_cases.random_policy_mean(episodes, seed, env_seed)
