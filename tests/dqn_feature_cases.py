"""The case tables of tests/test_dqn_feature_host.py and tests/test_gpu_dqn_feature.py and their restatement
(tests/dqn_feature_restatement.py), computed once per case and shared: the CPU suite checks what the cases cover (terminals, a
wrapping slot run, exploring and greedy transitions, zero masks, duplicate indices, index 0 and the last valid index, the Q
margins the action and argmax comparisons rest on, the relu pre-activation margins the gradient comparisons rest on), the GPU
suite compares dra_dqn_mlp_act, dra_dqn_mlp_update and DQNAgent's device path with them."""
import copy
import functools

import numpy as np
import torch

import dqn_feature_restatement as R

LR, DISCOUNT, GRADIENT_CLIP = 0.001, 0.99, 5
EPSILON = 0.5               # exploration of the kernel cases: explore = rand < 0.5 from a seeded RandomState
ENV_SEED, STEP0 = 70, 9     # the environment's seed; the device step counter's value before the launch
EP_RING_CAP, EP_RING_COUNT0 = 8, 6      # the test's episode ring is short and starts near its end: the appended rows wrap
MARGIN = 1e-4               # the smallest |q_1 - q_0| at a greedy transition / a double_q argmax the comparisons tolerate
PREACT_MARGIN = 1e-5        # the smallest |pre-activation| of a relu case: the derivative is the same in fp32 and fp64
MAX_K, MAX_B = 8, 256       # dra_dqn_mlp_supported's / dra_dqn_mlp_update_supported's caps

# (hidden, gate, transitions, replay capacity, first slot, horizon, padded parameter buffers, parameter seed, exploration seed):
# the example's; the smallest; a wrapping slot run (more transitions than slots: the later row of a slot stays) with episodes that
# end every second transition; the largest with the parameters behind a leading gap and NaN padding between them
ACT_CASES = ((64, "relu", 4, 64, 0, 200, False, 51, 251),
             (16, "tanh", 1, 16, 3, 200, False, 52, 252),
             (32, "relu", 8, 6, 4, 2, False, 53, 253),
             (64, "tanh", 8, 32, 10, 200, True, 54, 254))

# the update cases: every (hidden, gate) x every batch of UPDATE_BATCHES x double_q off / on over the ring "partial" (300 slots,
# 260 written, episodes of at most 9 steps: zero masks), then a ring that is full with `pos` in its middle and an all-one-action
# ring.  A case: (hidden, gate, batch, double_q, ring).  Its parameter seeds are UPDATE_SEED0 + 10 x its position + SEED_BUMP (the
# first bump, found on the CPU by find_seed_bumps(), at which the restatement alone keeps the margins above).
NETS = ((16, "relu"), (16, "tanh"), (32, "relu"), (32, "tanh"), (64, "relu"), (64, "tanh"))
UPDATE_BATCHES = (1, 10, 32, 64, 65, 256)
UPDATE_CASES = tuple((h, g, b, dq, "partial") for h, g in NETS for b in UPDATE_BATCHES for dq in (False, True)) + (
    (64, "relu", 32, False, "full_mid"), (32, "tanh", 65, True, "full_mid"), (64, "relu", 10, False, "action0"))
UPDATE_SEED0 = 400
SEED_BUMP = {(16, 'relu', 64, False, 'partial'): 2, (16, 'relu', 256, True, 'partial'): 3, (32, 'relu', 65, True, 'partial'): 2,
             (32, 'relu', 256, False, 'partial'): 2, (32, 'relu', 256, True, 'partial'): 2, (64, 'relu', 256, False, 'partial'): 6,
             (64, 'relu', 256, True, 'partial'): 1}
RINGS = dict(partial=dict(capacity=300, fed=260, horizon=9, seed=31, action0=False),
             full_mid=dict(capacity=96, fed=96 + 41, horizon=9, seed=32, action0=False),
             action0=dict(capacity=64, fed=40, horizon=200, seed=33, action0=True))

# the closed-loop test: three seeds, the statistic and where its bar comes from (tests/golden/dqn_feature/)
LEARN_SEEDS = (1, 2, 3)
LAST_EPISODES = 100

# the reference fixture (tests/golden/make_golden_dqn_feature.py): (tag, task seed, horizon, double_q, target_network_update_freq,
# hidden width -- the widths are small so that a parameter snapshot per step keeps the file small).  The replay's 48 slots fill
# exactly: the ring behind step s is the first 4 (s + 1) rows of the recorded one
FIXTURE = dict(capacity=48, batch=10, exploration_steps=8, eps=(0.6, 0.2, 40), np_seed=29, steps=12, k=4)
FIXTURE_TAGS = (("uniform", 11, 200, False, 200, 32), ("double_q", 13, 200, True, 200, 16), ("hz3", 17, 3, False, 200, 16),
                ("copy", 19, 200, False, 5, 16))

# DQNAgent, device path against host loop and restatement: 8 agent steps of 4 transitions, exploration_steps 6 (crossed in the
# middle of the second step's transitions), a target copy every 3 steps (after the third and the sixth), a replay of 24 slots
# (it wraps in the seventh step), episodes of at most 5 steps, epsilon from 0.8 to 0.1 over 30 calls
AGENT = dict(k=4, batch=10, capacity=24, exploration_steps=6, target_freq=3, horizon=5, steps=8, hidden=64, gate="relu",
             param_seed=72, task_seed=3, np_seed=13, eps=(0.8, 0.1, 30), discount=DISCOUNT, gradient_clip=GRADIENT_CLIP, lr=LR,
             double_q=False)


def act_id(c):
    return "h%d_%s_k%d_cap%d_slot%d_hz%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "_padded" if c[6] else "")


def update_id(c):
    return "h%d_%s_b%d_%s_%s" % (c[0], c[1], c[2], "double" if c[3] else "max", c[4])


def make_env(seed, horizon):
    from deeprl_amd.envs import CartPole
    env = CartPole(seed, horizon)
    return env, env.reset()


@functools.lru_cache(maxsize=None)
def _restated_act(case):
    hidden, gate, k_len, capacity, slot0, horizon, _, pseed, xseed = case
    params = R.init_params(hidden, pseed)
    env, raw = make_env(ENV_SEED, horizon)
    rs = np.random.RandomState(xseed)
    explore, rand = rs.rand(k_len) < EPSILON, rs.randint(2, size=k_len).astype(np.int64)
    if k_len == 1:
        explore[:] = False      # (the one transition of the smallest case is a greedy one)
    start = dict(params=params, raw=raw.copy(), seed=env.seed, explore=explore, random_action=rand)
    env32 = copy.deepcopy(env)
    ring, ring32 = R.new_ring(capacity), R.new_ring(capacity)
    want = R.act(params, env, raw, k_len, explore, rand, ring, slot0, gate=gate, step0=STEP0)
    want32 = R.act(params, env32, raw, k_len, explore, rand, ring32, slot0, gate=gate, step0=STEP0, dtype=torch.float32)
    want["fp32_same_actions"] = bool(np.array_equal(want["action"], want32["action"]))
    want["ring"] = ring
    return want, env, start


def restated_act(case):
    """(the restatement's launch -- q, action, events, raw, margin, ring --, its environment AFTER it, what it started from).
    Computed once per case; callers leave it unchanged."""
    return _restated_act(tuple(case))


@functools.lru_cache(maxsize=None)
def make_ring(kind):
    """dict(ring, pos, size): `fed` transitions of a uniformly random policy (action0: of action 0 alone) through the
    restatement's acting loop."""
    spec = RINGS[kind]
    env, raw = make_env(spec["seed"], spec["horizon"])
    rs = np.random.RandomState(spec["seed"])
    ring = R.new_ring(spec["capacity"])
    params = R.init_params(16, 1)
    pos = size = 0
    for _ in range(spec["fed"]):
        a = 0 if spec["action0"] else int(rs.randint(2))
        out = R.act(params, env, raw, 1, [True], [a], ring, pos)
        raw = out["raw"]
        if pos >= size:
            size += 1
        pos = (pos + 1) % spec["capacity"]
    return dict(ring=ring, pos=pos, size=size)


def case_indices(case):
    """The case's indices: the reference's rejection loop on a seeded RandomState; from 4 rows on with index 0, the last valid
    index and a duplicate planted."""
    batch, kind = case[2], case[4]
    rg = make_ring(kind)
    rs = np.random.RandomState(1000 + UPDATE_CASES.index(tuple(case)))
    idx = R.draw_indices(rs, batch, rg["pos"], rg["size"])
    if batch >= 4:
        last = rg["size"] - 2 if rg["size"] - 2 >= rg["pos"] else rg["pos"] - 2
        idx[0], idx[1], idx[3] = 0, last, idx[2]
    assert all(R.valid_index(int(i), rg["pos"], rg["size"]) for i in idx)
    return idx


def _update_at(case, bump):
    hidden, gate, batch, double_q, kind = case
    seed = UPDATE_SEED0 + 10 * UPDATE_CASES.index(tuple(case)) + bump
    params, target = R.init_params(hidden, seed), R.init_params(hidden, seed + 50000)
    rg = make_ring(kind)
    idx = case_indices(case)
    mb = R.minibatch(rg["ring"], idx)
    out = R.loss_and_grads(params, target, mb, DISCOUNT, double_q, gate)
    out32 = R.loss_and_grads(params, target, mb, DISCOUNT, double_q, gate, dtype=torch.float32)
    out.update(params=params, target=target, idx=idx, batch=mb, fp32_same_argmax=bool(np.array_equal(out["best"], out32["best"])))
    return out


def _margins_hold(case, out):
    if case[1] == "relu" and out["min_preact"] < PREACT_MARGIN:
        return False
    return not case[3] or (out["argmax_margin"] >= MARGIN and out["fp32_same_argmax"])


def find_seed_bumps(limit=40):
    """The table SEED_BUMP holds: per case the first bump at which the restatement keeps the margins (cases at bump 0 left out)."""
    table = {}
    for case in UPDATE_CASES:
        bump = next(b for b in range(limit) if _margins_hold(case, _update_at(case, b)))
        if bump:
            table[case] = bump
    return table


@functools.lru_cache(maxsize=None)
def _restated_update(case):
    return _update_at(case, SEED_BUMP.get(case, 0))


def restated_update(case):
    """The update case's parameters, indices and float32 minibatch and the fp64 results on them (q_target, td, loss, grads, the
    margins).  Callers leave it unchanged."""
    return _restated_update(tuple(case))


def epsilon_schedule(start, end, steps):
    """support.LinearSchedule's arithmetic: call() returns the value before the call and advances by one step."""
    inc = (end - start) / float(steps)
    state = dict(current=start)

    def call():
        v = state["current"]
        state["current"] = max(state["current"] + inc, end) if end < start else min(state["current"] + inc, end)
        return v
    call.state = state
    return call


@functools.lru_cache(maxsize=None)
def restated_agent_run(steps=None, exploration_steps=None, dtype=None):
    """R.agent_run over AGENT (fp64; dtype torch.float32: the margin test's run) with its np.random tail and the schedule's
    position behind the run."""
    a = dict(AGENT)
    if exploration_steps is not None:
        a["exploration_steps"] = exploration_steps
    init = R.init_params(a["hidden"], a["param_seed"])
    env, _ = make_env(a["task_seed"], a["horizon"])
    rs = np.random.RandomState(a["np_seed"])
    eps = epsilon_schedule(*a["eps"])
    out = R.agent_run(init, env, a, rs, eps, steps or a["steps"], dtype=dtype or R.F64)
    out.update(init=init, rng_tail=rs.randint(0, 1 << 30, size=3), epsilon=eps.state["current"])
    return out


def random_policy_mean(episodes=2000, seed=0, env_seed=1):
    """a2c_feature_cases.random_policy_mean: the uniformly random policy's mean return on envs.CartPole."""
    import a2c_feature_cases
    return a2c_feature_cases.random_policy_mean(episodes, seed, env_seed)
