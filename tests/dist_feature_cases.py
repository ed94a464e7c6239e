"""The case tables of tests/test_dist_feature_host.py and tests/test_gpu_dist_feature.py and their restatement
(tests/dist_feature_restatement.py), computed once per case and shared.  The CPU suite checks what the cases cover and the margins
every bit comparison rests on: at every greedy transition and every a_next choice of every case the restatement's two action values
are at least MARGIN apart (and the same arithmetic in fp32 chooses the same), at every relu unit the pre-activation is at least
PREACT_MARGIN from 0.  A case's parameter seed is its base seed plus the first bump at which the restatement ALONE keeps those
margins (first_bump: a deterministic search on the CPU, no row is ever excluded); the GPU suite compares dra_dist_mlp_act,
dra_dist_mlp_update and the two agents' device path with the same cases."""
import copy
import functools

import numpy as np
import torch

import dist_feature_restatement as R
from dqn_feature_cases import epsilon_schedule, make_env, random_policy_mean      # noqa: F401

LR, DISCOUNT, GRADIENT_CLIP = 0.001, 0.99, 5
EPSILON = 0.5               # exploration of the kernel cases: explore = rand < 0.5 from a seeded RandomState
ENV_SEED, STEP0 = 70, 9     # the environment's seed; the device step counter's value before the launch
EP_RING_CAP, EP_RING_COUNT0 = 8, 6      # the test's episode ring is short and starts near its end: the appended rows wrap
MARGIN = 1e-4               # the smallest |q_1 - q_0| at a greedy transition / an a_next choice the comparisons tolerate
PREACT_MARGIN = 1e-5        # the smallest |pre-activation| of a relu case: the derivative is the same in fp32 and fp64
MAX_K, MAX_B, MAX_ATOMS, ROW_BLOCK = 8, 256, 51, 16      # the kernels' caps and the update's row block
HEADS = ("c51", "qr")
HEAD_CODE = {"c51": 1, "qr": 2}
# the categorical support per atom count: the entry's 50 atoms on [-100, 100]; 51 on [-10, 10] (the pixel entries'); narrow ones
# for the small counts
SUPPORT = {2: (-1.0, 1.0), 20: (-10.0, 10.0), 50: (-100.0, 100.0), 51: (-10.0, 10.0)}


def spec_of(head, n, support=None):
    if head == "qr":
        return dict(head="qr", n=n, v_min=0.0, v_max=0.0)
    lo, hi = support or SUPPORT[n]
    return dict(head="c51", n=n, v_min=lo, v_max=hi)


def _hashable(spec):
    return (spec["head"], spec["n"], spec["v_min"], spec["v_max"])


# ------------------------------------------------------------------------------------------ the acting kernel
# (head, hidden, gate, atoms, transitions, replay capacity, first slot, horizon, padded parameter buffers, base seed): both heads x
# (16 tanh, 64 relu) x atoms {2, 20, 51} x transitions {1, 4, 8}; then per head a run that wraps the ring (first slot capacity - 2)
# and a horizon of 3 (episodes end inside the launch), the second behind padded parameter buffers
def _act_cases():
    out, seed = [], 600
    for head in HEADS:
        for hidden, gate in ((16, "tanh"), (64, "relu")):
            for n in (2, 20, 51):
                for k in (1, 4, 8):
                    out.append((head, hidden, gate, n, k, 64, 5, 200, False, seed))
                    seed += 50
        out.append((head, 32, "relu", 20, 8, 12, 10, 200, False, seed))
        out.append((head, 32, "tanh", 51, 8, 32, 3, 3, True, seed + 50))
        seed += 100
    return tuple(out)


ACT_CASES = _act_cases()


def act_id(c):
    return "%s_h%d_%s_n%d_k%d_cap%d_slot%d_hz%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], "_padded" if c[8] else "")


def _act_at(case, bump):
    head, hidden, gate, n, k_len, capacity, slot0, horizon, _, seed = case
    spec = spec_of(head, n)
    params = R.init_params(hidden, seed + bump, spec)
    env, raw = make_env(ENV_SEED, horizon)
    rs = np.random.RandomState(seed + 7)
    explore, rand = rs.rand(k_len) < EPSILON, rs.randint(2, size=k_len).astype(np.int64)
    if k_len == 1:
        explore[:] = False      # (the one transition of the smallest cases is a greedy one)
    else:
        explore[0], explore[1] = False, True      # (both kinds in every longer case)
    start = dict(params=params, raw=raw.copy(), seed=env.seed, explore=explore, random_action=rand, spec=spec)
    env32 = copy.deepcopy(env)
    ring, ring32 = R.new_ring(capacity), R.new_ring(capacity)
    want = R.act(params, env, raw, k_len, explore, rand, ring, slot0, spec, gate=gate, step0=STEP0)
    want32 = R.act(params, env32, raw, k_len, explore, rand, ring32, slot0, spec, gate=gate, step0=STEP0, dtype=torch.float32)
    want["fp32_same_actions"] = bool(np.array_equal(want["action"], want32["action"]))
    want["fp32_q_error"] = float(np.abs(want32["q"] - want["q"]).max() / (1e-5 * max(np.abs(want["q"]).max(), 1.0)))
    want["ring"] = ring
    return want, env, start


def first_bump(make, holds, limit=40):
    """(bump, what make(bump) returned) for the first bump < limit at which holds(...) is true."""
    for bump in range(limit):
        got = make(bump)
        if holds(got):
            return bump, got
    raise AssertionError("no seed bump below %d keeps the margins" % limit)


@functools.lru_cache(maxsize=None)
def _restated_act(case):
    bump, got = first_bump(lambda b: _act_at(case, b), lambda g: g[0]["margin"] >= MARGIN and g[0]["fp32_same_actions"])
    got[0]["bump"] = bump
    return got


def restated_act(case):
    """(the restatement's launch -- q, action, events, raw, margin, ring --, its environment AFTER it, what it started from).
    Computed once per case; callers leave it unchanged."""
    return _restated_act(tuple(case))


# ------------------------------------------------------------------------------------------ the update kernel
# rings: `fed` transitions of a uniformly random policy through the restatement's acting loop, then edited: action0 = action 0
# alone; clamps (c51) = rewards +-30 that push Tz past both ends of [-10, 10]; terminal (c51) = every mask 0: gamma m = 0, all mass
# on the one or two atoms around r; on_atoms (c51) = rewards 3 = 3 delta, every mask 1 (with discount 1 and the support [-25, 25]
# of 51 atoms, delta 1, every Tz is an atom or clamps onto the last one)
RINGS = dict(partial=dict(capacity=300, fed=260, horizon=9, seed=31),
             action0=dict(capacity=64, fed=40, horizon=200, seed=33, action0=True),
             clamps=dict(capacity=64, fed=48, horizon=9, seed=34, rewards=(30.0, -30.0, 6.0, -6.0)),
             terminal=dict(capacity=64, fed=48, horizon=9, seed=35, rewards=(0.3, 1.7), masks=0),
             on_atoms=dict(capacity=64, fed=48, horizon=9, seed=36, rewards=(3.0,), masks=1))
R_ = ROW_BLOCK
UPDATE_BATCHES = (1, 10, R_ - 1, R_, R_ + 1, 2 * R_ + 1)


# (head, atoms, hidden, gate, batch, double_q, ring, discount, support or None): both heads x atoms {2, 20, 50, 51} x the batches
# around the row block (c51: with and without double_q; every batch of 17 behind padded buffers; the networks go round the six
# (hidden, gate) pairs, the entries' own shape -- 50 atoms / hidden 64 / relu / batch 10 -- among them), 256 once per head, then the
# ring kinds
def _update_cases():
    out = []
    nets = ((16, "tanh"), (64, "relu"), (32, "relu"), (32, "tanh"), (64, "tanh"), (16, "relu"))
    for head in HEADS:
        i = 0
        for n in (2, 20, 50, 51):
            for b in UPDATE_BATCHES:
                hidden, gate = nets[i % len(nets)]
                for double_q in ((False, True) if head == "c51" else (False,)):
                    out.append((head, n, hidden, gate, b, double_q, "partial", DISCOUNT, None))
                i += 1
        out.append((head, 51, 64, "relu", 256, head == "c51", "partial", DISCOUNT, None))
        out.append((head, 20, 64, "relu", 10, False, "action0", DISCOUNT, None))
    out.append(("c51", 51, 32, "relu", 10, False, "clamps", DISCOUNT, None))
    out.append(("c51", 51, 32, "tanh", 10, True, "terminal", DISCOUNT, None))
    out.append(("c51", 51, 64, "relu", 10, False, "on_atoms", 1.0, (-25.0, 25.0)))
    assert len(set(out)) == len(out)
    return tuple(out)


UPDATE_CASES = _update_cases()
UPDATE_SEED0 = 4000


def update_id(c):
    return "%s_n%d_h%d_%s_b%d_%s_%s" % (c[0], c[1], c[2], c[3], c[4], "double" if c[5] else "max", c[6])


def update_padded(case):
    return case[4] == ROW_BLOCK + 1


def update_spec(case):
    return spec_of(case[0], case[1], case[8])


@functools.lru_cache(maxsize=None)
def make_ring(kind):
    """dict(ring, pos, size) of a ring kind."""
    spec = RINGS[kind]
    env, raw = make_env(spec["seed"], spec["horizon"])
    rs = np.random.RandomState(spec["seed"])
    ring = R.new_ring(spec["capacity"])
    plain = dict(head="qr", n=2, v_min=0.0, v_max=0.0)
    params = R.init_params(16, 1, plain)
    pos = size = 0
    for _ in range(spec["fed"]):
        a = 0 if spec.get("action0") else int(rs.randint(2))
        out = R.act(params, env, raw, 1, [True], [a], ring, pos, plain)
        raw = out["raw"]
        if pos >= size:
            size += 1
        pos = (pos + 1) % spec["capacity"]
    if "rewards" in spec:
        vals = spec["rewards"]
        ring["rewards"][:size] = [vals[i % len(vals)] for i in range(size)]
    if "masks" in spec:
        ring["masks"][:size] = spec["masks"]
    return dict(ring=ring, pos=pos, size=size)


def case_indices(case):
    """The case's indices: the reference's rejection loop on a seeded RandomState; from 4 rows on with index 0, the last valid
    index and a duplicate planted."""
    batch, kind = case[4], case[6]
    rg = make_ring(kind)
    rs = np.random.RandomState(1000 + UPDATE_CASES.index(tuple(case)))
    idx = R.draw_indices(rs, batch, rg["pos"], rg["size"])
    if batch >= 4:
        last = rg["size"] - 2 if rg["size"] - 2 >= rg["pos"] else rg["pos"] - 2
        idx[0], idx[1], idx[3] = 0, last, idx[2]
    assert all(R.valid_index(int(i), rg["pos"], rg["size"]) for i in idx)
    return idx


def _update_at(case, bump):
    head, n, hidden, gate, batch, double_q, kind, discount, _ = case
    spec = update_spec(case)
    seed = UPDATE_SEED0 + 50 * UPDATE_CASES.index(tuple(case)) + bump
    params, target = R.init_params(hidden, seed, spec), R.init_params(hidden, seed + 50000, spec)
    rg = make_ring(kind)
    idx = case_indices(case)
    mb = R.minibatch(rg["ring"], idx)
    out = R.loss_and_grads(params, target, mb, discount, spec, double_q, gate)
    out32 = R.loss_and_grads(params, target, mb, discount, spec, double_q, gate, dtype=torch.float32)
    out.update(params=params, target_params=target, idx=idx, batch=mb, spec=spec,
               fp32_same_argmax=bool(np.array_equal(out["a_next"], out32["a_next"])))
    return out


def _margins_hold(case, out):
    if case[3] == "relu" and out["min_preact"] < PREACT_MARGIN:
        return False
    return out["argmax_margin"] >= MARGIN and out["fp32_same_argmax"]


@functools.lru_cache(maxsize=None)
def _restated_update(case):
    bump, out = first_bump(lambda b: _update_at(case, b), lambda o: _margins_hold(case, o))
    out["bump"] = bump
    return out


def restated_update(case):
    """The update case's parameters (params, target_params), indices and float32 minibatch and the fp64 results on them.  Callers
    leave it unchanged."""
    return _restated_update(tuple(case))


# ------------------------------------------------------------------------------------------ the reference fixture
# tests/golden/make_golden_dist_feature.py: (tag, head, task seed, horizon, double_q, target_network_update_freq, hidden width);
# 20 atoms on [-10, 10] / 20 quantiles; the replay's 48 slots fill exactly
FIXTURE = dict(capacity=48, batch=10, exploration_steps=8, eps=(0.6, 0.2, 40), np_seed=29, steps=12, k=4, n=20, v_min=-10.0, v_max=10.0)
FIXTURE_TAGS = (("c51", "c51", 11, 200, False, 200, 32), ("c51_double_q", "c51", 13, 200, True, 200, 16),
                ("c51_hz3", "c51", 17, 3, False, 200, 16), ("c51_copy", "c51", 19, 200, False, 5, 16),
                ("qr", "qr", 23, 200, False, 200, 32), ("qr_hz3", "qr", 27, 3, False, 200, 16), ("qr_copy", "qr", 29, 200, False, 5, 16))


def fixture_spec(head):
    return spec_of(head, FIXTURE["n"], (FIXTURE["v_min"], FIXTURE["v_max"]))


# ------------------------------------------------------------------------------------------ the agents
# dqn_feature's agent case for both agent classes: 8 agent steps of 4 transitions, exploration_steps 6 (crossed inside the second
# step), a target copy every 3 steps, a replay of 24 slots (it wraps in the seventh step), episodes of at most 5 steps, epsilon from
# 0.8 to 0.1 over 30 calls; 20 atoms on [-10, 10] / 20 quantiles; param_seed is a base: the first bump that keeps the margins is used
AGENT = dict(k=4, batch=10, capacity=24, exploration_steps=6, target_freq=3, horizon=5, steps=8, hidden=64, gate="relu",
             param_seed=720, task_seed=3, np_seed=13, eps=(0.8, 0.1, 30), discount=DISCOUNT, gradient_clip=GRADIENT_CLIP, lr=LR,
             double_q=False, n=20, v_min=-10.0, v_max=10.0)
LEARN_SEEDS = (1, 2, 3)
LAST_EPISODES = 100


def _agent_run_at(head, bump, steps, exploration_steps, dtype):
    a = dict(AGENT)
    if exploration_steps is not None:
        a["exploration_steps"] = exploration_steps
    a["spec"] = spec = spec_of(head, a["n"], (a["v_min"], a["v_max"]))
    init = R.init_params(a["hidden"], a["param_seed"] + bump, spec)
    env, _ = make_env(a["task_seed"], a["horizon"])
    rs = np.random.RandomState(a["np_seed"])
    eps = epsilon_schedule(*a["eps"])
    out = R.agent_run(init, env, a, rs, eps, steps or a["steps"], dtype=dtype or R.F64)
    out.update(init=init, rng_tail=rs.randint(0, 1 << 30, size=3), epsilon=eps.state["current"], spec=spec)
    return out


def _agent_holds(head, steps, exploration_steps):
    def holds(out):
        if out["margin"] < MARGIN or out["argmax_margin"] < MARGIN or out["min_preact"] < PREACT_MARGIN:
            return False
        return np.array_equal(out["actions"], _agent_run_at(head, out["_bump"], steps, exploration_steps, torch.float32)["actions"])
    return holds


@functools.lru_cache(maxsize=None)
def agent_bump(head):
    """The first bump of AGENT's param_seed at which the 8-step run AND the 10-step run of the graph test keep the margins."""
    def make(b):
        out = _agent_run_at(head, b, None, None, None)
        out["_bump"] = b
        return out

    def holds(out):
        if not _agent_holds(head, None, None)(out):
            return False
        long = _agent_run_at(head, out["_bump"], 10, 14, None)
        long["_bump"] = out["_bump"]
        return _agent_holds(head, 10, 14)(long)
    return first_bump(make, holds)[0]


@functools.lru_cache(maxsize=None)
def restated_agent_run(head, steps=None, exploration_steps=None, dtype=None):
    """R.agent_run over AGENT for a head kind (fp64; dtype torch.float32: the margin test's run) with its np.random tail and the
    schedule's position behind the run."""
    return _agent_run_at(head, agent_bump(head), steps, exploration_steps, dtype)
