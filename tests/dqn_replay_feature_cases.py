"""The case tables of tests/test_dqn_replay_feature_host.py, tests/test_gpu_dqn_replay_feature.py and
tests/test_gpu_dqn_replay_feature_agent.py and their restatement (tests/dqn_replay_feature_restatement.py), computed once per case
and shared: the CPU suite checks what the cases cover (terminals at the first, a middle and the last position of a sampled window,
the index capacity - 1 - n_step, a duplicate, the largest importance weight in the last row block, the margins the argmax and relu
comparisons and the prioritised draws rest on), the GPU suite compares dra_dqn_replay_mlp_update and DQNAgent's device path under
config.fused_dqn_replay_feature with them."""
import functools
import random

import numpy as np
import torch

import dqn_feature_cases as K
import dqn_replay_feature_restatement as R

LR, DISCOUNT, GRADIENT_CLIP = K.LR, K.DISCOUNT, K.GRADIENT_CLIP
MARGIN, PREACT_MARGIN = K.MARGIN, K.PREACT_MARGIN
MAX_B, MAX_N_STEP = 256, 8      # dra_dqn_replay_mlp_update_supported's caps
REPLAY_EPS = 0.01

# two FULL rings of short episodes next to dqn_feature_cases' (a window of 8 always holds a terminal, one of 2 or 3 often does not):
# `pos` in the middle, so that capacity - 1 - n_step is a valid index
K.RINGS.setdefault("window_full", dict(capacity=64, fed=64 + 20, horizon=6, seed=35, action0=False))
K.RINGS.setdefault("window_long", dict(capacity=96, fed=96 + 30, horizon=13, seed=36, action0=False))
RINGS = K.RINGS

# (hidden, gate, batch, double_q, n_step, ring, per, replay_alpha, beta): hidden {16, 32, 64} x {relu, tanh}, the batches 1, 10, 63,
# 64, 65, 256 (one block and its edges, two blocks with a last block of one row, four blocks), windows of 1, 2, 3 and 8, both forms of
# q_next, the sqrt path (alpha 0.5) and powf (0.7), beta 0.4 and 1.0, and prob NULL (per False: the uniform replay's window).  The
# cases of 65 rows have their parameters behind a leading gap with NaN between them; the PER cases of 65 and 256 rows have the
# smallest probability -- the largest weight, the one every row is divided by -- in their LAST row.
UPDATE_CASES = ((64, "relu", 10, False, 3, "window_full", True, 0.5, 0.4),
                (16, "tanh", 1, False, 1, "window_full", True, 0.7, 1.0),
                (32, "relu", 63, True, 2, "window_full", True, 0.7, 0.4),
                (32, "tanh", 64, False, 8, "window_full", True, 0.5, 1.0),
                (16, "relu", 65, True, 3, "window_long", True, 0.7, 1.0),
                (64, "tanh", 256, True, 8, "window_long", True, 0.5, 0.4),
                (32, "relu", 10, False, 1, "window_long", True, 0.5, 0.4),
                (64, "relu", 65, False, 2, "window_full", False, 0.5, 0.4),
                (16, "tanh", 10, True, 8, "window_full", False, 0.5, 0.4))
UPDATE_SEED0 = 7400
# the first bump, found on the CPU by find_seed_bumps(), at which the restatement alone keeps the margins
SEED_BUMP = {(32, 'relu', 63, True, 2, 'window_full', True, 0.7, 0.4): 1}

# DQNAgent, device path against host loop and restatement, per kind: 10 agent steps of 4 transitions, exploration_steps 6 (crossed
# inside the second step), a target copy every 3 steps, a replay of 32 slots (it wraps in the ninth step) with n_step 3, minibatches
# of 8, episodes of at most 5 steps, epsilon from 0.8 to 0.1 over 30 calls.  The seeds (parameters, task, np.random, python random) are
# the first, found on the CPU by find_agent_seeds(), at which the restatement's run keeps the margins and shows what it is there for.
AGENT = dict(k=4, batch=8, capacity=32, exploration_steps=6, target_freq=3, horizon=5, steps=10, hidden=64, gate="relu", n_step=3,
             eps=(0.8, 0.1, 30), discount=DISCOUNT, gradient_clip=GRADIENT_CLIP, lr=LR, double_q=False, beta=(0.4, 1.0, 1e5),
             replay_eps=REPLAY_EPS, replay_alpha=0.5)
AGENT_SEEDS = dict(window=dict(param_seed=72, task_seed=3, np_seed=13, random_seed=17),
                   per=dict(param_seed=72, task_seed=3, np_seed=13, random_seed=17))
KINDS = ("window", "per")

# the reference fixture (tests/golden/make_golden_dqn_replay_feature.py): (tag, per, task seed, horizon, double_q,
# target_network_update_freq, hidden width), 12 steps of 4 transitions into a replay of 32 slots (it wraps) with n_step 3
FIXTURE = dict(capacity=32, batch=8, exploration_steps=8, eps=(0.6, 0.2, 40), np_seed=29, random_seed=31, steps=12, k=4, n_step=3,
               beta=(0.4, 1.0, 1e5), replay_eps=REPLAY_EPS, replay_alpha=0.5)
FIXTURE_TAGS = (("window", False, 11, 5, False, 5, 16), ("per", True, 13, 5, True, 5, 16))
FOLD_RING, FOLD_N_STEPS = "window_full", (1, 2, 3, 8)

LEARN_SEEDS, LAST_EPISODES = (1, 2, 3), 100


def update_id(c):
    return "h%d_%s_b%d_%s_n%d_%s_%s" % (c[0], c[1], c[2], "double" if c[3] else "max", c[4], c[5],
                                        "a%g_b%g" % (c[7], c[8]) if c[6] else "uniform")


make_ring, make_env = K.make_ring, K.make_env


def window_with_terminal_at(rg, n_step, where):
    """The first valid index whose window has a zero mask at position `where` -- its only one where such a window exists."""
    masks = rg["ring"]["masks"]
    found = [i for i in range(rg["size"]) if R.valid_index(i, rg["pos"], rg["size"], n_step) and masks[i + where] == 0]
    alone = [i for i in found if int((masks[i:i + n_step] == 0).sum()) == 1]
    return (alone or found or [None])[0]


def case_indices(case):
    """The case's data indices: the reference's rejection loop on a seeded RandomState; from 10 rows on with a terminal at the
    first, a middle and the last position of a window, the index capacity - 1 - n_step and a duplicate planted (rows 0 .. 5)."""
    batch, n_step, kind = case[2], case[4], case[5]
    rg = make_ring(kind)
    rs = np.random.RandomState(3000 + UPDATE_CASES.index(tuple(case)))
    idx = R.draw_indices(rs, batch, rg["pos"], rg["size"], n_step)
    if batch >= 10:
        for row, where in enumerate((0, n_step // 2, n_step - 1)):
            i = window_with_terminal_at(rg, n_step, where)
            if i is not None:
                idx[row] = i
        idx[3] = RINGS[kind]["capacity"] - 1 - n_step
        idx[5] = idx[4]
    assert all(R.valid_index(int(i), rg["pos"], rg["size"], n_step) for i in idx)
    return idx


def case_prob(case):
    """The case's sampling probabilities (float32), or None for a uniform case: from 65 rows on the smallest in the last row."""
    batch, per = case[2], case[6]
    if not per:
        return None
    rs = np.random.RandomState(5000 + UPDATE_CASES.index(tuple(case)))
    prob = rs.uniform(0.002, 0.05, batch).astype(np.float32)
    if batch >= 65:
        prob[-1] = np.float32(0.0005)
    return prob


def _update_at(case, bump):
    hidden, gate, batch, double_q, n_step, kind, per, alpha, beta = case
    seed = UPDATE_SEED0 + 10 * UPDATE_CASES.index(tuple(case)) + bump
    params, target = R.init_params(hidden, seed), R.init_params(hidden, seed + 50000)
    rg = make_ring(kind)
    idx, prob = case_indices(case), case_prob(case)
    mb = R.minibatch(rg["ring"], idx, n_step, DISCOUNT)
    kw = dict(prob=prob, beta=beta, replay_eps=REPLAY_EPS, replay_alpha=alpha)
    out = R.loss_and_grads(params, target, mb, DISCOUNT ** n_step, double_q, gate, **kw)
    out32 = R.loss_and_grads(params, target, mb, DISCOUNT ** n_step, double_q, gate, dtype=torch.float32, **kw)
    out.update(params=params, target=target, idx=idx, prob=prob, batch=mb,
               fp32_same_argmax=bool(np.array_equal(out["best"], out32["best"])))
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
    """The update case's parameters, data indices, probabilities and float32 n-step minibatch and the fp64 results on them
    (q_target, td, loss, prio, weights, grads, the margins).  Callers leave it unchanged."""
    return _restated_update(tuple(case))


def agent_cfg(kind, seeds=None):
    return dict(AGENT, per=kind == "per", **(seeds or AGENT_SEEDS[kind]))


def _agent_run(kind, seeds, steps, dtype):
    a = agent_cfg(kind, seeds)
    init = R.init_params(a["hidden"], a["param_seed"])
    env, _ = make_env(a["task_seed"], a["horizon"])
    rs, rnd = np.random.RandomState(a["np_seed"]), random.Random(a["random_seed"])
    eps = K.epsilon_schedule(*a["eps"])
    out = R.agent_run(init, env, a, rs, eps, rnd, steps or a["steps"], dtype=dtype or R.F64)
    out.update(init=init, rng_tail=rs.randint(0, 1 << 30, size=3), random_tail=[rnd.random() for _ in range(3)],
               epsilon=eps.state["current"])
    return out


@functools.lru_cache(maxsize=None)
def restated_agent_run(kind, steps=None, dtype=None):
    """R.agent_run over AGENT for the kind (fp64; dtype torch.float32: the margin test's run) with the generators' tails and the
    schedules' positions behind the run.  Callers leave it unchanged."""
    return _agent_run(kind, AGENT_SEEDS[kind], steps, dtype)


def run_conditions(out, per):
    """What a restated or recorded run shows: (updates that padded an invalid draw, updates that drew a leaf twice, updates with a
    terminal inside a sampled window, the smallest margin of the run -- greedy actions, double_q's argmax, the draws' uniforms)."""
    ups = [u for u in out["updates"] if u is not None]
    padded = sum(bool(u["padded"]) for u in ups) if per else 0
    twice = sum(len(set(u["leaves"].tolist())) < len(u["leaves"]) for u in ups) if per else 0
    terminal = sum(bool(u["window_terminal"]) for u in ups)
    return padded, twice, terminal, min(out["margin"], out["argmax_margin"], out["leaf_margin"])


def agent_run_ok(kind, out, out32):
    per = kind == "per"
    padded, twice, terminal, margin = run_conditions(out, per)
    if margin < MARGIN or out["min_preact"] < PREACT_MARGIN or terminal < 1 or (per and (padded < 1 or twice < 1)):
        return False
    same = np.array_equal(out["actions"], out32["actions"])
    return same and all((u is None) == (v is None) and (u is None or np.array_equal(u["data"], v["data"]))
                        for u, v in zip(out["updates"], out32["updates"]))


def find_agent_seeds(kind, limit=60):
    """AGENT_SEEDS[kind]: the first np.random / python random seed pair (13 + t, 17 + t) at which the run is well conditioned."""
    for t in range(limit):
        seeds = dict(AGENT_SEEDS[kind], np_seed=13 + t, random_seed=17 + t)
        if agent_run_ok(kind, _agent_run(kind, seeds, None, None), _agent_run(kind, seeds, None, torch.float32)):
            return seeds
    raise RuntimeError("no well-conditioned run of %s in %d seeds" % (kind, limit))


def restated(z, tag):
    """R.agent_run from a recorded reference run's initial parameters, target and seeds (tests/golden/dqn_replay_feature/steps.npz)."""
    f = FIXTURE
    _, per, task_seed, horizon, double_q, freq, hidden = next(t for t in FIXTURE_TAGS if t[0] == tag)
    cfg = dict(k=f["k"], batch=f["batch"], capacity=f["capacity"], exploration_steps=f["exploration_steps"], target_freq=freq,
               discount=DISCOUNT, n_step=f["n_step"], gradient_clip=GRADIENT_CLIP, lr=LR, double_q=bool(double_q), gate="relu",
               per=bool(per), beta=f["beta"], replay_eps=f["replay_eps"], replay_alpha=f["replay_alpha"])
    env, _ = make_env(task_seed, horizon)
    rs, rnd = np.random.RandomState(f["np_seed"]), random.Random(f["random_seed"])
    init = {k: z["%s_init_%s" % (tag, k)] for k in R.KEYS}
    target0 = {k: z["%s_target0_%s" % (tag, k)] for k in R.KEYS}
    out = R.agent_run(init, env, cfg, rs, K.epsilon_schedule(*f["eps"]), rnd, f["steps"], target0=target0)
    out.update(rng_tail=rs.randint(0, 1 << 30, size=3), random_tail=np.asarray([rnd.random() for _ in range(3)]))
    return out
