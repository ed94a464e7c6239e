"""The case tables of tests/test_rainbow_feature_host.py and tests/test_gpu_rainbow_feature.py and their restatement
(tests/rainbow_feature_restatement.py), computed once per case and shared.  The CPU suite checks what the cases cover and the
margins every bit comparison rests on: at every transition and every a_next choice of every case the restatement's two action
values are at least MARGIN apart (and the same arithmetic in fp32 chooses the same), at every relu unit the pre-activation is at
least PREACT_MARGIN from 0.  A case's parameter seed is its base seed plus the first bump at which the restatement ALONE keeps those
margins (dist_feature_cases.first_bump: a deterministic search on the CPU, no row is ever excluded)."""
import copy
import functools

import numpy as np
import torch

import rainbow_feature_restatement as R
from dist_feature_cases import SUPPORT, first_bump, make_env, make_ring as _dist_ring      # noqa: F401

DISCOUNT = 0.99
ENV_SEED, STEP0 = 70, 9     # the environment's seed; the device step counter's value before the launch
EP_RING_CAP, EP_RING_COUNT0 = 8, 6      # the test's episode ring is short and starts near its end: the appended rows wrap
MARGIN = 1e-4               # the smallest |q_1 - q_0| at a transition / an a_next choice the comparisons tolerate
PREACT_MARGIN = 1e-5        # the smallest |pre-activation| of a relu case: the derivative is the same in fp32 and fp64
MAX_K, MAX_B, MAX_ATOMS, MAX_N_STEP, ROW_BLOCK = 8, 64, 51, 8, 16      # the kernels' caps and the update's row block
REPLAY_EPS, REPLAY_ALPHA = 0.01, 0.5
NOISE_PAD = 5               # floats in front of a noise row's vectors and behind each of them (padded layouts)


def spec_of(n, support=None):
    lo, hi = support or SUPPORT[n]
    return dict(n=n, v_min=lo, v_max=hi)


def noise_layout(hidden, n, padded):
    """({state_dict key: offset in a noise row}, the row's length): the vectors in the draw order back to back at multiples of 4
    (nets._NoiseBlock's layout), or -- padded -- NOISE_PAD floats apart behind a leading gap."""
    offs, off = {}, NOISE_PAD if padded else 0
    for layer in R.DRAW_ORDER:
        o, i = R.dims(hidden, n)[layer]
        for b, size in zip(R.NOISE, (i, o, o)):
            offs["%s.%s" % (layer, b)] = off
            off += size + NOISE_PAD if padded else (size + 3) // 4 * 4
    return offs, off


def noise_row(z, hidden, n, padded, fill=np.nan):
    offs, size = noise_layout(hidden, n, padded)
    row = np.full(size, fill if padded else 0.0, dtype=np.float32)
    for k, o in offs.items():
        row[o:o + z[k].size] = z[k]
    return row


# ------------------------------------------------------------------------------------------ the acting kernel
# (hidden, gate, atoms, transitions, replay capacity, first slot, horizon, padded parameter and noise buffers, base seed): (16, 64) x
# both gates x atoms {2, 50, 51} x transitions {1, 4, 8}; then a run that wraps the ring (first slot capacity - 2) and a horizon of 3
# (episodes end inside the launch) behind padded buffers.  Every transition runs under a noise row of its own.
def _act_cases():
    out, seed = [], 900
    for hidden in (16, 64):
        for gate in ("relu", "tanh"):
            for n in (2, 50, 51):
                for k in (1, 4, 8):
                    out.append((hidden, gate, n, k, 64, 5, 200, False, seed))
                    seed += 50
    out.append((32, "relu", 50, 8, 12, 10, 200, False, seed))
    out.append((32, "tanh", 51, 8, 32, 3, 3, True, seed + 50))
    return tuple(out)


ACT_CASES = _act_cases()


def act_id(c):
    return "h%d_%s_n%d_k%d_cap%d_slot%d_hz%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], "_padded" if c[7] else "")


def _act_at(case, bump):
    hidden, gate, n, k_len, capacity, slot0, horizon, _, seed = case
    spec = spec_of(n)
    params = R.init_params(hidden, seed + bump, n)
    rows = [R.draw_noise(hidden, n, seed + 1000 + 7 * k) for k in range(k_len)]
    env, raw = make_env(ENV_SEED, horizon)
    explore, rand = np.zeros(k_len, dtype=bool), np.zeros(k_len, dtype=np.int64)      # epsilon is 0 under noisy layers
    start = dict(params=params, noise_rows=rows, raw=raw.copy(), seed=env.seed, explore=explore, random_action=rand, spec=spec)
    env32 = copy.deepcopy(env)
    ring, ring32 = R.new_ring(capacity), R.new_ring(capacity)
    want = R.act(params, rows, env, raw, k_len, explore, rand, ring, slot0, spec, gate=gate, step0=STEP0)
    want32 = R.act(params, rows, env32, raw, k_len, explore, rand, ring32, slot0, spec, gate=gate, step0=STEP0, dtype=torch.float32)
    want["fp32_same_actions"] = bool(np.array_equal(want["action"], want32["action"]))
    want["ring"] = ring
    return want, env, start


@functools.lru_cache(maxsize=None)
def _restated_act(case):
    bump, got = first_bump(lambda b: _act_at(case, b), lambda g: g[0]["margin"] >= MARGIN and g[0]["fp32_same_actions"])
    got[0]["bump"] = bump
    return got


def restated_act(case):
    """(the restatement's launch -- q, action, events, raw, margin, ring --, its environment AFTER it, what it started from).
    Computed once per case; callers leave it unchanged."""
    return _restated_act(tuple(case))


# the noise-row test: ONE parameter set, an observation near the origin and noise rows of which the even ones choose action 0 and the
# odd ones action 1 (found by a deterministic search): only a kernel that reads row k at transition k alternates
FLIP = dict(hidden=16, gate="tanh", n=50, k=8, seed=77)


def _flip_at(noise_seed):
    hidden, gate, n, k_len = FLIP["hidden"], FLIP["gate"], FLIP["n"], FLIP["k"]
    spec = spec_of(n)
    params = R.init_params(hidden, FLIP["seed"], n)
    env, raw = make_env(ENV_SEED, 200)
    p = R.to_t(params)
    rows, probe, seed = [], copy.deepcopy(env), noise_seed
    obs = raw.copy()
    with torch.no_grad():
        for k in range(k_len):
            while True:      # the first noise seed under which the greedy action at this observation is k % 2, with margin
                z = R.draw_noise(hidden, n, seed)
                seed += 1
                q = R.forward(p, R.to_t(z), obs.astype(np.float32)[None], spec, gate).numpy()[0]
                if int(np.argmax(q)) == k % 2 and abs(q[1] - q[0]) >= 100 * MARGIN:
                    break
            rows.append(z)
            s, _, done, _ = probe.step(k % 2)
            obs = np.asarray(probe.reset() if done else s, dtype=np.float64)
    explore, rand = np.zeros(k_len, dtype=bool), np.zeros(k_len, dtype=np.int64)
    start = dict(params=params, noise_rows=rows, raw=raw.copy(), seed=env.seed, explore=explore, random_action=rand, spec=spec)

    def run(noise_rows, e):
        ring = R.new_ring(64)
        out = R.act(params, noise_rows, e, raw, k_len, explore, rand, ring, 0, spec, gate=gate, step0=STEP0)
        out["ring"] = ring
        return out
    got = run(rows, env)
    alone = [run([rows[fixed]] * k_len, make_env(ENV_SEED, 200)[0])["action"] for fixed in (0, k_len - 1)]
    return got, env, start, alone


@functools.lru_cache(maxsize=None)
def flip_case():
    """(the restatement's launch, its environment AFTER it, what it started from): the first noise seed at which the actions
    alternate under the rows in turn and do NOT under row 0 alone or row K - 1 alone."""
    want = np.arange(FLIP["k"]) % 2
    _, got = first_bump(lambda b: _flip_at(5000 + 1000 * b),
                        lambda g: np.array_equal(g[0]["action"], want) and not any(np.array_equal(a, want) for a in g[3]))
    return got[:3]


# ------------------------------------------------------------------------------------------ the update kernel
# rings: dist_feature_cases' (transitions of a random policy, episodes of at most 9 steps in `partial`: terminals inside most n-step
# windows) with NON-UNIT rewards written over `partial`'s (the fold's order and its masks show); action0, clamps, terminal and
# on_atoms as they are there
@functools.lru_cache(maxsize=None)
def make_ring(kind):
    rg = _dist_ring(kind)
    ring = {k: v.copy() for k, v in rg["ring"].items()}
    if kind in ("partial", "action0"):
        i = np.arange(rg["size"])
        ring["rewards"][:rg["size"]] = 0.5 + 0.37 * (i % 7) - 0.9 * (i % 3 == 0)
    return dict(ring=ring, pos=rg["pos"], size=rg["size"])


UPDATE_BATCHES = (1, ROW_BLOCK - 1, ROW_BLOCK, ROW_BLOCK + 1, 2 * ROW_BLOCK, 2 * ROW_BLOCK + 1, MAX_B)


# (atoms, hidden, gate, batch, double_q, ring, n_step, beta, discount, support or None): atoms {2, 50, 51} x the batches around the row
# block and the cap, the networks going round the six (hidden, gate) pairs, double_q / n_step {3, 1} / beta {0.4, 1} alternating so
# that every value meets every atom count; the entry's own shape (50 atoms, hidden 64, relu, batch 32, double_q, n_step 3) among them;
# every batch of 17 behind padded buffers; then the ring kinds
def _update_cases():
    out = []
    nets = ((16, "tanh"), (64, "relu"), (32, "relu"), (32, "tanh"), (64, "tanh"), (16, "relu"))
    i = 0
    for n in (2, 50, 51):
        for b in UPDATE_BATCHES:
            hidden, gate = nets[i % len(nets)]
            out.append((n, hidden, gate, b, i % 2 == 0, "partial", 3 if i % 3 else 1, 0.4 if i % 4 < 2 else 1.0, DISCOUNT, None))
            i += 1
    out.append((50, 64, "relu", 32, True, "partial", 3, 0.4, DISCOUNT, None))
    out.append((50, 64, "relu", 32, False, "partial", 3, 1.0, DISCOUNT, None))
    out.append((51, 64, "tanh", MAX_B, True, "partial", MAX_N_STEP, 0.7, DISCOUNT, None))
    out.append((50, 64, "relu", 10, True, "action0", 3, 0.4, DISCOUNT, None))
    out.append((51, 32, "relu", 10, False, "clamps", 3, 0.4, DISCOUNT, None))
    out.append((51, 32, "tanh", 10, True, "terminal", 3, 1.0, DISCOUNT, None))
    out.append((51, 64, "relu", 10, False, "on_atoms", 1, 0.4, 1.0, (-25.0, 25.0)))
    out.append((51, 16, "relu", 10, True, "on_atoms", 3, 0.4, 1.0, (-25.0, 25.0)))
    assert len(set(out)) == len(out)
    return tuple(out)


UPDATE_CASES = _update_cases()
UPDATE_SEED0 = 7000


def update_id(c):
    return "n%d_h%d_%s_b%d_%s_%s_nstep%d_beta%g" % (c[0], c[1], c[2], c[3], "double" if c[4] else "max", c[5], c[6], c[7])


def update_padded(case):
    return case[3] == ROW_BLOCK + 1


def update_spec(case):
    return spec_of(case[0], case[9])


def valid_index(i, pos, size, n_step):
    """replay.py:105-110 with history_length 1."""
    return (i >= 0 and i + n_step < pos) or (i >= pos and i + n_step < size)


def case_indices(case):
    """The case's DATA indices: uniformly drawn valid ones from a seeded RandomState; from 4 rows on (n_step 3, a ring with
    terminals) a terminal at EVERY position of the window, and from 6 rows on index 0, the last valid index and a duplicate."""
    batch, kind, n_step = case[3], case[5], case[6]
    rg = make_ring(kind)
    rs = np.random.RandomState(3000 + UPDATE_CASES.index(tuple(case)))
    idx = []
    while len(idx) < batch:
        i = int(rs.randint(0, rg["size"]))
        if valid_index(i, rg["pos"], rg["size"], n_step):
            idx.append(i)
    idx = np.asarray(idx, dtype=np.int64)
    masks = rg["ring"]["masks"]
    if batch >= 4 and n_step == 3 and kind == "partial":
        t = next(j for j in range(10, rg["size"]) if masks[j] == 0)
        idx[0], idx[1], idx[2] = t, t - 1, t - 2
    if batch >= 6:
        last = max(j for j in range(rg["size"]) if valid_index(j, rg["pos"], rg["size"], n_step))
        idx[3], idx[4], idx[5] = 0, last, idx[2]
    assert all(valid_index(int(i), rg["pos"], rg["size"], n_step) for i in idx)
    return idx


def case_probs(case):
    """The sampling probabilities (float32): uniform in [1e-4, 0.1]; from 2 rows on one very small and one near 1."""
    rs = np.random.RandomState(8000 + UPDATE_CASES.index(tuple(case)))
    p = rs.uniform(1e-4, 0.1, case[3]).astype(np.float32)
    if case[3] >= 2:
        p[0], p[1] = 1e-7, 0.97
    return p


def _update_at(case, bump):
    n, hidden, gate, batch, double_q, kind, n_step, beta, discount, _ = case
    spec = update_spec(case)
    seed = UPDATE_SEED0 + 50 * UPDATE_CASES.index(tuple(case)) + bump
    params, target = R.init_params(hidden, seed, n), R.init_params(hidden, seed + 50000, n)
    noise, target_noise = R.draw_noise(hidden, n, seed + 1), R.draw_noise(hidden, n, seed + 2)
    rg = make_ring(kind)
    idx, prob = case_indices(case), case_probs(case)
    mb = R.minibatch(rg["ring"], idx, n_step, discount)
    args = (params, target, noise, target_noise, mb, prob, beta, discount ** n_step, spec, double_q, REPLAY_EPS, REPLAY_ALPHA, gate)
    out = R.loss_and_grads(*args)
    out32 = R.loss_and_grads(*args, dtype=torch.float32)
    out.update(params=params, target_params=target, noise=noise, target_noise=target_noise, idx=idx, prob=prob, batch=mb, spec=spec,
               fp32_same_argmax=bool(np.array_equal(out["a_next"], out32["a_next"])))
    return out


def _margins_hold(case, out):
    if case[2] == "relu" and out["min_preact"] < PREACT_MARGIN:
        return False
    return out["argmax_margin"] >= MARGIN and out["fp32_same_argmax"]


@functools.lru_cache(maxsize=None)
def _restated_update(case):
    bump, out = first_bump(lambda b: _update_at(case, b), lambda o: _margins_hold(case, o))
    out["bump"] = bump
    return out


def restated_update(case):
    """The update case's parameters, noise, indices, probabilities and float32 minibatch and the fp64 results on them.  Callers
    leave it unchanged."""
    return _restated_update(tuple(case))


# ------------------------------------------------------------------------------------------ the recorded runs (steps.npz)
# the recorded runs of the reference's CategoricalDQNAgent: 4 transitions per step, minibatches of 8 from a PrioritizedReplay of 48
# slots with n_step 3, exploration_steps 8 (two acting-only steps), then eleven steps that update -- the ring wraps in the last.
# (The first updates draw 8 strata from a dozen leaves of priority about 1: a leaf that straddles two strata is drawn twice.)
FIXTURE = dict(k=4, batch=8, capacity=48, exploration_steps=8, steps=13, n_step=3, np_seed=23, random_seed=29, noise_seed=31,
               std=0.1, beta=(0.4, 1.0, 1e5), replay_eps=0.01, replay_alpha=0.5, lr=0.001, gradient_clip=10)
# (tag, task seed, episode horizon, double_q, target copy period, hidden, atoms, v_min, v_max)
FIXTURE_TAGS = (("dq_n5", 3, 5, True, 200, 16, 5, -10.0, 10.0),
                ("plain_n3", 4, 5, False, 200, 16, 3, -10.0, 10.0),
                ("dq_n50_copy", 5, 7, True, 5, 16, 50, -100.0, 100.0))


def fixture_cfg(spec):
    """rainbow_feature_restatement.agent_run's cfg for a FIXTURE_TAGS row."""
    tag, task_seed, horizon, double_q, freq, hidden, n, lo, hi = spec
    f = FIXTURE
    return dict(k=f["k"], batch=f["batch"], capacity=f["capacity"], exploration_steps=f["exploration_steps"], target_freq=freq,
                discount=DISCOUNT, n_step=f["n_step"], gradient_clip=f["gradient_clip"], lr=f["lr"], double_q=double_q, gate="relu",
                spec=dict(n=n, v_min=lo, v_max=hi), hidden=hidden, std=f["std"], beta=f["beta"], replay_eps=f["replay_eps"],
                replay_alpha=f["replay_alpha"])


def unflat_noise(flat, hidden, n):
    """A recorded noise row (the vectors in R.NOISE_KEYS' order back to back) -> the dict of raw noise vectors."""
    out, at = {}, 0
    for layer in R.DRAW_ORDER:
        o, i = R.dims(hidden, n)[layer]
        for b, size in zip(R.NOISE, (i, o, o)):
            out["%s.%s" % (layer, b)] = np.asarray(flat[at:at + size], dtype=np.float32)
            at += size
    assert at == len(flat)
    return out


def fixture_updates(z, tag):
    """Per recorded update of `tag` what the update kernel is launched on and what the reference left: dict(params (before),
    target_params, noise, target_noise, ring, idx (DATA indices), prob, beta, kl, prio, after (the parameters behind the step))."""
    spec = next(t for t in FIXTURE_TAGS if t[0] == tag)
    hidden, n, cap = spec[5], spec[6], FIXTURE["capacity"]
    steps, copies = [int(s) for s in z[tag + "_update_steps"]], set(int(s) for s in z[tag + "_copies"])
    grab = lambda what, u=None: {k: (z["%s_%s_%s" % (tag, what, k)] if u is None else z["%s_%s_%s" % (tag, what, k)][u]) for k in R.KEYS}
    params, target, out = grab("init"), grab("target0"), []
    for u, step in enumerate(steps):
        after = grab("params", u)
        out.append(dict(params=params, target_params=target, noise=unflat_noise(z[tag + "_noise"][u], hidden, n),
                        target_noise=unflat_noise(z[tag + "_target_noise"][u], hidden, n),
                        ring={k: z["%s_ring_%s" % (tag, k)][u] for k in ("frames", "actions", "rewards", "masks")},
                        idx=z[tag + "_leaves"][u] - (cap - 1), prob=z[tag + "_prob"][u], beta=float(z[tag + "_beta"][u]),
                        kl=z[tag + "_kl"][u], prio=z[tag + "_prio"][u], after=after, spec=dict(n=n, v_min=spec[7], v_max=spec[8])))
        params = after
        if step in copies:
            target = after
    return out


def restated(z, tag):
    """rainbow_feature_restatement.agent_run on a recorded run's initial parameters and seeds (np.random and torch's generator are
    seeded here and left where the run leaves them; python's random is an instance of its own)."""
    import random
    spec = next(t for t in FIXTURE_TAGS if t[0] == tag)
    f = FIXTURE
    init = {k: z["%s_init_%s" % (tag, k)] for k in R.KEYS}
    target0 = {k: z["%s_target0_%s" % (tag, k)] for k in R.KEYS}
    env, _ = make_env(spec[1], spec[2])
    np.random.seed(f["np_seed"])
    torch.manual_seed(f["noise_seed"])
    rnd = random.Random(f["random_seed"])
    out = R.agent_run(init, env, fixture_cfg(spec), rnd, f["steps"], target0=target0)
    out["random_tail"] = np.asarray([rnd.random() for _ in range(3)])
    return out
