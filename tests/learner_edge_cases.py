"""Edge-shape cases, the float64 reference and the bar for the fused DQN learner (csrc/learner.hip: dra_dqn_learner_update / _step /
_act) at the batch sizes, action counts and head sizes where its code changes path.  NOT a test file: CPU only, imported by
tests/test_learner_edge_cases_host.py (which proves on the CPU that the inputs carry the bar, that every first update has
unambiguous ReLU gates and that every case reaches the path it is named for) and by tests/test_gpu_learner_edges.py (which holds
the kernels to it).

The reference is ONE whole update in float64 on the CPU from a given float32 state: oracle.net_oracle (nature_conv_body_margin,
the vanilla / categorical / quantile heads), oracle.loss_oracle (dqn_td_error, c51_kl, qr_loss), autograd, the gradient norm as
the float64 root of the sum of squares, the clip of torch.nn.utils.clip_grad_norm_, then net_oracle.rmsprop_step / adam_step --
every tensor float64 built from its float32 value, scalar hyperparameters first rounded to float32 (as the kernels hold them).
Every update is judged on its own: the reference starts from the learner's exported state before that update.

The bar is the project's 1e-5 of scale, not a number tuned to the kernels:
  out, vec     head outputs (q / logits / quantiles) and the loss vector (TD errors / KL per sample / quantile loss per target
               quantile): max |got - want| <= 1e-5 x max |want| per tensor
  loss, norm   1e-5 relative (the norm against the float64 sum of squares)
  params       rtol 1e-5, atol 2e-6 (RMSprop) / 5e-6 (Adam): the existing figures of tests/test_gpu_agents.py
  state, grad  the two optimizer-state tensors per parameter tensor after the FIRST update (zero state before it: they are
               (1 - alpha) g and (1 - alpha) g^2, resp. (1 - beta1) g and (1 - beta2) g^2, of the clipped gradient g -- every
               gradient element, signed, on every path) and, where a path leaves it there, the flat gradient itself:
               max |got - want| <= 1e-5 x max |want| per tensor
An update whose float64 ReLU margin (the smallest |pre-activation| of the differentiated forward) is below 5e-7 is judged at 100x
(two correct float32 implementations may gate that unit differently): never the first update of a case (proved on the CPU), at
most one later update per case.  BAR_OVERRIDES is where a tensor whose INPUTS cannot carry 1e-5 would get max(1e-5, 4 x the error
of the float32 CPU run of the same reference), with both figures beside it; it is empty: the float32 CPU run meets every bar."""
import functools

import numpy as np
import torch

import fake_envs
from oracle import loss_oracle as L, net_oracle as N, numerics_oracle as NUM
from oracle.async_schedule_oracle import draw_uniform_indices
from oracle.replay_oracle import UniformReplayOracle
from oracle.synth_oracle import synth_transitions

BAR = 1e-5
MARGIN = 5e-7                # nature_conv_body_margin below this: an ambiguous ReLU gate
AMBIGUOUS_FACTOR = 100.0
CAP = 512                    # ring slots
RING_SEED = 9
DONE_PERIOD = 3              # a third of the synthetic transitions are terminal: no minibatch set without one
GAMMA = 0.99
PARAM_SEEDS = (21, 22)       # fake_envs.numpy_params: online, target ("normal" initialisation)
# (case name, tensor key) -> (bar, error / scale of the float32 CPU run of the reference on the same inputs)
BAR_OVERRIDES = {}

HEADS = {
    # head: parameter prefix, optimizer, and the hyperparameters DQNLearnerBench gives it (examples.py of the reference)
    "vanilla": dict(param="fc_head", optimizer="rmsprop", clip=5.0, lr=0.00025, alpha=0.95, eps=0.01, atol=2e-6),
    "c51": dict(param="fc_categorical", optimizer="adam", clip=0.5, lr=0.00025, alpha=0.0, eps=0.01 / 32, atol=5e-6, v_min=-10.0,
                v_max=10.0, betas=(0.9, 0.999)),
    "qr": dict(param="fc_quantiles", optimizer="adam", clip=5.0, lr=0.00005, alpha=0.0, eps=0.01 / 32, atol=5e-6, betas=(0.9, 0.999)),
}

# variant bits of include/deeprl_amd.h the path conditions name (deeprl_amd.ops.VAR_*; restated: this module imports no product code)
V_FUSED_BWD, V_ONESHOT_DGRAD, V_ONESHOT_FWD, V_ONESHOT_WGRAD, V_PINNED_IDX = 1, 2, 4, 8, 16
V_ACTOR_PARAMS, V_PIPE_GATHER, V_ACTOR_V3, V_GATHER_IN_GRAPH, V_ACTOR_RING, V_ACTOR_FUSED_CONV1 = 64, 128, 512, 2048, 4096, 8192
V_GATHER_ON_UPDATE, V_RING_DIRECT, V_HEAD_CHAIN, V_LATE_FOLD, V_ACTOR_MEGA = 16384, 32768, 65536, 524288, 1048576
V_DEFER_FC4, V_ACTOR_PERSIST, V_FWD_CHAIN, V_BWD_CHAIN, V_FLAG_SYNC, V_LANE_EAGER = 8388608, 16777216, 33554432, 67108864, 134217728, 268435456
V_TARGET_AHEAD, V_BWD_CHAIN_FC = 536870912, 1073741824
CHAIN_BITS = V_FWD_CHAIN | V_BWD_CHAIN | V_BWD_CHAIN_FC | V_HEAD_CHAIN | V_DEFER_FC4 | V_TARGET_AHEAD


def _case(name, batch, actions, head="vanilla", atoms=0, double_q=False, idx_seed=77, reaches=None, actor=False, updates=4, why=""):
    return dict(name=name, B=batch, A=actions, head=head, atoms=atoms, double_q=double_q, idx_seed=idx_seed, reaches=reaches or {},
                actor=actor, updates=updates, why=why, n_out=actions * (atoms if head != "vanilla" else 1))


# ---- the in-order path: DQNLearner.update(idx): capture + two replays + one eager update, at variant 0 and at the library default.
# `reaches`: the path flags (DQNLearner.path_flags(), at the library default) the case is named for.  idx_seed: chosen by
# tests/test_learner_edge_cases_host.py's rules (first update unambiguous, terminal and non-terminal rows, the actions wanted).
IN_ORDER_CASES = [
    # batches, 4 actions, VanillaNet
    _case("batch1-one-sample", 1, 4, idx_seed=60, reaches=dict(late=True, fchain=False, defer=False, head_pf=False)),
    _case("batch5-odd-below-every-switch", 5, 4, idx_seed=60, reaches=dict(late=True, fchain=False, head_pf=False)),
    _case("batch16-last-small-conv-shape", 16, 4, idx_seed=62, reaches=dict(fchain=False, bchain=False, defer=False, head_pf=True)),
    _case("batch17-first-chained-batch", 17, 4, idx_seed=64, reaches=dict(fchain=True, bchain=True, defer=True, fs=True, head_pf=False)),
    _case("batch24-w4-prefetch-on", 24, 4, idx_seed=60, reaches=dict(fchain=True, head_pf=True)),
    _case("batch31-head-wgrad-remainder", 31, 4, idx_seed=93, reaches=dict(fchain=True, bchain=True, late=True, head_pf=False)),
    _case("batch33-late-fold-off", 33, 4, idx_seed=128, reaches=dict(late=False, fchain=False, bchain=False, defer=False, head_pf=False)),
    _case("batch40-norm-then-step", 40, 4, idx_seed=121, reaches=dict(late=False, head_pf=False)),
    _case("batch128-throughput-shape", 128, 4, idx_seed=103, reaches=dict(late=False, defer=False), updates=3,
          why="three updates (capture + two replays): the eager fourth is dropped to keep the case to a few seconds"),
    # actions, batch 17, VanillaNet (two networks: the head's weights stay in registers while 2 A <= 16)
    _case("actions1", 17, 1, idx_seed=72, actor=True),
    _case("actions3", 17, 3, idx_seed=69),
    _case("actions8-head-weights-in-registers", 17, 8, idx_seed=68),
    _case("actions9-head-fallback-loop", 17, 9, idx_seed=60, actor=True),
    _case("actions18", 17, 18, idx_seed=62, actor=True),
    _case("actions64-last-that-fits", 17, 64, idx_seed=73, actor=True),
    # double-Q (three networks: the switch is at 3 A <= 16)
    _case("double-q-actions5-head-weights-in-registers", 17, 5, idx_seed=62, double_q=True, reaches=dict(fchain=False, bchain=False, defer=False)),
    _case("double-q-actions6-head-fallback-loop", 17, 6, idx_seed=60, double_q=True, reaches=dict(fchain=False)),
    _case("double-q-batch32-actions64", 32, 64, idx_seed=114, double_q=True, reaches=dict(fchain=False, late=True, head_pf=True)),
    _case("double-q-batch5-actions18", 5, 18, idx_seed=61, double_q=True),
    # categorical head (Adam)
    _case("c51-batch5-actions3", 5, 3, "c51", 51, idx_seed=61, reaches=dict(late=True, fchain=False, defer=False)),
    _case("c51-batch17-actions18", 17, 18, "c51", 51, idx_seed=60, reaches=dict(late=True, fchain=False, defer=False)),
    _case("c51-batch32-actions64-atoms64-n-out-limit", 32, 64, "c51", 64, idx_seed=111, reaches=dict(late=False), actor=True,
          why="n_out = 4096 = kMaxHeadOut; 2 x 4096 head partials do not fit the late fold's 4096"),
    _case("c51-batch7-two-atoms", 7, 4, "c51", 2, idx_seed=61),
    _case("c51-double-q-batch17-actions6", 17, 6, "c51", 51, idx_seed=63, double_q=True),
    # quantile head (Adam; the loss vector has one entry per target quantile)
    _case("qr-batch7-atoms200-more-than-batch", 7, 6, "qr", 200, idx_seed=70, reaches=dict(late=True)),
    _case("qr-batch40-atoms8-fewer-than-batch", 40, 2, "qr", 8, idx_seed=69, reaches=dict(late=False)),
    _case("qr-batch3-actions20-atoms200-n-out-4000", 3, 20, "qr", 200, idx_seed=71, reaches=dict(late=False), actor=True),
]
BATCH_CASES = [c for c in IN_ORDER_CASES if c["name"].startswith("batch")]
ACTION_CASES = [c for c in IN_ORDER_CASES if c["name"].startswith("actions")]
DOUBLE_Q_CASES = [c for c in IN_ORDER_CASES if c["double_q"]]

# ---- the pipelined path: DQNLearnerBench(batch, n_actions, actor=True, async_actor=True), 8 agent steps on a CAP-slot ring.
# seed: the bench's (ring contents, actor randomness); draw_seed: the global np.random stream of the minibatch draws.
PIPE_STEPS = 8


def _pipe(name, batch, actions, seed=3, draw_seed=5, reaches=None):
    c = _case(name, batch, actions, reaches=reaches, updates=PIPE_STEPS)
    c.update(seed=seed, draw_seed=draw_seed, chained=16 < batch <= 32)
    return c


PIPELINED_CASES = [
    _pipe("pipe-batch17-first-chained-batch", 17, 4, draw_seed=13, reaches=dict(fchain=True, bchain=True, defer=True, fs=True)),
    _pipe("pipe-batch24-w4-prefetch-on", 24, 4, draw_seed=26, reaches=dict(fchain=True, bchain=True, defer=True, fs=True, head_pf=True)),
    _pipe("pipe-batch31-head-wgrad-remainder", 31, 4, draw_seed=23, reaches=dict(fchain=True, bchain=True, defer=True, fs=True, head_pf=False)),
    _pipe("pipe-batch32-actions1", 32, 1, draw_seed=45, reaches=dict(fchain=True, bchain=True, fs=True)),
    _pipe("pipe-batch32-actions9-head-fallback-loop", 32, 9, draw_seed=187, reaches=dict(fchain=True, bchain=True, fs=True)),
    _pipe("pipe-batch32-actions18", 32, 18, draw_seed=163, reaches=dict(fchain=True, bchain=True, fs=True)),
    _pipe("pipe-batch17-actions64", 17, 64, draw_seed=7, reaches=dict(fchain=True, bchain=True, fs=True)),
    _pipe("pipe-batch33-outside-every-chain", 33, 4, draw_seed=120, reaches=dict(fchain=False, bchain=False, fs=False, late=False, defer=False)),
]


def schedule_oracle(c, params, dtype=torch.float64):
    """oracle.async_schedule_oracle.AsyncDqnScheduleOracle for a pipelined case: its ring, minibatch draws and actor steps (the
    updates are reference_update's).  The prefilled ring's masks are DONE_PERIOD's (the bench's environment keeps its own 800 for
    the transitions the actor adds): frames, actions and rewards do not depend on the period."""
    from oracle.async_schedule_oracle import AsyncDqnScheduleOracle
    orc = AsyncDqnScheduleOracle(params, params, CAP, c["B"], c["seed"], n_actions=c["A"], epsilon=0.01, dtype=dtype)
    orc.rep.mask[:] = synth_transitions(0, CAP, 7056, seed=c["seed"], n_actions=c["A"], done_period=DONE_PERIOD)[3]
    return orc


def by_name(name):
    for c in IN_ORDER_CASES + PIPELINED_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


# ---- the path conditions of dra_dqn_learner_create / run_body, restated as a table --------------------------------------------
LATE_PARTIALS_MAX = 4096                                    # dra_norm_partials_max
LATE_PARTIALS_OTHER = (16 * 13, 145 + 129, 256)             # fc4's weight-gradient workgroups, conv3 + conv2 folds, conv1's fold (at most)


def late_partials(c):
    """(at least, at most) sums of squares the late fold reduces: 2 per head output + the rest."""
    return 2 * c["n_out"] + 1, 2 * c["n_out"] + sum(LATE_PARTIALS_OTHER)


def expected_flags(c, variant, pipelined=False):
    """What DQNLearner.path_flags() must report for case `c` on a learner created with the DRA_VAR_* mask `variant`:
    the conditions of csrc/learner.hip, one line each.  pipelined: after steps of the async pipeline (ring-direct updates);
    otherwise after in-order update() calls (gathered minibatch: no chained launch carries it)."""
    b, vanilla, dq = c["B"], c["head"] == "vanilla", c["double_q"] and c["head"] != "qr"
    has = lambda bits: (variant & bits) == bits
    ring_direct = has(V_RING_DIRECT | V_ONESHOT_WGRAD | V_GATHER_ON_UPDATE | V_PINNED_IDX)
    lo, hi = late_partials(c)
    assert hi <= LATE_PARTIALS_MAX or lo > LATE_PARTIALS_MAX, "the table cannot tell whether %s folds late" % c["name"]
    # the one-pass weight gradients write one slab per sample: conv2 / conv3 fold late up to 32 slabs
    late = has(V_LATE_FOLD | V_ONESHOT_WGRAD | V_ONESHOT_DGRAD | V_FUSED_BWD) and b <= 32 and hi <= LATE_PARTIALS_MAX
    actor_ring = V_RING_DIRECT | V_GATHER_ON_UPDATE | V_ACTOR_PARAMS | V_ACTOR_RING | V_ACTOR_FUSED_CONV1 | V_ACTOR_MEGA
    defer = (has(V_DEFER_FC4 | actor_ring | V_ONESHOT_FWD) and ring_direct and late and vanilla and HEADS[c["head"]]["optimizer"] == "rmsprop"
             and not dq and 16 < b < 128)
    fchain = has(V_FWD_CHAIN) and ring_direct and vanilla and not dq and 16 < b <= 32
    bchain = has(V_BWD_CHAIN) and ring_direct and late and vanilla and not dq and 16 < b <= 32
    fs = (has(V_FLAG_SYNC | actor_ring | V_PIPE_GATHER | V_ACTOR_PERSIST) and fchain and vanilla
          and not variant & (V_GATHER_IN_GRAPH | V_ACTOR_V3))
    ah = has(V_TARGET_AHEAD | V_LANE_EAGER | V_ONESHOT_FWD) and fs and bchain and not dq and b <= 32
    # the last VanillaNet head launch: chained only in the ring-direct pipeline's forward chain; two networks split fc4's K 14 ways
    head_chain = (pipelined and has(V_HEAD_CHAIN | V_ONESHOT_DGRAD | V_ONESHOT_FWD) and fchain and b <= 32 and not dq and late
                  and not variant & V_BWD_CHAIN_FC)
    head_pf = vanilla and has(V_ONESHOT_DGRAD) and b % 8 == 0 and b <= 32 and not head_chain
    return dict(late=late, defer=defer, fchain=fchain, bchain=bchain, fs=fs, ah=ah, per2_ride=False, head_chain=head_chain, head_pf=head_pf)


def head_weights_in_registers(c):
    """head_fused_body keeps the head's weights in registers while nz * A <= 16 (nz networks: 2, 3 with double-Q)."""
    return (3 if c["double_q"] else 2) * c["A"] <= 16


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def head_shapes(c):
    h = HEADS[c["head"]]["param"]
    return fake_envs.NATURE_SHAPES + [(h + ".weight", (c["n_out"], 512)), (h + ".bias", (c["n_out"],))]


def initial_state(c):
    """{'params', 'target', 'state1', 'state2'} -> {name: float32 array}: "normal" initialisation, zero optimizer state."""
    p = fake_envs.numpy_params(head_shapes(c), PARAM_SEEDS[0])
    t = fake_envs.numpy_params(head_shapes(c), PARAM_SEEDS[1])
    return dict(params=p, target=t, state1={k: np.zeros_like(v) for k, v in p.items()}, state2={k: np.zeros_like(v) for k, v in p.items()})


@functools.lru_cache(maxsize=None)
def ring_oracle(n_actions, seed=RING_SEED, done_period=DONE_PERIOD, cap=CAP):
    """The CAP-slot ring dra_ring_fill_synthetic(0, CAP, 0, seed, n_actions, done_period) leaves, as the replay oracle."""
    frames, act, rew, msk = synth_transitions(0, cap, 7056, seed=seed, n_actions=n_actions, done_period=done_period)
    orc = UniformReplayOracle(cap, 1, 1, GAMMA, 4)
    for t in range(cap):
        orc.feed_one(frames[t].reshape(84, 84), act[t], rew[t], msk[t])
    return orc


def case_indices(c):
    """The minibatch indices of the case's updates: UniformReplay.sample's rejection loop (replay.py:92-110) on a private seed."""
    keep = np.random.get_state()
    try:
        np.random.seed(c["idx_seed"])
        return [draw_uniform_indices(CAP, 0, c["B"], 4, 1) for _ in range(c["updates"])]
    finally:
        np.random.set_state(keep)


def gather(c, idx):
    """(state, action, reward, next_state, mask) of the minibatch, as UniformReplayOracle.gather returns them."""
    return ring_oracle(c["A"]).gather(idx)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _f32(x):
    return float(np.float32(x))


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


def _as_quantile_keys(c, p):
    """The head's parameters under QuantileNet's names: net_oracle.quantile_head is `linear, view [B, A, N]` -- the raw outputs
    (logits) of the categorical head too."""
    h = HEADS[c["head"]]["param"]
    return {"fc_quantiles.weight": p[h + ".weight"], "fc_quantiles.bias": p[h + ".bias"]}


def action_values(c, p, phi):
    """What the actor takes the argmax of (AsyncDqnScheduleOracle._action_values)."""
    if c["head"] == "c51":
        h = HEADS["c51"]
        atoms = torch.tensor(np.linspace(h["v_min"], h["v_max"], c["atoms"]), dtype=torch.float32).to(phi.dtype)
        return (N.categorical_head(p, phi, c["A"], c["atoms"])[0] * atoms).sum(-1)
    if c["head"] == "qr":
        return N.quantile_head(p, phi, c["A"], c["atoms"]).mean(-1)
    return N.vanilla_head(p, phi)


def reference_actor_q(c, params, stack, dtype=torch.float64):
    """Action values of ONE uint8 [4, 84, 84] observation on `params` ({name: float32 array})."""
    p = {k: _t(v, dtype) for k, v in params.items()}
    with torch.no_grad():
        return action_values(c, p, N.nature_conv_body(p, _t(NUM.image_normalize_sync(stack[None]), dtype))).numpy()[0].astype(np.float64)


def reference_update(c, state, batch, opt_step, dtype=torch.float64):
    """One update of DQN_agent.py:101-134 (CategoricalDQN_agent.py / QuantileRegressionDQN_agent.py for their heads) in `dtype`
    from the float32 `state` ({'params', 'target', 'state1', 'state2'} -> {name: array}) on the minibatch `batch` (gather());
    opt_step: Adam's 1-based step count.  Returns float64 arrays: out (q / logits / quantiles), vec (TD errors / loss vector),
    loss, norm, margin, grads (before the clip), params / state1 / state2 after the step (RMSprop: square_avg, grad_avg; Adam:
    exp_avg, exp_avg_sq)."""
    h = HEADS[c["head"]]
    st, ac, rw, ns, mk = batch
    p = {k: _t(v, dtype).requires_grad_(True) for k, v in state["params"].items()}
    pt = {k: _t(v, dtype) for k, v in state["target"].items()}
    names = list(p)
    x, xn = _t(NUM.image_normalize_sync(st), dtype), _t(NUM.image_normalize_sync(ns), dtype)
    a_t, r_t, m_t, gamma = torch.from_numpy(np.asarray(ac, dtype=np.int64)), _t(rw, dtype), _t(mk, dtype), _f32(GAMMA)
    A, n = c["A"], c["atoms"]
    phi, margin = N.nature_conv_body_margin(p, x)
    with torch.no_grad():
        phi_t = N.nature_conv_body(pt, xn)
        phi_o = N.nature_conv_body(p, xn) if (c["double_q"] and c["head"] != "qr") else None     # (QR: the target network only)
    if c["head"] == "vanilla":
        out = N.vanilla_head(p, phi)
        with torch.no_grad():
            qn = N.vanilla_head(pt, phi_t)
            qno = N.vanilla_head(p, phi_o) if phi_o is not None else None
        vec = L.dqn_td_error(out, qn, a_t, r_t, m_t, gamma, q_next_online=qno)
        loss = L.dqn_reduce(vec)
    elif c["head"] == "c51":
        atoms = torch.tensor(np.linspace(h["v_min"], h["v_max"], n), dtype=torch.float32).to(dtype)     # CategoricalDQN_agent.py:33
        out = N.quantile_head(_as_quantile_keys(c, p), phi, A, n)                                        # the logits
        _, log_prob = N.categorical_head(p, phi, A, n)
        with torch.no_grad():
            prob_t = N.categorical_head(pt, phi_t, A, n)[0]
            prob_o = N.categorical_head(p, phi_o, A, n)[0] if phi_o is not None else None
        vec = L.c51_kl(log_prob, prob_t, a_t, r_t, m_t, gamma, atoms, _f32(h["v_min"]), _f32(h["v_max"]), prob_next_online=prob_o)
        loss = vec.mean()
    else:
        out = N.quantile_head(p, phi, A, n)
        with torch.no_grad():
            qn = N.quantile_head(pt, phi_t, A, n)
        vec = L.qr_loss(out, qn, a_t, r_t, m_t, gamma)
        loss = vec.mean()
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    norm = torch.sqrt(sum((g * g).sum() for g in grads))
    coef = _f32(h["clip"]) / (norm + _f32(1e-6))                     # torch.nn.utils.clip_grad_norm_ (DQN_agent.py:132)
    clipped = [g * coef for g in grads] if float(coef) < 1 else list(grads)
    new_p, s1, s2 = {}, {}, {}
    with torch.no_grad():
        for k, g in zip(names, clipped):
            a, b = _t(state["state1"][k], dtype), _t(state["state2"][k], dtype)
            if h["optimizer"] == "rmsprop":
                new_p[k], s1[k], s2[k] = N.rmsprop_step(p[k], g, a, b, _f32(h["lr"]), _f32(h["alpha"]), _f32(h["eps"]), True)
            else:
                new_p[k], s1[k], s2[k] = N.adam_step(p[k], g, a, b, opt_step, _f32(h["lr"]), _f32(h["betas"][0]), _f32(h["betas"][1]),
                                                     _f32(h["eps"]))
    d = lambda v: v.detach().numpy().astype(np.float64)
    return dict(out=d(out), vec=d(vec), loss=float(loss.detach()), norm=float(norm), margin=float(margin), clipped=float(coef) < 1,
                grads={k: d(g) for k, g in zip(names, grads)}, params={k: d(v) for k, v in new_p.items()},
                state1={k: d(v) for k, v in s1.items()}, state2={k: d(v) for k, v in s2.items()})


def next_state(state, ref):
    """The float32 state an implementation holds after the update `ref` describes."""
    f = lambda d_: {k: v.astype(np.float32) for k, v in d_.items()}
    return dict(params=f(ref["params"]), target=state["target"], state1=f(ref["state1"]), state2=f(ref["state2"]))


@functools.lru_cache(maxsize=None)
def first_update(name, wide=True):
    """The case's first update (initial parameters, zero optimizer state) in float64, or in float32 on the CPU."""
    c = by_name(name)
    return reference_update(c, initial_state(c), gather(c, case_indices(c)[0]), 1, torch.float64 if wide else torch.float32)


# ---- the bar ---------------------------------------------------------------------------------------------------------------
def _scaled(got, want):
    """max |got - want| / max |want| (0 / 0 = 0: where float64 says a tensor is exactly zero, so must the kernel)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    if not np.isfinite(err):
        return float("inf")
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def measure(c, got, want, with_state):
    """error / scale of every compared tensor -> {key: figure}; 'params:*' in units of its bar (atol + rtol |want|)."""
    atol = HEADS[c["head"]]["atol"]
    out = dict(out=_scaled(got["out"], want["out"]), vec=_scaled(got["vec"], want["vec"]),
               loss=abs(got["loss"] - want["loss"]) / abs(want["loss"]), norm=abs(got["norm"] - want["norm"]) / want["norm"])
    for k, w in want["params"].items():
        g = np.asarray(got["params"][k], dtype=np.float64)
        out["params:" + k] = float((np.abs(g - w) / (atol + BAR * np.abs(w))).max()) * BAR      # (x BAR: the bar of every key is BAR)
    if with_state:
        for which in ("state1", "state2"):
            for k, w in want[which].items():
                out[which + ":" + k] = _scaled(got[which][k], w)
    for k, g in (got.get("grads") or {}).items():
        out["grad:" + k] = _scaled(g, want["grads"][k])
    return out


def judge(c, figures, ambiguous, what):
    """Every figure of measure() against its bar (BAR, BAR_OVERRIDES; x 100 for an ambiguous update)."""
    f = AMBIGUOUS_FACTOR if ambiguous else 1.0
    bad = {k: v for k, v in figures.items() if not v <= f * BAR_OVERRIDES.get((c["name"], k), (BAR,))[0]}
    assert not bad, "%s, %s%s: beyond the bar (error / scale, bar %g): %s" % (c["name"], what, " (ambiguous ReLU gate: x100)" if ambiguous else "",
                                                                             f * BAR, {k: "%.3g" % v for k, v in bad.items()})
