"""Restatement of what dra_dqn_replay_mlp_update (csrc/dqn_mlp.hip) and DQNAgent's cart-pole device path under
config.fused_dqn_replay_feature compute (TEST INFRASTRUCTURE ONLY): dqn_feature_restatement's acting loop and network over the
n-step minibatch (replay.py:112-140: the fold, the masks' AND, next state = frame idx + n_step), one update with optional
priorities and importance weights (DQN_agent.py:81-99, 120-129) and the agent step with the prioritised replay's bookkeeping
(rainbow_feature_restatement's SumTree and per_draw: utils/sum_tree.py, replay.py:160-196).  fp64 by default; dtype=torch.float32
runs the same arithmetic in fp32 (the margin tests).  tests/test_dqn_replay_feature_host.py pins it to the reference's own run and
replay (tests/golden/dqn_replay_feature/) before a GPU test leans on it."""
import numpy as np
import torch

from dqn_feature_restatement import KEYS, F64, act, forward, init_params, new_ring, rmsprop_step, to_t      # noqa: F401
from rainbow_feature_restatement import SumTree, per_draw      # noqa: F401


def fold(rewards, masks, i, n_step, discount):
    """replay.py:135-139 at data index i -> (the folded reward: a python float, fp64; the AND of the window's masks)."""
    cum_r, cum_mask = 0, 1
    for s in reversed(range(n_step)):
        cum_r = float(rewards[i + s]) + int(masks[i + s]) * discount * cum_r
        cum_mask = cum_mask and int(masks[i + s])
    return cum_r, cum_mask


def minibatch(ring, idx, n_step, discount):
    """What tensor() hands the networks at the DATA indices idx: float32 states (frame idx), next states (frame idx + n_step), the
    folded rewards and the masks' AND narrowed to float32; int64 actions (of row idx)."""
    idx = np.asarray(idx, dtype=np.int64)
    folded = [fold(ring["rewards"], ring["masks"], int(i), n_step, discount) for i in idx]
    return dict(state=ring["frames"][idx].astype(np.float32), next_state=ring["frames"][idx + n_step].astype(np.float32),
                action=ring["actions"][idx].astype(np.int64),
                reward=np.asarray([f[0] for f in folded], dtype=np.float64).astype(np.float32),
                mask=np.asarray([f[1] for f in folded]).astype(np.float32))


def valid_index(index, pos, size, n_step):
    """replay.py:105-110 with history_length 1."""
    return (index >= 0 and index + n_step < pos) or (index >= pos and index + n_step < size)


def draw_indices(rs, batch, pos, size, n_step):
    """replay.py:92-103's rejection loop on the RandomState `rs`: one randint(0, size) per attempt."""
    out = []
    while len(out) < batch:
        i = int(rs.randint(0, size))
        if valid_index(i, pos, size, n_step):
            out.append(i)
    return np.asarray(out, dtype=np.int64)


def loss_and_grads(params, target, batch, bootstrap, double_q=False, gate="relu", prob=None, beta=None, replay_eps=0.01,
                   replay_alpha=0.5, dtype=F64):
    """DQN_agent.py:81-99, 120-129 on a minibatch; bootstrap = discount ** n_step.  prob None: the uniform replay's update (no
    weights, no priorities).  -> dict(q_target [B], td = q_target - q_a [B] (UNWEIGHTED), loss = 0.5 mean (td w)^2, prio = (|td| +
    eps) ** alpha and weights = (prob B + 1e-6) ** -beta / their maximum (None without prob), grads by name, min_preact,
    argmax_margin, best)."""
    p, pt = to_t(params, dtype, requires_grad=True), to_t(target, dtype)
    keep_t, keep_o, keep = {}, {}, {}
    with torch.no_grad():
        q_next = forward(pt, batch["next_state"], gate, keep_t)
        q_on = forward(p, batch["next_state"], gate, keep_o)
        best = torch.argmax(q_on, dim=-1)
        q_next = q_next.gather(1, best.unsqueeze(-1)).squeeze(1) if double_q else q_next.max(1)[0]
    rewards, masks = torch.as_tensor(batch["reward"], dtype=dtype), torch.as_tensor(batch["mask"], dtype=dtype)
    q_target = rewards + bootstrap * q_next * masks
    q = forward(p, batch["state"], gate, keep)
    q_a = q.gather(1, torch.as_tensor(batch["action"]).unsqueeze(-1)).squeeze(-1)
    td = q_target - q_a
    prio = weights = None
    loss_vec = td
    if prob is not None:
        sp = torch.as_tensor(np.asarray(prob, dtype=np.float32)).to(dtype)
        prio = (td.detach().abs() + replay_eps) ** replay_alpha
        weights = (sp * sp.shape[0] + 1e-6) ** (-float(beta))
        weights = weights / weights.max()
        loss_vec = td * weights
    loss = loss_vec.pow(2).mul(0.5).mean()
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    pre = [keep_t, keep] + ([keep_o] if double_q else [])
    return dict(q_target=q_target.detach().numpy(), td=td.detach().numpy(), loss=float(loss.detach()),
                prio=None if prio is None else prio.numpy(), weights=None if weights is None else weights.numpy(),
                grads={k: g.numpy() for k, g in zip(names, grads)},
                min_preact=float(min(min(np.abs(d["z1"].numpy()).min(), np.abs(d["z2"].numpy()).min()) for d in pre)),
                argmax_margin=float((q_on[:, 1] - q_on[:, 0]).abs().min()), best=best.numpy())


def leaf_margin(tree, u, data_capacity):
    """The distance of the uniform u from the nearest boundary between two leaves' intervals, as a fraction of the tree's total:
    the descent (s <= left goes left) lands on the same leaf in fp32 and fp64 arithmetic while this is large."""
    leaves = tree.tree[data_capacity - 1:]
    edges = np.cumsum(leaves)
    total = float(tree.total())
    inner = edges[:-1][(leaves[:-1] > 0) | (leaves[1:] > 0)]
    return float(np.min(np.abs(inner - u))) / total if inner.size else 1.0


class _MarginRandom:
    """python's random with the margin of every uniform() against the tree it is drawn for recorded."""

    def __init__(self, rnd):
        self.rnd, self.tree, self.capacity, self.margin = rnd, None, 0, float("inf")

    def uniform(self, a, b):
        u = self.rnd.uniform(a, b)
        self.margin = min(self.margin, leaf_margin(self.tree, u, self.capacity))
        return u

    def choice(self, seq):
        return self.rnd.choice(seq)


def agent_run(init, env, cfg, rs, eps, rnd, n_steps, dtype=F64, target0=None):
    """n_steps DQNAgent.step()s in the reference's order: dqn_feature_restatement.agent_run with an n-step window and, for cfg["per"],
    the prioritised replay -- the feed's tree add at max_priority per transition; past exploration_steps the prioritised draw
    (`rnd`: python's random), beta (one schedule call per update), the update, the priorities' commit with max_priority.  cfg:
    dict(k, batch, capacity, exploration_steps, target_freq, discount, n_step, gradient_clip, lr, double_q, gate, per, beta =
    (start, end, steps), replay_eps, replay_alpha).  -> dict(actions [n_steps, K], flags, random_actions, slots, updates (per step
    None or dict(data, td, prio, loss, window_terminal and for per: drawn, leaves, prob, padded, total, beta)), params (per step,
    after it), target, ring, events, copies, margin, argmax_margin, leaf_margin, min_preact, pos, size, total and for per: tree,
    pending, max_priority, beta (the schedule's position))."""
    params = {k: np.asarray(v, dtype=np.float64).copy() for k, v in init.items()}
    target = {k: np.asarray(v, dtype=np.float64).copy() for k, v in (target0 or params).items()}
    cap, k_len, n_step, per = cfg["capacity"], cfg["k"], cfg["n_step"], bool(cfg["per"])
    ring, tree = new_ring(cap), SumTree(cap)
    rnd = _MarginRandom(rnd)
    rnd.tree, rnd.capacity = tree, cap
    raw = env.reset()
    pos = size = total = actor_steps = 0
    max_priority, sq = 1.0, None
    b0, b1, bsteps = cfg.get("beta", (0.4, 1.0, 1e5))
    beta, beta_inc = b0, (b1 - b0) / float(bsteps)
    out = dict(actions=[], flags=[], random_actions=[], slots=[], updates=[], events=[], params=[], copies=[],
               margin=float("inf"), argmax_margin=float("inf"), min_preact=float("inf"))
    for step in range(n_steps):
        explore, rand = np.empty(k_len, dtype=bool), np.empty(k_len, dtype=np.int64)
        for k in range(k_len):
            e = 1 if actor_steps < cfg["exploration_steps"] else eps()
            rand[k] = rs.randint(2, size=1)[0]
            explore[k] = rs.rand(1)[0] < e
            actor_steps += 1
        a = act(params, env, raw, k_len, explore, rand, ring, pos, gate=cfg["gate"], step0=total, dtype=dtype)
        raw = a["raw"]
        out["slots"].append(pos)
        for _ in range(k_len):
            if pos >= size:
                size += 1
            pos = (pos + 1) % cap
            if per:
                tree.add(max_priority)
        total += k_len
        u = None
        if total > cfg["exploration_steps"]:
            u = {}
            prob = this_beta = None
            if per:
                u["total"] = float(tree.total())
                u["drawn"], u["leaves"], prob, data, u["padded"] = per_draw(tree, rnd, cfg["batch"], pos, size, n_step)
                this_beta, beta = beta, min(beta + beta_inc, b1)
                u.update(prob=prob, beta=this_beta)
            else:
                data = draw_indices(rs, cfg["batch"], pos, size, n_step)
            mb = minibatch(ring, data, n_step, cfg["discount"])
            g = loss_and_grads(params, target, mb, cfg["discount"] ** n_step, cfg["double_q"], cfg["gate"], prob, this_beta,
                               cfg.get("replay_eps", 0.01), cfg.get("replay_alpha", 0.5), dtype)
            if per:
                for leaf, p in zip(u["leaves"], g["prio"]):
                    max_priority = max(max_priority, float(p))
                    tree.update(int(leaf), float(p))
            params, sq = rmsprop_step(params, g["grads"], cfg["gradient_clip"], cfg["lr"], square_avg=sq)
            out["min_preact"] = min(out["min_preact"], g["min_preact"])
            if cfg["double_q"]:
                out["argmax_margin"] = min(out["argmax_margin"], g["argmax_margin"])
            u.update(data=data, td=g["td"], prio=g["prio"], loss=g["loss"], window_terminal=bool((mb["mask"] == 0).any()))
        if total / k_len % cfg["target_freq"] == 0:
            target = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
            out["copies"].append(step)
        out["actions"].append(a["action"]); out["flags"].append(explore); out["random_actions"].append(rand)
        out["updates"].append(u); out["events"] += a["events"]
        out["params"].append({k: np.asarray(v).copy() for k, v in params.items()})
        out["margin"] = min(out["margin"], a["margin"])
    out.update(ring=ring, target=target, pos=pos, size=size, total=total, actions=np.stack(out["actions"]),
               flags=np.stack(out["flags"]), random_actions=np.stack(out["random_actions"]), leaf_margin=rnd.margin)
    if per:
        out.update(tree=tree.tree.copy(), pending=sorted(tree.pending), max_priority=max_priority, beta=beta)
    return out
