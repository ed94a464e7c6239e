"""Restatement of what csrc/rainbow_mlp.hip computes (TEST INFRASTRUCTURE ONLY): RainbowNet over a two-layer noisy FCBody
(network_heads.py:57-86, network_utils.py:31-83: W = mu_w + sigma_w * (f(out) (x) f(in)), b = mu_b + sigma_b * f(out_b), f(x) =
sign(x) sqrt|x|, all from the RAW noise vectors), the dueling combination, the action values (CategoricalDQN_agent.py:22-24), the
acting loop with one noise row per transition (DQN_agent.py:24-45) over envs.CartPole, which is imported, not restated, the n-step
minibatch (replay.py:112-140) and the prioritised update (CategoricalDQN_agent.py:60-89 through oracle/loss_oracle.py's c51_kl,
DQN_agent.py:120-129) with autograd's gradients of all sixteen tensors.  fp64 by default; dtype=torch.float32 runs the same
arithmetic in fp32 (the margin tests).  tests/test_rainbow_feature_host.py pins the network to the reference's own RainbowNet
(tests/golden/rainbow_feature/modules.npz) before a GPU test leans on it.

Parameters and noise are dicts keyed like the network's state_dict()."""
import os
import sys

import numpy as np
import torch

from dqn_feature_restatement import new_ring      # noqa: F401
from nstep_feature_restatement import to_t

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import loss_oracle as L      # noqa: E402

F64 = torch.float64
_GATES = {"relu": torch.relu, "tanh": torch.tanh}
LAYERS = ("body.layers.0", "body.layers.1", "fc_value", "fc_advantage")      # the net struct's order
DRAW_ORDER = ("fc_value", "fc_advantage", "body.layers.0", "body.layers.1")  # reset_noise()'s (network_heads.py:73-77)
PARAMS = ("weight_mu", "weight_sigma", "bias_mu", "bias_sigma")
NOISE = ("noise_in", "noise_out_weight", "noise_out_bias")
KEYS = tuple("%s.%s" % (l, p) for l in LAYERS for p in PARAMS)
NOISE_KEYS = tuple("%s.%s" % (l, b) for l in DRAW_ORDER for b in NOISE)


def dims(hidden, n, state_dim=4, n_actions=2):
    """{layer: (out, in)}"""
    return {"body.layers.0": (hidden, state_dim), "body.layers.1": (hidden, hidden), "fc_value": (n, hidden),
            "fc_advantage": (n_actions * n, hidden)}


def init_params(hidden, seed, n, head_scale=0.3):
    """float32 numpy parameters: means of O(0.3), sigmas spread over [0.5, 2] x the layers' initial constant and of both signs."""
    rs = np.random.RandomState(seed)
    out = {}
    for layer, (o, i) in dims(hidden, n).items():
        scale = {"body.layers.0": 0.8, "body.layers.1": 0.25}.get(layer, head_scale)
        out[layer + ".weight_mu"] = (rs.randn(o, i) * scale).astype(np.float32)
        out[layer + ".weight_sigma"] = (rs.uniform(0.5, 2.0, (o, i)) * rs.choice([-1, 1], (o, i)) * 0.4 / np.sqrt(i)).astype(np.float32)
        out[layer + ".bias_mu"] = (rs.randn(o) * 0.1).astype(np.float32)
        out[layer + ".bias_sigma"] = (rs.uniform(0.5, 2.0, o) * rs.choice([-1, 1], o) * 0.4 / np.sqrt(o)).astype(np.float32)
    return out


def draw_noise(hidden, n, seed, std=1.0):
    """The twelve raw noise vectors (float32) of one reset_noise(): normal draws of scale `std` (the entry's is Config.NOISY_LAYER_STD; the
    kernel cases take 1.0 so that the noisy part of every weight is of the mean's size), with one exact 0 and both signs."""
    rs = np.random.RandomState(seed)
    out = {}
    for layer in DRAW_ORDER:
        o, i = dims(hidden, n)[layer]
        for b, size in zip(NOISE, (i, o, o)):
            out["%s.%s" % (layer, b)] = (rs.randn(size) * std).astype(np.float32)
    out["body.layers.1.noise_in"][0] = 0.0
    return out


def noise_f(x):
    return x.sign() * x.abs().sqrt()


def effective(p, z, layer):
    """(W, b) of a noisy layer under the raw noise z (tensors of one dtype)."""
    eps_w = torch.outer(noise_f(z[layer + ".noise_out_weight"]), noise_f(z[layer + ".noise_in"]))
    w = p[layer + ".weight_mu"] + p[layer + ".weight_sigma"] * eps_w
    b = p[layer + ".bias_mu"] + p[layer + ".bias_sigma"] * noise_f(z[layer + ".noise_out_bias"])
    return w, b


def logits(p, z, obs, n, gate="relu", keep=None):
    """The dueling logits [rows, A, N] in the dtype of the parameters; `keep` receives the pre-activations."""
    lin = torch.nn.functional.linear
    dt = p[KEYS[0]].dtype
    g = _GATES[gate]
    x = torch.as_tensor(np.asarray(obs), dtype=dt)
    z1 = lin(x, *effective(p, z, "body.layers.0"))
    z2 = lin(g(z1), *effective(p, z, "body.layers.1"))
    if keep is not None:
        keep["z1"], keep["z2"] = z1.detach(), z2.detach()
    phi = g(z2)
    value = lin(phi, *effective(p, z, "fc_value")).view(-1, 1, n)
    adv = lin(phi, *effective(p, z, "fc_advantage")).view(x.shape[0], -1, n)
    return value + (adv - adv.mean(1, keepdim=True))


def atoms(spec):
    """tensor(np.linspace(v_min, v_max, n)): float32 values."""
    return np.linspace(spec["v_min"], spec["v_max"], spec["n"]).astype(np.float32)


def action_values(out, spec):
    zt = torch.as_tensor(atoms(spec)).to(out.dtype)
    return (torch.softmax(out, dim=-1) * zt).sum(-1)


def forward(p, z, obs, spec, gate="relu", keep=None):
    return action_values(logits(p, z, obs, spec["n"], gate, keep), spec)


def act(params, noise_rows, env, raw, k_len, explore, random_action, ring, slot0, spec, gate="relu", step0=0, reward_coef=1.0,
        dtype=F64):
    """dqn_feature_restatement.act with transition k under noise_rows[k]: q of the float32 observation, action =
    random_action[k] where explore[k] else np.argmax(q), the environment step with the auto reset, the ring row.  -> its dict."""
    p = to_t(params, dtype)
    cap = ring["actions"].shape[0]
    raw = np.asarray(raw, dtype=np.float64).copy()
    qs, acts, events, margin = [], [], [], float("inf")
    with torch.no_grad():
        for k in range(k_len):
            q = forward(p, to_t(noise_rows[k], dtype), raw.astype(np.float32)[None], spec, gate).to(F64).numpy()[0]
            if explore[k]:
                a = int(random_action[k])
            else:
                a = int(np.argmax(q))
                margin = min(margin, float(abs(q[1] - q[0])))
            slot = (slot0 + k) % cap
            ring["frames"][slot] = raw
            s, r, done, info = env.step(a)
            if done:
                events.append((step0 + k, 0, float(info['episodic_return'])))
                s = env.reset()
            ring["actions"][slot], ring["rewards"][slot], ring["masks"][slot] = a, reward_coef * r, 0 if done else 1
            qs.append(q)
            acts.append(a)
            raw = np.asarray(s, dtype=np.float64)
    return dict(q=np.stack(qs), action=np.asarray(acts, dtype=np.int64), events=events, raw=raw, margin=margin)


def minibatch(ring, idx, n_step, discount):
    """replay.py:112-140 with history_length 1 at the DATA indices idx: float32 states (frame idx), next states (frame idx + n),
    the folded reward (python floats: fp64) and the masks' product narrowed to float32; int64 actions."""
    idx = np.asarray(idx, dtype=np.int64)
    rew, msk = [], []
    for i in idx:
        cum_r, cum_mask = 0, 1
        for s in reversed(range(n_step)):
            cum_r = float(ring["rewards"][i + s]) + int(ring["masks"][i + s]) * discount * cum_r
            cum_mask = cum_mask and int(ring["masks"][i + s])
        rew.append(cum_r)
        msk.append(cum_mask)
    return dict(state=ring["frames"][idx].astype(np.float32), next_state=ring["frames"][idx + n_step].astype(np.float32),
                action=ring["actions"][idx].astype(np.int64), reward=np.asarray(rew, dtype=np.float64).astype(np.float32),
                mask=np.asarray(msk).astype(np.float32))


def loss_and_grads(params, target, noise, target_noise, batch, prob, beta, bootstrap, spec, double_q=True, replay_eps=0.01,
                   replay_alpha=0.5, gate="relu", dtype=F64):
    """DQN_agent.py:114-131 with CategoricalDQN_agent.py:60-89 on a minibatch: the target network under target_noise, the online one
    under `noise` -> dict(loss, loss_vec (KL [B]), prio, weights, q_next [B, A] (the TARGET's), target [B, N], a_next, grads by
    name, argmax_margin, min_preact)."""
    n = spec["n"]
    p, pt = to_t(params, dtype, requires_grad=True), to_t(target, dtype)
    z, zt = to_t(noise, dtype), to_t(target_noise, dtype)
    rewards, masks = torch.as_tensor(batch["reward"], dtype=dtype), torch.as_tensor(batch["mask"], dtype=dtype)
    actions = torch.as_tensor(batch["action"])
    keep_t, keep_o, keep = {}, {}, {}
    b = torch.arange(actions.shape[0])
    at = torch.as_tensor(atoms(spec)).to(dtype)
    with torch.no_grad():
        out_t = logits(pt, zt, batch["next_state"], n, gate, keep_t)
        q_next = action_values(out_t, spec)
        q_choice = q_next
        if double_q:
            out_o = logits(p, z, batch["next_state"], n, gate, keep_o)
            q_choice = action_values(out_o, spec)
        a_next = torch.argmax(q_choice, dim=-1)
    out = logits(p, z, batch["state"], n, gate, keep)
    prob_t = torch.softmax(out_t, dim=-1)
    prob_o = torch.softmax(out_o, dim=-1) if double_q else None
    vec = L.c51_kl(torch.log_softmax(out, dim=-1), prob_t, actions, rewards, masks, bootstrap, at, spec["v_min"], spec["v_max"],
                   prob_next_online=prob_o)
    delta = (spec["v_max"] - spec["v_min"]) / float(n - 1)
    tz = (rewards.unsqueeze(-1) + bootstrap * masks.unsqueeze(-1) * at.view(1, -1)).clamp(spec["v_min"], spec["v_max"]).unsqueeze(1)
    tgt = ((1 - (tz - at.view(1, -1, 1)).abs() / delta).clamp(0, 1) * prob_t[b, a_next, :].unsqueeze(1)).sum(-1)
    sp = torch.as_tensor(np.asarray(prob, dtype=np.float32)).to(dtype)
    prio = (vec.detach().abs() + replay_eps) ** replay_alpha
    weights = (sp * sp.shape[0] + 1e-6) ** (-float(beta))
    weights = weights / weights.max()
    loss = (vec * weights).mean()
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    pre = [keep_t, keep] + ([keep_o] if keep_o else [])
    return dict(loss=float(loss.detach()), loss_vec=vec.detach().numpy(), prio=prio.numpy(), weights=weights.numpy(),
                q_next=q_next.numpy(), target=tgt.detach().numpy(), a_next=a_next.numpy(),
                grads={k: g.numpy() for k, g in zip(names, grads)},
                argmax_margin=float((q_choice[:, 1] - q_choice[:, 0]).abs().min()),
                min_preact=float(min(min(np.abs(d["z1"].numpy()).min(), np.abs(d["z2"].numpy()).min()) for d in pre)))


# ------------------------------------------------------------------------------------------ one agent step
class SumTree:
    """utils/sum_tree.py in fp64: add at the write cursor, update gated on the pending set, the descent (s <= left goes left)."""

    def __init__(self, capacity):
        self.capacity, self.tree, self.write, self.pending = capacity, np.zeros(2 * capacity - 1), 0, set()

    def total(self):
        return self.tree[0]

    def add(self, p):
        idx = self.write + self.capacity - 1
        self.pending.add(idx)
        self.update(idx, p)
        self.write = (self.write + 1) % self.capacity

    def update(self, idx, p):
        if idx not in self.pending:
            return
        self.pending.remove(idx)
        change = p - self.tree[idx]
        self.tree[idx] = p
        while idx != 0:
            idx = (idx - 1) // 2
            self.tree[idx] += change

    def get(self, s):
        idx = 0
        while 2 * idx + 1 < len(self.tree):
            left = 2 * idx + 1
            if s <= self.tree[left]:
                idx = left
            else:
                idx, s = left + 1, s - self.tree[left]
        self.pending.add(idx)
        return idx, self.tree[idx], idx - self.capacity + 1


def reset_noise(hidden, n, std):
    """One RainbowNet.reset_noise() (network_heads.py:73-77, network_utils.py:73-76) on torch's global generator: float32 normal
    draws, per layer in DRAW_ORDER noise_in, noise_out_weight, noise_out_bias."""
    out = {}
    for layer in DRAW_ORDER:
        o, i = dims(hidden, n)[layer]
        for b, size in zip(NOISE, (i, o, o)):
            out["%s.%s" % (layer, b)] = torch.zeros(size).normal_(std=std).numpy()
    return out


def per_draw(tree, rnd, batch, pos, size, n_step):
    """replay.py:164-186: one rnd.uniform per segment, the descent, the validity check, the padding through rnd.choice.
    -> (drawn leaves [batch], leaves [batch] after the check and the padding, probabilities, data indices, whether it padded)"""
    segment = tree.total() / batch
    drawn, kept = [], []
    for i in range(batch):
        idx, p, data = tree.get(rnd.uniform(segment * i, segment * (i + 1)))
        drawn.append(idx)
        if (data >= 0 and data + n_step < pos) or (data >= pos and data + n_step < size):
            kept.append((idx, p / tree.total(), data))
    padded = len(kept) < batch
    while len(kept) < batch:
        kept.append(rnd.choice(kept))
    return (np.asarray(drawn, dtype=np.int64), np.asarray([t[0] for t in kept], dtype=np.int64),
            np.asarray([t[1] for t in kept], dtype=np.float64), np.asarray([t[2] for t in kept], dtype=np.int64), padded)


def agent_run(init, env, cfg, rnd, n_steps, target0=None, dtype=F64, noise_fn=None):
    """n_steps CategoricalDQNAgent.step()s on rainbow_feature's kind of configuration in the reference's order (DQN_agent.py:24-45,
    101-138): per transition a reset_noise() (torch's generator), np.random as epsilon_greedy(0, q) consumes it, the greedy action,
    the feed with the tree's add at max_priority; past exploration_steps the prioritised draw (`rnd`: python's random), the
    target's and the online network's reset_noise(), beta, the update (loss_and_grads), the priorities' commit with max_priority,
    clip + RMSprop; the target copy when total_steps / K % freq == 0.  cfg: dict(k, batch, capacity, exploration_steps,
    target_freq, discount, n_step, gradient_clip, lr, double_q, gate, spec, hidden, std, beta = (start, end, steps), replay_eps,
    replay_alpha); noise_fn("online" | "target") -> the raw noise of that network's next reset_noise() (default: reset_noise on
    torch's generator, as the reference draws it).  -> dict(actions, rows (the acting noise per step), updates (per step None or dict(drawn, leaves, prob, data,
    padded, total, beta, noise, target_noise, kl, prio, loss)), params (per step, after it), target, ring, rings (per step),
    tree, pending, max_priority, margin, argmax_margin, events, pos, size, total)."""
    from nstep_feature_restatement import rmsprop_step
    params = {k: np.asarray(v, dtype=np.float64).copy() for k, v in init.items()}
    target = {k: np.asarray(v, dtype=np.float64).copy() for k, v in (target0 or params).items()}
    spec, k_len, cap, n_step = cfg["spec"], cfg["k"], cfg["capacity"], cfg["n_step"]
    noise_fn = noise_fn or (lambda which: reset_noise(cfg["hidden"], spec["n"], cfg["std"]))
    ring, tree = new_ring(cap), SumTree(cap)
    raw = env.reset()
    pos = size = total = 0
    max_priority, sq = 1.0, None
    b0, b1, bsteps = cfg["beta"]
    beta, beta_inc = b0, (b1 - b0) / float(bsteps)
    out = dict(actions=[], rows=[], updates=[], params=[], rings=[], events=[], copies=[], margin=float("inf"),
               argmax_margin=float("inf"), min_preact=float("inf"))
    for step in range(n_steps):
        rows = []
        for _ in range(k_len):
            rows.append(noise_fn("online"))
            np.random.randint(2, size=1)
            np.random.rand(1)
        a = act(params, rows, env, raw, k_len, np.zeros(k_len, dtype=bool), np.zeros(k_len, dtype=np.int64), ring, pos, spec,
                gate=cfg["gate"], step0=total, dtype=dtype)
        raw = a["raw"]
        for _ in range(k_len):
            if pos >= size:
                size += 1
            pos = (pos + 1) % cap
            tree.add(max_priority)
        total += k_len
        u = None
        if total > cfg["exploration_steps"]:
            tree_total = float(tree.total())
            drawn, leaves, prob, data, padded = per_draw(tree, rnd, cfg["batch"], pos, size, n_step)
            tz, z = noise_fn("target"), noise_fn("online")
            this_beta, beta = beta, min(beta + beta_inc, b1)
            mb = minibatch(ring, data, n_step, cfg["discount"])
            g = loss_and_grads(params, target, z, tz, mb, prob, this_beta, cfg["discount"] ** n_step, spec, cfg["double_q"],
                               cfg["replay_eps"], cfg["replay_alpha"], cfg["gate"], dtype)
            for leaf, p in zip(leaves, g["prio"]):
                max_priority = max(max_priority, float(p))
                tree.update(int(leaf), float(p))
            params, sq = rmsprop_step(params, g["grads"], cfg["gradient_clip"], cfg["lr"], square_avg=sq)
            out["argmax_margin"] = min(out["argmax_margin"], g["argmax_margin"])
            out["min_preact"] = min(out["min_preact"], g["min_preact"])
            u = dict(drawn=drawn, leaves=leaves, prob=prob, data=data, padded=padded, total=tree_total, beta=this_beta, noise=z,
                     target_noise=tz, kl=g["loss_vec"], prio=g["prio"], loss=g["loss"], window_terminal=bool((mb["mask"] == 0).any()))
        if total / k_len % cfg["target_freq"] == 0:
            target = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
            out["copies"].append(step)
        out["actions"].append(a["action"]); out["rows"].append(rows); out["updates"].append(u); out["events"] += a["events"]
        out["params"].append({k: np.asarray(v).copy() for k, v in params.items()})
        out["rings"].append({k: v.copy() for k, v in ring.items()})
        out["margin"] = min(out["margin"], a["margin"])
    out.update(actions=np.stack(out["actions"]), ring=ring, target=target, tree=tree.tree.copy(), pending=sorted(tree.pending),
               max_priority=max_priority, pos=pos, size=size, total=total)
    return out
