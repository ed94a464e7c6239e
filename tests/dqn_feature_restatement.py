"""Restatement of what csrc/dqn_mlp.hip and DQNAgent's cart-pole device path compute (TEST INFRASTRUCTURE ONLY): the acting loop
with the draws made ahead (DQN_agent.py:23-45, torch_utils.py:51-58) over envs.CartPole, which is imported, not restated, feeding
a ring of four arrays (replay.py:75-90 with history_length 1, n_step 1), the minibatch (replay.py:112-140: state = frame idx,
next state = frame idx + 1), one update (DQN_agent.py:81-99, 128-133 with torch.optim.RMSprop's step) and the target copy
(DQN_agent.py:136-138).  The forward, the parameter layout and RMSprop are nstep_feature_restatement's.  fp64 by default;
dtype=torch.float32 runs the same arithmetic in fp32 (the margin tests).  tests/test_dqn_feature_host.py pins it to the
reference's own run (tests/golden/dqn_feature/) before a GPU test leans on it."""
import numpy as np
import torch

import nstep_feature_restatement as R
from nstep_feature_restatement import KEYS, forward, init_params, rmsprop_step, to_t      # noqa: F401

F64 = torch.float64


def new_ring(capacity):
    """The replay ring's four arrays: fp64 frames [capacity, 4], int64 actions, fp64 rewards, int32 masks; unwritten slots hold
    NaN / -1 so that a comparison sees a row that should not have been written."""
    return dict(frames=np.full((capacity, 4), np.nan), actions=np.full(capacity, -1, dtype=np.int64),
                rewards=np.full(capacity, np.nan), masks=np.full(capacity, -1, dtype=np.int32))


def act(params, env, raw, k_len, explore, random_action, ring, slot0, gate="relu", step0=0, reward_coef=1.0, dtype=F64):
    """k_len transitions of ONE envs.CartPole from the fp64 observation `raw`: q of the float32 observation, action =
    random_action[k] where explore[k] else np.argmax(q) (the first maximum), the environment step with the auto reset, ring row
    (slot0 + k) % capacity = (the fp64 observation the action was chosen on, action, reward_coef * reward, 1 - done).
    -> dict(q [k, 2] fp64, action [k], events [(step counter, 0, return)], raw (the observation the next call starts from),
    margin: the smallest |q_1 - q_0| at a non-exploring transition)."""
    p = to_t(params, dtype)
    cap = ring["actions"].shape[0]
    raw = np.asarray(raw, dtype=np.float64).copy()
    qs, acts, events, margin = [], [], [], float("inf")
    with torch.no_grad():
        for k in range(k_len):
            q = forward(p, raw.astype(np.float32)[None], gate).to(F64).numpy()[0]
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


def minibatch(ring, idx):
    """What tensor() hands the networks: float32 states (frame idx), next states (frame idx + 1), rewards and masks; int64 actions."""
    idx = np.asarray(idx, dtype=np.int64)
    return dict(state=ring["frames"][idx].astype(np.float32), next_state=ring["frames"][idx + 1].astype(np.float32),
                action=ring["actions"][idx].astype(np.int64), reward=ring["rewards"][idx].astype(np.float32),
                mask=ring["masks"][idx].astype(np.float32))


def loss_and_grads(params, target, batch, discount, double_q=False, gate="relu", dtype=F64):
    """DQN_agent.py:81-99, 128-129 on a minibatch -> dict(q_target [B], td = q_target - q_a [B], loss = 0.5 mean td^2, grads by
    name, min_preact: the smallest |pre-activation| of the three forwards, argmax_margin: the smallest |q_1 - q_0| of the online
    network on the next states (what double_q's argmax rests on), best: that argmax)."""
    p, pt = to_t(params, dtype, requires_grad=True), to_t(target, dtype)
    keep_t, keep_o, keep = {}, {}, {}
    with torch.no_grad():
        q_next = forward(pt, batch["next_state"], gate, keep_t)
        q_on = forward(p, batch["next_state"], gate, keep_o)
        best = torch.argmax(q_on, dim=-1)
        q_next = q_next.gather(1, best.unsqueeze(-1)).squeeze(1) if double_q else q_next.max(1)[0]
    rewards, masks = torch.as_tensor(batch["reward"], dtype=dtype), torch.as_tensor(batch["mask"], dtype=dtype)
    q_target = rewards + discount * q_next * masks
    q = forward(p, batch["state"], gate, keep)
    q_a = q.gather(1, torch.as_tensor(batch["action"]).unsqueeze(-1)).squeeze(-1)
    td = q_target - q_a
    loss = td.pow(2).mul(0.5).mean()
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    pre = [keep_t, keep] + ([keep_o] if double_q else [])
    return dict(q_target=q_target.detach().numpy(), td=td.detach().numpy(), loss=float(loss.detach()),
                grads={k: g.numpy() for k, g in zip(names, grads)},
                min_preact=float(min(min(np.abs(d["z1"].numpy()).min(), np.abs(d["z2"].numpy()).min()) for d in pre)),
                argmax_margin=float((q_on[:, 1] - q_on[:, 0]).abs().min()), best=best.numpy())


def update(params, target, ring, idx, discount, gradient_clip, lr, double_q=False, gate="relu", square_avg=None):
    """One update on the ring's rows at idx -> (new parameters, dict of loss_and_grads' fields and square_avg)."""
    out = loss_and_grads(params, target, minibatch(ring, idx), discount, double_q, gate)
    new, sq = rmsprop_step(params, out["grads"], gradient_clip, lr, square_avg=square_avg)
    out["square_avg"] = sq
    return new, out


def valid_index(index, pos, size):
    """replay.py:105-110 with history_length 1, n_step 1."""
    return (index >= 0 and index + 1 < pos) or (index >= pos and index + 1 < size)


def draw_indices(rs, batch, pos, size):
    """replay.py:92-103's rejection loop on the RandomState `rs`: one randint(0, size) per attempt."""
    out = []
    while len(out) < batch:
        i = int(rs.randint(0, size))
        if valid_index(i, pos, size):
            out.append(i)
    return np.asarray(out, dtype=np.int64)


def agent_run(init, env, cfg, rs, eps, n_steps, dtype=F64, target0=None):
    """n_steps DQNAgent.step()s in the reference's order: per transition [epsilon (1 below exploration_steps without a schedule
    call, else eps()), randint(2, size=1), rand(1)], the feed, the minibatch's draws and the update once total_steps >
    exploration_steps, the target copy when total_steps / K % freq == 0 (true division).  cfg: dict(k, batch, capacity,
    exploration_steps, target_freq, discount, gradient_clip, lr, double_q, gate); target0: the target's parameters at the
    start when they are not the online ones.  -> dict(actions [n_steps, K], flags,
    random_actions, slots, indices (per step, None before learning), losses, ring, events, params (per step, after it), target,
    margin, argmax_margin, explored, greedy, copies (the steps after which the target was copied), pos, size, total)."""
    params = {k: np.asarray(v, dtype=np.float64).copy() for k, v in init.items()}
    target = {k: np.asarray(v, dtype=np.float64).copy() for k, v in (target0 or params).items()}
    ring = new_ring(cfg["capacity"])
    raw = env.reset()
    k_len = cfg["k"]
    pos = size = total = actor_steps = 0
    sq = None
    out = dict(actions=[], flags=[], random_actions=[], slots=[], indices=[], losses=[], events=[], params=[], copies=[],
               margin=float("inf"), argmax_margin=float("inf"), explored=0, greedy=0, min_preact=float("inf"))
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
            pos = (pos + 1) % cfg["capacity"]
        total += k_len
        idx = None
        if total > cfg["exploration_steps"]:
            idx = draw_indices(rs, cfg["batch"], pos, size)
            params, u = update(params, target, ring, idx, cfg["discount"], cfg["gradient_clip"], cfg["lr"], cfg["double_q"],
                               cfg["gate"], sq)
            sq = u["square_avg"]
            out["losses"].append(u["loss"])
            out["min_preact"] = min(out["min_preact"], u["min_preact"])
            if cfg["double_q"]:
                out["argmax_margin"] = min(out["argmax_margin"], u["argmax_margin"])
        if total / k_len % cfg["target_freq"] == 0:
            target = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
            out["copies"].append(step)
        out["actions"].append(a["action"]); out["flags"].append(explore); out["random_actions"].append(rand)
        out["indices"].append(idx); out["events"] += a["events"]
        out["params"].append({k: np.asarray(v).copy() for k, v in params.items()})
        out["margin"] = min(out["margin"], a["margin"])
        out["explored"] += int(explore.sum()); out["greedy"] += int((~explore).sum())
    out.update(ring=ring, target=target, pos=pos, size=size, total=total, actions=np.stack(out["actions"]),
               flags=np.stack(out["flags"]), random_actions=np.stack(out["random_actions"]))
    return out
