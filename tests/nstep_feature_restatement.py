"""Restatement of what csrc/q_mlp.hip and NStepDQNAgent's cart-pole device path compute (TEST INFRASTRUCTURE ONLY): the VanillaNet
forward (network_heads.py:11-21 over a two-layer FCBody, network_bodies.py:50-73), the epsilon-greedy rollout with the draws made
ahead (NStepDQN_agent.py:31-57, torch_utils.py:51-58) over envs.CartPole, which is imported, not restated, and one update
(NStepDQN_agent.py:58-67 with torch.optim.RMSprop's step, its running average carried from update to update).  fp64 by default;
dtype=torch.float32 runs the same arithmetic in fp32 (the margin test, the order-exact returns).
tests/test_nstep_feature_host.py pins it to the reference's own run (tests/golden/nstep_feature/) before a GPU test leans on it.
Parameters are dicts keyed like VanillaNet.state_dict()."""
import math

import numpy as np
import torch

F64 = torch.float64
_GATES = {"relu": torch.relu, "tanh": torch.tanh}
KEYS = ("body.layers.0.weight", "body.layers.0.bias", "body.layers.1.weight", "body.layers.1.bias", "fc_head.weight", "fc_head.bias")


def to_t(params, dtype=F64, requires_grad=False):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(requires_grad) for k, v in params.items()}


def init_params(hidden, seed, state_dim=4, n_actions=2):
    """float32 numpy parameters, O(0.3) scale: action values that differ (the reference's head starts orthogonal at scale 1)."""
    rs = np.random.RandomState(seed)
    mk = lambda *shape, scale=0.3: (rs.randn(*shape) * scale).astype(np.float32)
    return {"body.layers.0.weight": mk(hidden, state_dim, scale=0.8), "body.layers.0.bias": mk(hidden, scale=0.1),
            "body.layers.1.weight": mk(hidden, hidden, scale=0.25), "body.layers.1.bias": mk(hidden, scale=0.1),
            "fc_head.weight": mk(n_actions, hidden, scale=0.3), "fc_head.bias": mk(n_actions, scale=0.05)}


def forward(p, obs, gate="relu", keep=None):
    """q [n, A] in the dtype of the parameters; `keep` (a dict) receives the two layers' pre-activations."""
    dt = p["fc_head.weight"].dtype
    g = _GATES[gate]
    x = torch.as_tensor(np.asarray(obs), dtype=dt)
    z1 = torch.nn.functional.linear(x, p["body.layers.0.weight"], p["body.layers.0.bias"])
    z2 = torch.nn.functional.linear(g(z1), p["body.layers.1.weight"], p["body.layers.1.bias"])
    if keep is not None:
        keep["z1"], keep["z2"] = z1.detach(), z2.detach()
    return torch.nn.functional.linear(g(z2), p["fc_head.weight"], p["fc_head.bias"])


def returns(reward, mask, bootstrap, discount, dtype=np.float64):
    """NStepDQN_agent.py:57-60 in the reference's loop and operation order, r + (discount * m) * ret with one rounding per
    operation in `dtype` (float32: what the reference's fp32 tensors and the kernels compute, bit for bit): reward / mask [T, N],
    bootstrap [N] -> ret [T, N]."""
    reward, mask = np.asarray(reward, dtype=dtype), np.asarray(mask, dtype=dtype)
    ret = np.asarray(bootstrap, dtype=dtype).reshape(-1)
    g = dtype(discount)
    out = np.zeros(reward.shape, dtype=dtype)
    for i in reversed(range(reward.shape[0])):
        ret = (reward[i] + ((g * mask[i]).astype(dtype) * ret).astype(dtype)).astype(dtype)
        out[i] = ret
    return out


def loss_and_grads(params, states, actions, reward, mask, bootstrap, discount, gate="relu"):
    """fp64: states [T, N, S], actions / reward / mask [T, N], bootstrap [N] -> (ret [T, N], loss, {name: gradient of
    0.5 mean (q_a - ret)^2}, q [T, N, A], pre-activations)."""
    p = to_t(params, requires_grad=True)
    t_len, n = np.asarray(reward).shape
    ret = returns(reward, mask, bootstrap, discount)
    keep = {}
    q = forward(p, np.asarray(states, dtype=np.float64).reshape(t_len * n, -1), gate, keep)
    q_a = q.gather(1, torch.as_tensor(np.asarray(actions), dtype=torch.int64).reshape(-1, 1))
    loss = 0.5 * (q_a - torch.as_tensor(ret).reshape(-1, 1)).pow(2).mean()
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    return (ret, float(loss.detach()), {k: g.numpy() for k, g in zip(names, grads)}, q.detach().numpy().reshape(t_len, n, -1),
            {k: v.numpy() for k, v in keep.items()})


def rmsprop_step(params, grads, gradient_clip, lr, alpha=0.99, eps=1e-8, square_avg=None):
    """nn.utils.clip_grad_norm_ + torch.optim.RMSprop.step in fp64 -> (new parameters, the running averages)."""
    total = math.sqrt(sum(float((g ** 2).sum()) for g in grads.values()))
    coef = min(1.0, gradient_clip / (total + 1e-6))
    new, sq_new = {}, {}
    for k, g in grads.items():
        g = g * coef
        sq = (1.0 - alpha) * g * g if square_avg is None else alpha * square_avg[k] + (1.0 - alpha) * g * g
        sq_new[k] = sq
        new[k] = np.asarray(params[k], dtype=np.float64) - lr * g / (np.sqrt(sq) + eps)
    return new, sq_new


def nstep_update(params, boot_params, states, actions, reward, mask, discount, gradient_clip, lr, gate="relu", square_avg=None):
    """One NStepDQNAgent.step's update: states [T + 1, N, S] (the last row is the bootstrap observation, valued by `boot_params`:
    the target network's, or the online ones when the copy fell inside the rollout).  Returns (new parameters, dict of q, ret,
    loss, bootstrap, grads, square_avg)."""
    t_len = np.asarray(reward).shape[0]
    with torch.no_grad():
        boot = forward(to_t(boot_params), np.asarray(states[t_len], dtype=np.float64), gate).max(dim=1)[0].numpy()
    ret, loss, grads, q, _ = loss_and_grads(params, states[:t_len], actions, reward, mask, boot, discount, gate)
    new, sq = rmsprop_step(params, grads, gradient_clip, lr, square_avg=square_avg)
    return new, dict(q=q, ret=ret, loss=loss, bootstrap=boot, grads=grads, square_avg=sq)


def rollout(params, target_params, envs, raw_states, t_len, explore, random_action, gate="relu", step0=0, reward_coef=1.0, dtype=F64):
    """NStepDQN_agent.py:31-57 over envs.CartPole objects (stepped with DummyVecEnv's auto reset): q on the float32 observation,
    action = random_action[t, i] where explore[t, i] else np.argmax(q) (the first maximum).  Returns float32 state [T, N, 4], q
    [T, N, 2], int64 action [T, N], reward / mask [T, N], bootstrap [N] (max_a of the TARGET parameters' q on the last
    observation), `events` (step counter, environment, episodic return) in (step, environment) order, `raw_states` (the fp64
    observations the next rollout starts from) and `margin`: the smallest |q_1 - q_0| at a NON-exploring (step, environment)."""
    p, pt = to_t(params, dtype), to_t(target_params, dtype)
    n = len(envs)
    out = dict(state=[], q=[], action=[], reward=[], mask=[])
    events, margin = [], float("inf")
    raw = np.asarray(raw_states, dtype=np.float64)
    explore = np.asarray(explore).astype(bool)
    with torch.no_grad():
        for t in range(t_len):
            x = raw.astype(np.float32)
            q = forward(p, x, gate).to(F64).numpy()
            acts = np.where(explore[t], np.asarray(random_action[t]), np.argmax(q, axis=1)).astype(np.int64)
            gap = np.abs(q[:, 1] - q[:, 0])[~explore[t]]
            if gap.size:
                margin = min(margin, float(gap.min()))
            nxt, done = [], []
            for i, e in enumerate(envs):
                s, _, d, info = e.step(int(acts[i]))
                if d:
                    events.append((step0 + t, i, float(info['episodic_return'])))
                    s = e.reset()
                nxt.append(s)
                done.append(d)
            out["state"].append(x)
            out["q"].append(q)
            out["action"].append(acts)
            out["reward"].append(np.full(n, np.float32(1.0 * reward_coef), dtype=np.float32))
            out["mask"].append(1.0 - np.asarray(done, dtype=np.float32))
            raw = np.stack(nxt)
        boot = forward(pt, raw.astype(np.float32), gate).to(F64).numpy().max(axis=1)
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(events=events, raw_states=raw, margin=margin, bootstrap=boot, bootstrap_state=raw.astype(np.float32))
    return res
