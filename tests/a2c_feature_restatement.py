"""Restatement of what csrc/cat_mlp.hip and A2CAgent's cart-pole device path compute (TEST INFRASTRUCTURE ONLY): the categorical
actor-critic forward (network_heads.py:217-255 over a two-layer FCBody, network_bodies.py:50-73), one A2C update
(A2C_agent.py:43-64 with torch.optim.RMSprop's step, its running average carried from update to update), the Gumbel-max action
stream of dra_gumbel_sample, and the rollout (A2C_agent.py:22-41) over envs.CartPole, which is imported, not restated.  fp64 by
default; dtype=torch.float32 runs the same forward in fp32 (the margin test).  tests/test_a2c_feature_host.py pins it to the
reference's own run (tests/golden/a2c_feature/) before a GPU test leans on it.  Parameters are dicts keyed like
CategoricalActorCriticNet.state_dict()."""
import math

import numpy as np
import torch

F64 = torch.float64
_GATES = {"relu": torch.relu, "tanh": torch.tanh}
_M = np.uint64
KEYS = ("phi_body.layers.0.weight", "phi_body.layers.0.bias", "phi_body.layers.1.weight", "phi_body.layers.1.bias",
        "fc_action.weight", "fc_action.bias", "fc_critic.weight", "fc_critic.bias")


def to_t(params, dtype=F64, requires_grad=False):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(requires_grad) for k, v in params.items()}


def init_params(hidden, seed, state_dim=4, n_actions=2):
    """float32 numpy parameters, O(0.3) scale: logits and values that matter (the reference's heads start at 1e-3)."""
    rs = np.random.RandomState(seed)
    mk = lambda *shape, scale=0.3: (rs.randn(*shape) * scale).astype(np.float32)
    return {"phi_body.layers.0.weight": mk(hidden, state_dim, scale=0.8), "phi_body.layers.0.bias": mk(hidden, scale=0.1),
            "phi_body.layers.1.weight": mk(hidden, hidden, scale=0.25), "phi_body.layers.1.bias": mk(hidden, scale=0.1),
            "fc_action.weight": mk(n_actions, hidden, scale=0.3), "fc_action.bias": mk(n_actions, scale=0.05),
            "fc_critic.weight": mk(1, hidden, scale=0.2), "fc_critic.bias": mk(1, scale=0.05)}


def _mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _M(30))) * _M(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _M(27))) * _M(0x94D049BB133111EB)
        return z ^ (z >> _M(31))


def gumbel_noise(noise_seed, step, rows, n_actions):
    """-log(-log u) of dra_gumbel_sample's stream for sampler step `step` and GLOBAL rows `rows` -> fp64 [len(rows), n_actions].
    u = (k + 0.5) / 2^23 with k the hash's top 23 bits: exact in fp32 and fp64 alike."""
    with np.errstate(over="ignore"):
        base = _mix64(_M(noise_seed & 0xFFFFFFFFFFFFFFFF) * _M(0x9E3779B97F4A7C15) + _M(step))
        h = _mix64(base + np.asarray(rows, dtype=np.uint64)[:, None] * _M(64) + np.arange(n_actions, dtype=np.uint64)[None, :])
    u = ((h >> _M(41)).astype(np.float64) + 0.5) / 8388608.0
    return -np.log(-np.log(u))


def forward(p, obs, gate="tanh"):
    """(logits [n, A], v [n, 1]) in the dtype of the parameters."""
    dt = p["fc_action.weight"].dtype
    g = _GATES[gate]
    x = torch.as_tensor(np.asarray(obs), dtype=dt)
    h = g(torch.nn.functional.linear(x, p["phi_body.layers.0.weight"], p["phi_body.layers.0.bias"]))
    h = g(torch.nn.functional.linear(h, p["phi_body.layers.1.weight"], p["phi_body.layers.1.bias"]))
    return (torch.nn.functional.linear(h, p["fc_action.weight"], p["fc_action.bias"]),
            torch.nn.functional.linear(h, p["fc_critic.weight"], p["fc_critic.bias"]))


def head(logits, action):
    """(log_pi_a [n, 1], entropy [n, 1]) of Categorical(logits=logits) for given actions."""
    lsm = torch.log_softmax(logits, dim=-1)
    lp = lsm.gather(1, torch.as_tensor(np.asarray(action), dtype=torch.int64).reshape(-1, 1))
    ent = -(lsm.exp() * lsm).sum(-1, keepdim=True)
    return lp, ent


def gae(reward, mask, value, discount, tau):
    """A2C_agent.py:43-53 with use_gae: reward / mask [T, N, 1], value [T + 1, N, 1] -> (advantage, ret) [T, N, 1]."""
    t_len = reward.shape[0]
    adv, ret = torch.zeros_like(reward), torch.zeros_like(reward)
    a, r = torch.zeros_like(reward[0]), value[t_len]
    for i in reversed(range(t_len)):
        r = reward[i] + discount * mask[i] * r
        td = reward[i] + discount * mask[i] * value[i + 1] - value[i]
        a = a * tau * discount * mask[i] + td
        adv[i], ret[i] = a, r
    return adv, ret


def a2c_update(params, states, actions, reward, mask, discount, tau, entropy_weight, value_loss_weight, gradient_clip, lr,
               alpha=0.99, eps=1e-8, gate="tanh", square_avg=None):
    """One A2CAgent.step's update: states [T + 1, N, S] (the last row is the bootstrap observation), actions [T, N], reward / mask
    [T, N, 1]; square_avg: torch.optim.RMSprop's running averages (None: a fresh optimiser).  Returns (new parameters, dict of
    log_pi_a, entropy, v, adv, ret, square_avg)."""
    p = to_t(params, requires_grad=True)
    t_len, n = reward.shape[0], reward.shape[1]
    s = torch.as_tensor(np.asarray(states), dtype=F64)
    logits, v = forward(p, s[:t_len].reshape(t_len * n, -1), gate)
    lp, ent = head(logits, np.asarray(actions).reshape(-1))
    with torch.no_grad():
        v_boot = forward(p, s[t_len], gate)[1]
        value = torch.cat([v.detach().reshape(t_len, n, 1), v_boot.reshape(1, n, 1)])
        adv, ret = gae(torch.as_tensor(np.asarray(reward), dtype=F64).reshape(t_len, n, 1),
                       torch.as_tensor(np.asarray(mask), dtype=F64).reshape(t_len, n, 1), value, discount, tau)
    policy_loss = -(lp * adv.reshape(-1, 1)).mean()
    value_loss = 0.5 * (ret.reshape(-1, 1) - v).pow(2).mean()
    loss = policy_loss - entropy_weight * ent.mean() + value_loss_weight * value_loss
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    total = math.sqrt(sum(float((g ** 2).sum()) for g in grads))
    coef = min(1.0, gradient_clip / (total + 1e-6))            # nn.utils.clip_grad_norm_
    new, sq_new = {}, {}
    for k, g in zip(names, grads):
        g = g * coef
        sq = (1.0 - alpha) * g * g if square_avg is None else alpha * square_avg[k] + (1.0 - alpha) * g * g
        sq_new[k] = sq
        new[k] = (p[k].detach() - lr * g / (sq.sqrt() + eps)).numpy()
    keep = dict(log_pi_a=lp.detach().reshape(t_len, n, 1).numpy(), entropy=ent.detach().reshape(t_len, n, 1).numpy(),
                v=value.numpy(), adv=adv.numpy(), ret=ret.numpy(), square_avg=sq_new)
    return new, keep


def rollout(params, envs, raw_states, t_len, noise_seed, sampler_step0, gate="tanh", n_global=None, env0=0, reward_coef=1.0,
            dtype=F64):
    """A2C_agent.py:22-41 over envs.CartPole objects (stepped with DummyVecEnv's auto reset): the policy acts on the float32
    observation, the action is argmax(logits + Gumbel noise of (noise_seed, sampler_step0 + t, env0 + i)) with ties to the
    lower index.  Returns float32 state [T, N, 4], int64 action [T, N], v [T + 1, N], reward / mask [T, N], `events`
    (sampler step, global environment, episodic return) in (step, environment) order, `raw_states` (the fp64 observations the
    next rollout starts from) and `margin`: the smallest |perturbed logit 1 - perturbed logit 0| of the rollout."""
    p = to_t(params, dtype)
    n = len(envs)
    out = dict(state=[], action=[], v=[], reward=[], mask=[])
    events, margin = [], float("inf")
    raw = np.asarray(raw_states, dtype=np.float64)
    with torch.no_grad():
        for t in range(t_len):
            x = raw.astype(np.float32)
            logits, v = forward(p, x, gate)
            pert = logits.to(F64).numpy() + gumbel_noise(noise_seed, sampler_step0 + t, env0 + np.arange(n), logits.shape[1])
            acts = np.argmax(pert, axis=1)          # (first maximum: the kernel's strict `>`)
            srt = np.sort(pert, axis=1)
            margin = min(margin, float((srt[:, -1] - srt[:, -2]).min()))
            nxt, done = [], []
            for i, e in enumerate(envs):
                s, _, d, info = e.step(int(acts[i]))
                if d:
                    events.append((sampler_step0 + t, env0 + i, float(info['episodic_return'])))
                    s = e.reset()
                nxt.append(s)
                done.append(d)
            out["state"].append(x)
            out["action"].append(acts.astype(np.int64))
            out["v"].append(v.to(F64).numpy().reshape(-1))
            out["reward"].append(np.full(n, np.float32(1.0 * reward_coef), dtype=np.float32))
            out["mask"].append(1.0 - np.asarray(done, dtype=np.float32))
            raw = np.stack(nxt)
        out["v"].append(forward(p, raw.astype(np.float32), gate)[1].to(F64).numpy().reshape(-1))
    res = {k: np.stack(v) for k, v in out.items()}
    res["events"], res["raw_states"], res["margin"] = events, raw, margin
    res["bootstrap_state"] = raw.astype(np.float32)
    return res
