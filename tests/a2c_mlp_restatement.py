"""fp64 restatement of what csrc/a2c_mlp.hip and A2CAgent's device path compute (TEST INFRASTRUCTURE ONLY): the relu / tanh
Gaussian actor-critic forward (network_heads.py:198-214 over two FCBody stacks, network_bodies.py:50-73), the head's gradients,
one A2C update (A2C_agent.py:43-64 with torch.optim.RMSprop's step) and the rollout (A2C_agent.py:22-41) over the oracle's
synthetic continuous environments, observation normaliser and hashed action noise, which are imported, not restated.
tests/test_a2c_continuous_host.py pins it to the reference's own run (tests/golden/a2c_continuous/) before a GPU test leans on it.
Parameters are dicts keyed like GaussianActorCriticNet.state_dict()."""
import math

import numpy as np
import torch

from oracle.numerics_oracle import MeanStdNormalizerOracle, RunningMeanStdOracle  # noqa: F401  (re-exported for the tests)
from oracle.ppo_mlp_oracle import ContinuousEnvOracle, gauss_noise  # noqa: F401

F64 = torch.float64
_GATES = {"relu": torch.relu, "tanh": torch.tanh}
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def to64(params, requires_grad=False, dtype=F64):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(requires_grad) for k, v in params.items()}


def init_params(state_dim, action_dim, hidden, seed):
    """float32 numpy parameters, O(0.1) scale, std spread over both signs."""
    rs = np.random.RandomState(seed)
    mk = lambda *shape, scale=0.3: (rs.randn(*shape) * scale).astype(np.float32)
    p = {"std": mk(action_dim, scale=0.4)}
    for body in ("actor_body", "critic_body"):
        p[body + ".layers.0.weight"], p[body + ".layers.0.bias"] = mk(hidden, state_dim), mk(hidden, scale=0.1)
        p[body + ".layers.1.weight"], p[body + ".layers.1.bias"] = mk(hidden, hidden, scale=0.15), mk(hidden, scale=0.1)
    p["fc_action.weight"], p["fc_action.bias"] = mk(action_dim, hidden, scale=0.1), mk(action_dim, scale=0.05)
    p["fc_critic.weight"], p["fc_critic.bias"] = mk(1, hidden, scale=0.1), mk(1, scale=0.05)
    return p


def softplus(x):
    """F.softplus (beta 1): linear above the threshold 20."""
    return torch.where(x > 20.0, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def _body(p, prefix, x, gate):
    g = _GATES[gate]
    h = g(torch.nn.functional.linear(x, p[prefix + ".layers.0.weight"], p[prefix + ".layers.0.bias"]))
    return g(torch.nn.functional.linear(h, p[prefix + ".layers.1.weight"], p[prefix + ".layers.1.bias"]))


def head(z, std, action):
    """(mean, log_pi_a [n, 1], entropy [n, 1]) of Normal(tanh(z), softplus(std)) for given actions."""
    mean = torch.tanh(z)
    scale = softplus(std)
    lp = (-(action - mean) ** 2 / (2.0 * scale ** 2) - torch.log(scale) - HALF_LOG_2PI).sum(-1, keepdim=True)
    ent = (0.5 + HALF_LOG_2PI + torch.log(scale)).sum(-1, keepdim=True).expand(z.shape[0], 1)
    return mean, lp, ent


def head_grads(z, std, action, g_lp, g_ent):
    """(dz, dstd) of head() for the output gradients g_lp, g_ent [n, 1], by autograd in fp64."""
    z = torch.as_tensor(np.asarray(z), dtype=F64).clone().requires_grad_(True)
    std = torch.as_tensor(np.asarray(std), dtype=F64).clone().requires_grad_(True)
    _, lp, ent = head(z, std, torch.as_tensor(np.asarray(action), dtype=F64))
    torch.autograd.backward([lp, ent], [torch.as_tensor(np.asarray(g_lp), dtype=F64).reshape(-1, 1),
                                        torch.as_tensor(np.asarray(g_ent), dtype=F64).reshape(-1, 1)])
    return z.grad.numpy(), std.grad.numpy()


def forward(p, obs, action=None, noise=None, gate="relu", dtype=F64):
    """network_heads.py:198-214; `noise`: the standard normals of dist.sample() (action = mean + scale * noise).  `dtype`: the
    type the forward runs in (the parameters `p` are expected in it)."""
    obs = torch.as_tensor(np.asarray(obs), dtype=dtype)
    z = torch.nn.functional.linear(_body(p, "actor_body", obs, gate), p["fc_action.weight"], p["fc_action.bias"])
    v = torch.nn.functional.linear(_body(p, "critic_body", obs, gate), p["fc_critic.weight"], p["fc_critic.bias"])
    if action is None:
        with torch.no_grad():
            action = torch.tanh(z) + softplus(p["std"]) * torch.as_tensor(np.asarray(noise), dtype=dtype)
    else:
        action = torch.as_tensor(np.asarray(action), dtype=dtype)
    mean, lp, ent = head(z, p["std"], action)
    return dict(action=action, log_pi_a=lp, entropy=ent, mean=mean, v=v, z=z)


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
               alpha=0.99, eps=1e-8, gate="relu"):
    """One A2CAgent.step's update from a fresh RMSprop: states [T + 1, N, S] (the last row is the bootstrap observation),
    actions [T, N, A], reward / mask [T, N, 1].  Returns (new parameters, dict of log_pi_a, entropy, v, adv, ret)."""
    p = to64(params, requires_grad=True)
    t_len, n = reward.shape[0], reward.shape[1]
    s = torch.as_tensor(np.asarray(states), dtype=F64)
    pred = forward(p, s[:t_len].reshape(t_len * n, -1), torch.as_tensor(np.asarray(actions), dtype=F64).reshape(t_len * n, -1),
                   gate=gate)
    with torch.no_grad():
        v_boot = forward(p, s[t_len], noise=np.zeros((n, actions.shape[-1])), gate=gate)["v"]
        value = torch.cat([pred["v"].detach().reshape(t_len, n, 1), v_boot.reshape(1, n, 1)])
        adv, ret = gae(torch.as_tensor(np.asarray(reward), dtype=F64), torch.as_tensor(np.asarray(mask), dtype=F64), value,
                       discount, tau)
    policy_loss = -(pred["log_pi_a"] * adv.reshape(-1, 1)).mean()
    value_loss = 0.5 * (ret.reshape(-1, 1) - pred["v"]).pow(2).mean()
    loss = policy_loss - entropy_weight * pred["entropy"].mean() + value_loss_weight * value_loss
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    total = math.sqrt(sum(float((g ** 2).sum()) for g in grads))
    coef = min(1.0, gradient_clip / (total + 1e-6))            # nn.utils.clip_grad_norm_
    new = {}
    for k, g in zip(names, grads):
        g = g * coef
        sq = (1.0 - alpha) * g * g                              # torch.optim.RMSprop, first step: square_avg starts at zero
        new[k] = (p[k].detach() - lr * g / (sq.sqrt() + eps)).numpy()
    keep = dict(log_pi_a=pred["log_pi_a"].detach().reshape(t_len, n, 1).numpy(), entropy=pred["entropy"].detach().reshape(t_len, n, 1).numpy(),
                v=value.numpy(), adv=adv.numpy(), ret=ret.numpy(), grads={k: g.numpy() for k, g in zip(names, grads)})
    return new, keep


def start_envs(seeds, state_dim, action_dim, horizon, pre_steps=None):
    """(environments, their raw observations [n, S]) after reset() and, for environment i, pre_steps[i] steps with zero actions:
    a start whose step counters differ from one environment to the next.  pre_steps None: fresh environments."""
    envs = [ContinuousEnvOracle(s, state_dim, action_dim, horizon) for s in seeds]
    raw = []
    for i, e in enumerate(envs):
        s = e.reset()
        for _ in range(pre_steps[i] if pre_steps is not None else 0):
            s, _, _ = e.step(np.zeros(action_dim, dtype=np.float32))
        raw.append(s)
    return envs, np.stack(raw)


def warm_normalizer(kind, state_dim, warm_rows, clip=10.0):
    """(normaliser, statistics [2 S + 1] = mean, var, count) for `kind`: "identity" (None, and the statistics a fresh
    RunningMeanStd holds), or a MeanStdNormalizerOracle clipping at +-clip that has seen `warm_rows` rows, updating
    ("meanstd-update") or read-only ("meanstd-readonly") from here on."""
    if kind == "identity":
        return None, np.concatenate([np.zeros(state_dim), np.ones(state_dim), [0.0]])
    norm = MeanStdNormalizerOracle(clip=clip)
    norm.rms = RunningMeanStdOracle(shape=(1, state_dim))
    norm(np.random.RandomState(5).randn(warm_rows, state_dim) * 0.05 + 0.01)
    norm.read_only = kind == "meanstd-readonly"
    return norm, np.concatenate([norm.rms.mean.reshape(-1), norm.rms.var.reshape(-1), [norm.rms.count]])


def rollout(params, envs, raw_states, normalizer, t_len, noise_seed, sampler_step0, gate="relu", n_global=None, env0=0,
            reward_coef=1.0, dtype=F64):
    """A2C_agent.py:22-41 over ContinuousEnvOracle environments: per step the normaliser is called on the CURRENT raw observation
    (it folds it into its statistics unless read-only), the policy acts on the float32 result, the environments step; the
    bootstrap observation is normalised (and folded) too.  normalizer None: the identity.  Returns float arrays state [T, N, S],
    action [T, N, A], v [T + 1, N], reward / mask [T, N], cur_state (the normalised bootstrap observation), raw_states, and
    the number of terminals.  `dtype`: the type both forwards run in (environments and normaliser stay fp64)."""
    p = to64(params, dtype=dtype)
    n = len(envs)
    n_global = n_global or n
    a_dim = p["fc_action.weight"].shape[0]
    out = dict(state=[], action=[], v=[], reward=[], mask=[])
    raw = np.asarray(raw_states, dtype=np.float64)
    norm = lambda r: np.asarray(normalizer(r) if normalizer is not None else r, dtype=np.float32)
    with torch.no_grad():
        for t in range(t_len):
            x = norm(raw)
            noise = gauss_noise(noise_seed, sampler_step0 + t, n_global, env0 + np.arange(n), a_dim)
            pred = forward(p, x, noise=noise, gate=gate, dtype=dtype)
            acts = pred["action"].numpy()
            nxt, rew, done = [], [], []
            for i, e in enumerate(envs):
                s, r, d = e.step(acts[i].astype(np.float32))
                nxt.append(s); rew.append(r); done.append(d)
            out["state"].append(x.copy()); out["action"].append(acts.copy()); out["v"].append(pred["v"].numpy().reshape(-1))
            out["reward"].append(np.asarray(np.asarray(rew) * reward_coef, dtype=np.float32))
            out["mask"].append(np.asarray(1 - np.asarray(done), dtype=np.float32))
            raw = np.stack(nxt)
        x = norm(raw)
        out["v"].append(forward(p, x, noise=np.zeros((n, a_dim)), gate=gate, dtype=dtype)["v"].numpy().reshape(-1))
    res = {k: np.stack(v) for k, v in out.items()}
    res["cur_state"], res["raw_states"] = x, raw
    res["terminals"] = int((res["mask"] == 0).sum())
    return res
