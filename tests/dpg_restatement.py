"""fp64 restatement of the DDPG and TD3 updates (DDPG_agent.py:75-100, TD3_agent.py:72-108), what csrc/dpg_mlp.hip is held to:
targets, both losses' gradients (torch autograd in fp64 over the agent's own expressions), torch.optim.Adam's step, the soft
target update and TD3's cadence.  tests/test_dpg_update_host.py pins it to the reference's recorded updates.

Parameters travel as dicts of fp64 tensors under canonical names: a.w1 a.b1 a.w2 a.b2 a.w3 a.b3 (actor_body.layers[0..1],
fc_action) and c0.* / c1.* (the critic(s)); `canonical` / `NAMES` translate from the two networks' state_dict names."""
import numpy as np
import torch

LAYERS = ("w1", "b1", "w2", "b2", "w3", "b3")
_SUFFIX = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias")


def _names(body, head):
    return ["%s.%s" % (body, s) for s in _SUFFIX] + [head + ".weight", head + ".bias"]


# canonical prefix -> the six state_dict names, per network class
NAMES = {1: {"a": _names("actor_body", "fc_action"), "c0": _names("critic_body", "fc_critic")},
         2: {"a": _names("actor_body", "fc_action"), "c0": _names("critic_body_1", "fc_critic_1"),
             "c1": _names("critic_body_2", "fc_critic_2")}}


def canonical(state_dict, n_critics, prefix=""):
    """{'a.w1': fp64 tensor, ...} from a DeterministicActorCriticNet (n_critics 1) / TD3Net (2) state_dict (arrays or tensors)."""
    out = {}
    for role, names in NAMES[n_critics].items():
        for lay, n in zip(LAYERS, names):
            out["%s.%s" % (role, lay)] = torch.as_tensor(np.asarray(state_dict[prefix + n]), dtype=torch.float64).clone()
    return out


def gate_fn(gate):
    return {1: torch.relu, 2: torch.tanh}[gate]


def mlp(p, role, x, gate):
    g = gate_fn(gate)
    h = g(x @ p[role + ".w1"].t() + p[role + ".b1"])
    h = g(h @ p[role + ".w2"].t() + p[role + ".b2"])
    return h @ p[role + ".w3"].t() + p[role + ".b3"]


def actor(p, s, gate):
    return torch.tanh(mlp(p, "a", s, gate))


def critic(p, c, s, a, gate):
    return mlp(p, "c%d" % c, torch.cat([s, a], dim=1), gate)


def f64(x):
    """A minibatch field as the agents hand it to the network: narrowed to fp32 first (torch_utils.py:20-25)."""
    return torch.as_tensor(np.asarray(x, dtype=np.float32).astype(np.float64))


def target_y(tgt, batch, hp, n_critics, gate, noise=None):
    """y [B][1]; `noise`: TD3's standard normals [B][A] (randn_like's draw, or the counter-hash stream)."""
    s2, r, m = f64(batch["next_state"]), f64(batch["reward"]).reshape(-1, 1), f64(batch["mask"]).reshape(-1, 1)
    a2 = actor(tgt, s2, gate)
    if n_critics == 2:
        nz = (f64(noise) * hp["td3_noise"]).clamp(-hp["td3_noise_clip"], hp["td3_noise_clip"])
        a2 = (a2 + nz).clamp(hp["action_low"], hp["action_high"])
        qn = torch.min(critic(tgt, 0, s2, a2, gate), critic(tgt, 1, s2, a2, gate))
    else:
        qn = critic(tgt, 0, s2, a2, gate)
    return r + hp["discount"] * m * qn


def adam(p, g, m, v, t, hp):
    """torch.optim.Adam (no amsgrad / weight decay) on one tensor, in place; t is the 1-based step count."""
    b1, b2 = hp["beta1"], hp["beta2"]
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    denom = v.sqrt() / np.sqrt(1 - b2 ** t) + hp["eps"]
    p.sub_(hp["lr"] / (1 - b1 ** t) * (m / denom))


class State:
    """Online / target parameters, Adam moments and the two optimisers' step counts."""

    def __init__(self, online, target, n_critics, gate, exp_avg=None, exp_avg_sq=None):
        self.online = {k: v.clone() for k, v in online.items()}
        self.target = {k: v.clone() for k, v in target.items()}
        self.m = {k: torch.zeros_like(v) for k, v in online.items()} if exp_avg is None else {k: v.clone() for k, v in exp_avg.items()}
        self.v = {k: torch.zeros_like(v) for k, v in online.items()} if exp_avg_sq is None else {k: v.clone() for k, v in exp_avg_sq.items()}
        self.n_critics, self.gate = n_critics, gate
        self.t_actor = self.t_critic = 0

    def _step(self, keys, grads, t, hp):
        for k, g in zip(keys, grads):
            adam(self.online[k], g, self.m[k], self.v[k], t, hp)

    def critic_update(self, batch, hp, noise=None):
        """Returns dict(y, q [n_critics][B], loss [B]) of the step (q, loss before the parameters move)."""
        nc, gate = self.n_critics, self.gate
        y = target_y(self.target, batch, hp, nc, gate, noise)
        keys = [k for k in self.online if k.startswith("c")]
        leaves = {k: self.online[k].clone().requires_grad_(True) for k in keys}
        p = dict(self.online, **leaves)
        s, a = f64(batch["state"]), f64(batch["action"])
        qs = [critic(p, c, s, a, gate) for c in range(nc)]
        if nc == 1:
            rows = (qs[0] - y).pow(2).mul(0.5).sum(-1)
        else:
            rows = ((qs[0] - y).pow(2) + (qs[1] - y).pow(2)).sum(-1)     # mse_loss + mse_loss: means over the B x 1 elements
        grads = torch.autograd.grad(rows.mean(), [leaves[k] for k in keys])
        self.t_critic += 1
        self._step(keys, grads, self.t_critic, hp)
        return dict(y=y.detach().reshape(-1).numpy(), q=np.stack([q.detach().reshape(-1).numpy() for q in qs]),
                    loss=rows.detach().numpy())

    def actor_update(self, batch, hp):
        gate = self.gate
        keys = [k for k in self.online if k.startswith("a.")]
        leaves = {k: self.online[k].clone().requires_grad_(True) for k in keys}
        p = dict(self.online, **leaves)
        s = f64(batch["state"])
        loss = -critic(p, 0, s, actor(p, s, gate), gate).mean()
        grads = torch.autograd.grad(loss, [leaves[k] for k in keys])
        self.t_actor += 1
        self._step(keys, grads, self.t_actor, hp)

    def soft_update(self, mix):
        for k in self.target:
            self.target[k].mul_(1.0 - mix).add_(self.online[k] * mix)

    def update(self, batch, hp, policy_step=True, noise=None):
        """One agent update: DDPG always takes the policy step; TD3 on the steps its delay test selects."""
        out = self.critic_update(batch, hp, noise)
        if policy_step:
            self.actor_update(batch, hp)
            self.soft_update(hp["target_network_mix"])
        return out


def hash_noise(seed, counter, batch, a_dim):
    """The smoothing noise the kernel draws when none is passed: gauss_noise(seed, t = counter, n_global = B, rows, A)."""
    from oracle.ppo_mlp_oracle import gauss_noise
    return gauss_noise(seed, counter, batch, np.arange(batch), a_dim)
