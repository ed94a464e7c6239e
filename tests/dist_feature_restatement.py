"""Restatement of what csrc/dist_mlp.hip and the cart-pole device path of CategoricalDQNAgent / QuantileRegressionDQNAgent compute
(TEST INFRASTRUCTURE ONLY): CategoricalNet / QuantileNet over a two-layer FCBody (network_heads.py:40-54, 89-102), the action
values (CategoricalDQN_agent.py:22-24: sum_j softmax_j z_j; QuantileRegressionDQN_agent.py:18-20: the quantiles' mean), the acting
loop with the draws made ahead, the ring and the minibatch (dqn_feature_restatement's, with this module's action values), the two
losses (oracle/loss_oracle.py's c51_kl and qr_loss on fp64 tensors) with autograd's gradients, RMSprop's step and the target copy.
fp64 by default; dtype=torch.float32 runs the same arithmetic in fp32 (the margin tests).  The atoms are np.linspace in fp64
NARROWED to float32 (what tensor(config.atoms) hands the networks), tau likewise.  tests/test_dist_feature_host.py pins it to the
reference's own run (tests/golden/dist_feature/) before a GPU test leans on it.

A spec is dict(head="c51" | "qr", n=atoms per action, v_min, v_max (c51)).  Parameters are dicts keyed like the network's
state_dict()."""
import os
import sys

import numpy as np
import torch

import dqn_feature_restatement as D
from dqn_feature_restatement import draw_indices, minibatch, new_ring, valid_index      # noqa: F401
from nstep_feature_restatement import rmsprop_step, to_t      # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import loss_oracle as L      # noqa: E402

F64 = torch.float64
_D_ACT, _D_AGENT_RUN = D.act, D.agent_run
_GATES = {"relu": torch.relu, "tanh": torch.tanh}
HEAD_LAYER = {"c51": "fc_categorical", "qr": "fc_quantiles"}
BODY_KEYS = ("body.layers.0.weight", "body.layers.0.bias", "body.layers.1.weight", "body.layers.1.bias")


def keys(head):
    return BODY_KEYS + (HEAD_LAYER[head] + ".weight", HEAD_LAYER[head] + ".bias")


def init_params(hidden, seed, spec, state_dim=4, n_actions=2, head_scale=0.3):
    """float32 numpy parameters, O(0.3) scale: distributions and quantiles that differ between the actions."""
    rs = np.random.RandomState(seed)
    mk = lambda *shape, scale=0.3: (rs.randn(*shape) * scale).astype(np.float32)
    w, b = keys(spec["head"])[4:]
    return {"body.layers.0.weight": mk(hidden, state_dim, scale=0.8), "body.layers.0.bias": mk(hidden, scale=0.1),
            "body.layers.1.weight": mk(hidden, hidden, scale=0.25), "body.layers.1.bias": mk(hidden, scale=0.1),
            w: mk(n_actions * spec["n"], hidden, scale=head_scale), b: mk(n_actions * spec["n"], scale=0.05)}


def atoms(spec):
    """tensor(np.linspace(v_min, v_max, n)): float32 values."""
    return np.linspace(spec["v_min"], spec["v_max"], spec["n"]).astype(np.float32)


def taus(n):
    """QuantileRegressionDQN_agent.py:39-40: tensor((2 i + 1) / (2 N)): float32 values."""
    return ((2 * np.arange(n) + 1) / (2.0 * n)).astype(np.float32)


def head_out(p, obs, spec, gate="relu", keep=None):
    """The head's output [n, A, N] (logits / quantiles) in the dtype of the parameters; `keep` receives the pre-activations."""
    w, b = keys(spec["head"])[4:]
    dt = p[w].dtype
    g = _GATES[gate]
    x = torch.as_tensor(np.asarray(obs), dtype=dt)
    z1 = torch.nn.functional.linear(x, p["body.layers.0.weight"], p["body.layers.0.bias"])
    z2 = torch.nn.functional.linear(g(z1), p["body.layers.1.weight"], p["body.layers.1.bias"])
    if keep is not None:
        keep["z1"], keep["z2"] = z1.detach(), z2.detach()
    return torch.nn.functional.linear(g(z2), p[w], p[b]).view(x.shape[0], -1, spec["n"])


def action_values(out, spec):
    """q [n, A] of a head output."""
    if spec["head"] == "c51":
        z = torch.as_tensor(atoms(spec)).to(out.dtype)
        return (torch.softmax(out, dim=-1) * z).sum(-1)
    return out.mean(-1)


def forward(p, obs, spec, gate="relu", keep=None):
    return action_values(head_out(p, obs, spec, gate, keep), spec)


def act(params, env, raw, k_len, explore, random_action, ring, slot0, spec, gate="relu", step0=0, reward_coef=1.0, dtype=F64):
    """dqn_feature_restatement.act with this module's action values (its `forward` is a module global: swapped for the call)."""
    saved = D.forward
    D.forward = lambda p, obs, g: forward(p, obs, spec, g)
    try:
        return _D_ACT(params, env, raw, k_len, explore, random_action, ring, slot0, gate=gate, step0=step0,
                      reward_coef=reward_coef, dtype=dtype)
    finally:
        D.forward = saved


def loss_and_grads(params, target, batch, discount, spec, double_q=False, gate="relu", dtype=F64):
    """CategoricalDQN_agent.py:60-89 / QuantileRegressionDQN_agent.py:55-77 on a minibatch -> dict(loss, loss_vec (c51: KL [B]; qr:
    the per-target-quantile vector [N]), q_next [B, A] (the TARGET network's action values of the next states), target [B, N] (the
    projected probabilities, or the target quantiles), a_next [B], grads by name, argmax_margin: the smallest |q_1 - q_0| the choice
    of a_next rests on, min_preact: the smallest |pre-activation| of the forwards)."""
    head, n = spec["head"], spec["n"]
    p, pt = to_t(params, dtype, requires_grad=True), to_t(target, dtype)
    rewards, masks = torch.as_tensor(batch["reward"], dtype=dtype), torch.as_tensor(batch["mask"], dtype=dtype)
    actions = torch.as_tensor(batch["action"])
    keep_t, keep_o, keep = {}, {}, {}
    b = torch.arange(actions.shape[0])
    with torch.no_grad():
        out_t = head_out(pt, batch["next_state"], spec, gate, keep_t)
        q_next = action_values(out_t, spec)
        q_choice = q_next
        if head == "c51" and double_q:
            out_o = head_out(p, batch["next_state"], spec, gate, keep_o)
            q_choice = action_values(out_o, spec)
        a_next = torch.argmax(q_choice, dim=-1)
    out = head_out(p, batch["state"], spec, gate, keep)
    if head == "c51":
        z = torch.as_tensor(atoms(spec)).to(dtype)
        prob_t = torch.softmax(out_t, dim=-1)
        prob_o = torch.softmax(out_o, dim=-1) if double_q else None
        vec = L.c51_kl(torch.log_softmax(out, dim=-1), prob_t, actions, rewards, masks, discount, z, spec["v_min"], spec["v_max"],
                       prob_next_online=prob_o)
        delta = (spec["v_max"] - spec["v_min"]) / float(n - 1)
        tz = (rewards.unsqueeze(-1) + discount * masks.unsqueeze(-1) * z.view(1, -1)).clamp(spec["v_min"], spec["v_max"]).unsqueeze(1)
        tgt = ((1 - (tz - z.view(1, -1, 1)).abs() / delta).clamp(0, 1) * prob_t[b, a_next, :].unsqueeze(1)).sum(-1)
    else:
        vec = L.qr_loss(out, out_t, actions, rewards, masks, discount)
        tgt = rewards.unsqueeze(-1) + discount * masks.unsqueeze(-1) * out_t[b, a_next, :]
    loss = vec.mean()
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    pre = [keep_t, keep] + ([keep_o] if keep_o else [])
    return dict(loss=float(loss.detach()), loss_vec=vec.detach().numpy(), q_next=q_next.numpy(), target=tgt.detach().numpy(),
                a_next=a_next.numpy(), grads={k: g.numpy() for k, g in zip(names, grads)},
                argmax_margin=float((q_choice[:, 1] - q_choice[:, 0]).abs().min()),
                min_preact=float(min(min(np.abs(d["z1"].numpy()).min(), np.abs(d["z2"].numpy()).min()) for d in pre)))


def update(params, target, ring, idx, discount, gradient_clip, lr, spec, double_q=False, gate="relu", square_avg=None):
    """One update on the ring's rows at idx -> (new parameters, dict of loss_and_grads' fields and square_avg)."""
    out = loss_and_grads(params, target, minibatch(ring, idx), discount, spec, double_q, gate)
    new, sq = rmsprop_step(params, out["grads"], gradient_clip, lr, square_avg=square_avg)
    out["square_avg"] = sq
    return new, out


def agent_run(init, env, cfg, rs, eps, n_steps, dtype=F64, target0=None):
    """dqn_feature_restatement.agent_run over this module's act and update; cfg carries `spec` besides dqn_feature's fields.
    argmax_margin: the smallest margin of EVERY update's a_next choices (dqn_feature's keeps double_q's alone)."""
    spec = cfg["spec"]
    saved = D.act, D.update
    margins = []

    def _update(params, target, ring, idx, discount, clip, lr, double_q, gate, sq):
        new, u = update(params, target, ring, idx, discount, clip, lr, spec, double_q, gate, sq)
        margins.append(u["argmax_margin"])
        return new, u
    D.act = lambda params, env_, raw, k_len, explore, rand, ring, pos, gate="relu", step0=0, dtype=F64: act(
        params, env_, raw, k_len, explore, rand, ring, pos, spec, gate=gate, step0=step0, dtype=dtype)
    D.update = _update
    try:
        out = _D_AGENT_RUN(init, env, cfg, rs, eps, n_steps, dtype=dtype, target0=target0)
        out["argmax_margin"] = min(margins) if margins else float("inf")
        return out
    finally:
        D.act, D.update = saved
