"""Restatement of what the evaluation kernels (csrc/eval_act.h: dra_dqn_mlp_eval, dra_dist_mlp_eval, dra_rainbow_mlp_eval) and
DQNAgent.eval_episodes under config.fused_eval compute (TEST INFRASTRUCTURE ONLY): BaseAgent.py:60-77 over DummyVecEnv's auto
reset -- reset, q of the float32 observation in fp64, the first maximum, step, reset on done -- over envs.CartPole, which is
imported, not restated.  The forwards are the three feature restatements' (`forward_of`).  tests/test_eval_host.py pins it to
BaseAgent.eval_episodes of the project's own agents on the CPU and to the reference's DQNAgent.eval_episodes before a GPU test
leans on it."""
import numpy as np
import torch

import dist_feature_restatement as DR
import dqn_feature_restatement as QR
import rainbow_feature_restatement as RR

F64 = torch.float64
Q_BAR = 1e-5            # feature_kernel_harness._fraction's bar on q: this fraction of the largest |q|, floor 1.0
MARGIN_BARS = 100       # the smallest |q1 - q0| of a case must be this many bars: no argmax is a near tie


def forward_of(kind, gate="relu", spec=None, noise=None):
    """forward(p, obs) -> q [rows, 2] of a kind: 'dqn' (dqn_feature_restatement), 'dist' (dist_feature_restatement under `spec`),
    'rainbow' (rainbow_feature_restatement under `spec` and ONE raw noise dict, as tensors of the parameters' dtype)."""
    if kind == "dqn":
        return lambda p, obs: QR.forward(p, obs, gate)
    if kind == "dist":
        return lambda p, obs: DR.forward(p, obs, spec, gate)
    assert kind == "rainbow"
    return lambda p, obs: RR.forward(p, {k: torch.as_tensor(v, dtype=next(iter(p.values())).dtype) for k, v in noise.items()}, obs, spec, gate)


def evaluate(forward, params, env, n_episodes, dtype=F64):
    """n_episodes greedy episodes of `env` (an envs.CartPole, left where the last auto reset leaves it) under forward(p, obs).
    -> dict(returns [n] fp64, lengths [n] int32, q [steps, 2] fp64, steps, state (the environment's fp64 words), counter,
    ep_steps, ep_return, margin: the smallest |q1 - q0| seen, scale: the largest |q|)."""
    p = QR.to_t(params, dtype)
    returns, lengths, qs, margin = [], [], [], float("inf")
    with torch.no_grad():
        raw = env.reset()
        while len(returns) < n_episodes:
            q = forward(p, np.asarray(raw, dtype=np.float64).astype(np.float32)[None]).to(F64).numpy()[0]
            qs.append(q)
            margin = min(margin, float(abs(q[1] - q[0])))
            length = env.steps + 1
            raw, _, done, info = env.step(int(np.argmax(q)))
            if done:
                returns.append(float(info['episodic_return']))
                lengths.append(length)
                raw = env.reset()
    q = np.stack(qs)
    return dict(returns=np.asarray(returns, dtype=np.float64), lengths=np.asarray(lengths, dtype=np.int32), q=q, steps=len(qs),
                state=np.asarray(raw, dtype=np.float64), counter=int(env.c), ep_steps=int(env.steps), ep_return=float(env.ret),
                margin=margin, scale=float(np.abs(q).max()))


def q_bar(out):
    """The harness's bar on q for this run."""
    return Q_BAR * max(out["scale"], 1.0)


def comparable(out, horizon, both_ways=True):
    """Whether a greedy trajectory may be compared with an fp32 kernel's: no argmax within MARGIN_BARS bars of a tie, and --
    both_ways -- episodes that end by the horizon AND episodes that end by the pole or the cart."""
    if out["margin"] < MARGIN_BARS * q_bar(out):
        return False
    if not both_ways:
        return True
    return bool((out["lengths"] == horizon).any() and (out["lengths"] < horizon).any())
