#!/usr/bin/env python
"""Generates tests/golden/ddpg_td3/ddpg_td3_update.npz by running the REFERENCE's own code (tests/ref_shim.py):

  single DDPGAgent.step / TD3Agent.step updates (DDPG_agent.py:75-100, TD3_agent.py:72-108) on fake_envs.ContinuousTask, a few
  updates after warm-up (so that Adam's moments are not zero), at two sizes.  Per case -- ddpg, td3 on a policy step, td3 on a
  critic-only step -- the sampled minibatch (replay.sample wrapped), TD3's randn_like draw (wrapped), and online parameters,
  target parameters, Adam moments and step counts before and after.

The heads are scaled up as make_golden_a2c_continuous.py does, so that every term matters.  The generator asserts that each
batch has terminal and non-terminal rows, that TD3's noise clip binds on some but not all elements, that the action clamp
binds, and that every hidden layer of the online networks has both gated-off (dead) and live relu outputs on the batch.

Re-run:  python tests/golden/make_golden_ddpg_td3_update.py        (needs the reference checkout; GOLDEN_OUT redirects the output)
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from golden import make_golden as G  # noqa: E402  (loads the reference through tests/ref_shim.py)
import dpg_restatement as R  # noqa: E402
import fake_envs  # noqa: E402

ref = G.ref

# tag, (B, S, A, H1, H2), horizon of the fake task
SIZES = (("b8", (8, 5, 2, 16, 16), 3), ("b20", (20, 7, 3, 20, 12), 4))
# seeds for which the reference's run satisfies every assertion below (searched on the CPU)
SEEDS = {("b8", "ddpg"): 1, ("b8", "td3"): 5, ("b20", "ddpg"): 1, ("b20", "td3"): 1}
DISCOUNT, MIX, LR, TD3_NOISE, TD3_NOISE_CLIP, TD3_DELAY = 0.99, 5e-3, 1e-3, 0.2, 0.3, 2
HEAD_SCALE, ACTION_HEAD_SCALE = 300.0, 2000.0     # (the action head further: tanh has to come within the noise clip of +-1)
UPDATES_BEFORE = 3        # updates the agent has already made when the recorded ones start


def _agent(algo, dims, horizon, seed):
    b, s, a, h1, h2 = dims
    cfg = ref.Config()
    cfg.merge(dict(game="fake", log_level=0, tag=algo))
    cfg.task_fn = lambda: fake_envs.ContinuousTask(seed=seed, state_dim=s, action_dim=a, horizon=horizon)
    cfg.eval_env = cfg.task_fn()
    opt = lambda p: torch.optim.Adam(p, lr=LR)
    if algo == "ddpg":
        cfg.network_fn = lambda: ref.DeterministicActorCriticNet(
            s, a, actor_body=ref.FCBody(s, (h1, h2), gate=torch.relu), critic_body=ref.FCBody(s + a, (h1, h2), gate=torch.relu),
            actor_opt_fn=opt, critic_opt_fn=opt)
        cfg.replay_fn = lambda: ref.UniformReplay(memory_size=400, batch_size=b)
        cfg.random_process_fn = lambda: ref.OrnsteinUhlenbeckProcess(size=(a,), std=ref.LinearSchedule(0.2))
        cls = ref.DDPGAgent
    else:
        cfg.network_fn = lambda: ref.TD3Net(
            a, actor_body_fn=lambda: ref.FCBody(s, (h1, h2), gate=torch.relu),
            critic_body_fn=lambda: ref.FCBody(s + a, (h1, h2), gate=torch.relu), actor_opt_fn=opt, critic_opt_fn=opt)
        cfg.replay_fn = lambda: ref.ReplayWrapper(ref.UniformReplay, dict(memory_size=400, batch_size=b), False)
        cfg.random_process_fn = lambda: ref.GaussianProcess(size=(a,), std=ref.LinearSchedule(0.1))
        cfg.td3_noise, cfg.td3_noise_clip, cfg.td3_delay = TD3_NOISE, TD3_NOISE_CLIP, TD3_DELAY
        cls = ref.TD3Agent
    cfg.discount, cfg.warm_up, cfg.target_network_mix, cfg.max_steps = DISCOUNT, 3 * b, MIX, 1e5
    torch.manual_seed(seed)
    np.random.seed(seed + 10)
    random.seed(seed + 10)
    agent = cls(cfg)
    with torch.no_grad():
        for net in (agent.network, agent.target_network):
            for name, p in net.named_parameters():
                if name.startswith("fc_") and name.endswith("weight"):
                    p.mul_(ACTION_HEAD_SCALE if name.startswith("fc_action") else HEAD_SCALE)
    return agent


def _snapshot(out, key, agent):
    for n, v in agent.network.state_dict().items():
        out["%s_online_%s" % (key, n)] = v.detach().numpy().copy()
    for n, v in agent.target_network.state_dict().items():
        out["%s_target_%s" % (key, n)] = v.detach().numpy().copy()
    names = {id(p): n for n, p in agent.network.named_parameters()}
    for tag, opt in (("actor", agent.network.actor_opt), ("critic", agent.network.critic_opt)):
        step = 0
        for grp in opt.param_groups:
            for p in grp["params"]:
                st = opt.state.get(p, {})
                m, v = st.get("exp_avg"), st.get("exp_avg_sq")
                out["%s_m_%s" % (key, names[id(p)])] = (m if m is not None else torch.zeros_like(p)).detach().numpy().copy()
                out["%s_v_%s" % (key, names[id(p)])] = (v if v is not None else torch.zeros_like(p)).detach().numpy().copy()
                step = max(step, int(st.get("step", 0)))
        out["%s_t_%s" % (key, tag)] = np.asarray(step)


def _recorded_step(out, case, agent, n_critics):
    """One agent.step with replay.sample and torch.randn_like wrapped; snapshots before and after."""
    seen = {}
    raw_sample, raw_randn = agent.replay.sample, torch.randn_like

    def sample(*a, **k):
        tr = raw_sample(*a, **k)
        seen["batch"] = tr
        return tr

    def randn_like(x, *a, **k):
        nz = raw_randn(x, *a, **k)
        seen["a_next"], seen["noise"] = x.detach().numpy().copy(), nz.detach().numpy().copy()
        return nz

    _snapshot(out, case + "_before", agent)
    before = {k[len(case) + 1:]: v for k, v in out.items() if k.startswith(case + "_before_online_")}
    agent.replay.sample, torch.randn_like = sample, randn_like
    try:
        agent.step()
    finally:
        agent.replay.sample, torch.randn_like = raw_sample, raw_randn
    _snapshot(out, case + "_after", agent)
    tr = seen["batch"]
    batch = dict(state=np.asarray(tr.state, dtype=np.float64), action=np.asarray(tr.action, dtype=np.float64),
                 reward=np.asarray(tr.reward, dtype=np.float64).reshape(-1), next_state=np.asarray(tr.next_state, dtype=np.float64),
                 mask=np.asarray(tr.mask, dtype=np.float64).reshape(-1))
    for k, v in batch.items():
        out["%s_batch_%s" % (case, k)] = v
    out[case + "_total_steps"] = np.asarray(agent.total_steps)
    assert (batch["mask"] == 0).any() and (batch["mask"] == 1).any(), case
    if n_critics == 2:
        nz, a_next = seen["noise"], seen["a_next"]
        out[case + "_noise"] = nz
        bound = np.abs(nz * TD3_NOISE) > TD3_NOISE_CLIP
        assert bound.any() and not bound.all(), case
        moved = a_next + np.clip(nz * TD3_NOISE, -TD3_NOISE_CLIP, TD3_NOISE_CLIP)
        assert (np.abs(moved) > 1.0).any(), case
    # every hidden layer of the online networks has gated-off (dead) and live relu outputs on this batch
    p = R.canonical(before, n_critics, prefix="before_online_")
    s, a = R.f64(batch["state"]), R.f64(batch["action"])
    for role, x in [("a", s)] + [("c%d" % c, torch.cat([s, a], dim=1)) for c in range(n_critics)]:
        h1 = torch.relu(x @ p[role + ".w1"].t() + p[role + ".b1"])
        h2 = torch.relu(h1 @ p[role + ".w2"].t() + p[role + ".b2"])
        for h in (h1, h2):
            assert (h == 0).any() and (h > 0).any(), (case, role)


def gen():
    out = {}
    restore = G._quiet_logger()
    try:
        for tag, dims, horizon in SIZES:
            for algo in ("ddpg", "td3"):
                agent = _agent(algo, dims, horizon, SEEDS[tag, algo])
                warm = agent.config.warm_up
                for _ in range(warm - 1 + UPDATES_BEFORE):
                    agent.step()
                if algo == "ddpg":
                    _recorded_step(out, "%s_ddpg" % tag, agent, 1)
                else:
                    for _ in range(2):
                        policy = bool((agent.total_steps + 1) % TD3_DELAY)
                        _recorded_step(out, "%s_td3_%s" % (tag, "policy" if policy else "critic"), agent, 2)
                out["%s_dims" % tag] = np.asarray(dims)
    finally:
        restore()
    out["hyper"] = np.asarray([DISCOUNT, MIX, LR, TD3_NOISE, TD3_NOISE_CLIP, TD3_DELAY])
    return out


def main():
    out_dir = os.path.join(os.environ.get("GOLDEN_OUT", HERE), "ddpg_td3")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "ddpg_td3_update.npz")
    np.savez_compressed(path, **gen())
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
