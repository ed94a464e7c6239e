"""DDPGAgent / TD3Agent with `config.fused_dpg_env` on (deeprl_amd/dpg_env.py: the environment on the device, one acting launch per
transition that writes the ring row) against the same agents with the switch off, `config.fused_dpg_update` on in both: 40 steps
over a replay of 24 slots (the ring wraps), warm_up 8, batch 8, (32, 24) networks.  Both paths run the same kernels on the same
data, so everything is compared to the bit: the ring, the drawn indices, the episode lines, np.random's tail, the parameters."""
import numpy as np
import pytest
import torch

from feature_kernel_harness import _bits, _Rec, dra  # noqa: F401

pytestmark = pytest.mark.gpu

STEPS, CAP, BATCH, WARM = 40, 24, 8, 8


def _agent(d, kind, game, device, horizon, monkeypatch, x0=None):
    import deeprl_amd.agents as agents_mod
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    d.random_seed(3)
    c = d.Config()
    c.merge(dict(game=game, log_level=0, tag="t", fused_dpg_update=True, fused_dpg_env=device, episode_drain_interval=7))
    c.task_fn = lambda: d.Task(c.game, seed=5, synthetic_done_period=horizon)
    c.eval_env = d.Task(c.game, seed=6, synthetic_done_period=horizon)
    adam = lambda p: torch.optim.Adam(p, lr=1e-3)
    body = lambda n: d.FCBody(n, (32, 24), gate=torch.relu)
    if kind == "ddpg":
        c.network_fn = lambda: d.DeterministicActorCriticNet(c.state_dim, c.action_dim, actor_body=body(c.state_dim),
                                                             critic_body=body(c.state_dim + c.action_dim), actor_opt_fn=adam,
                                                             critic_opt_fn=adam)
        c.replay_fn = lambda: d.UniformReplay(memory_size=CAP, batch_size=BATCH)
        c.random_process_fn = lambda: d.OrnsteinUhlenbeckProcess(size=(c.action_dim,), std=d.LinearSchedule(0.2), x0=x0)
    else:
        c.network_fn = lambda: d.TD3Net(c.action_dim, actor_body_fn=lambda: body(c.state_dim),
                                        critic_body_fn=lambda: body(c.state_dim + c.action_dim), actor_opt_fn=adam, critic_opt_fn=adam)
        c.replay_fn = lambda: d.ReplayWrapper(d.UniformReplay, dict(memory_size=CAP, batch_size=BATCH))
        c.random_process_fn = lambda: d.GaussianProcess(size=(c.action_dim,), std=d.LinearSchedule(0.1))
        c.td3_noise, c.td3_noise_clip, c.td3_delay = 0.2, 0.5, 2
    c.discount, c.warm_up, c.target_network_mix, c.max_steps = 0.99, WARM, 5e-3, int(1e6)
    agent = (d.DDPGAgent if kind == "ddpg" else d.TD3Agent)(c)
    return agent, rec


def _run(d, kind, game, device, horizon, monkeypatch):
    import deeprl_amd.replay as replay_mod
    drawn = []
    real = getattr(replay_mod.draw_uniform_indices, "_real", replay_mod.draw_uniform_indices)
    spy = lambda *a: drawn.append(np.array(real(*a))) or drawn[-1]
    spy._real = real
    monkeypatch.setattr(replay_mod, "draw_uniform_indices", spy)
    agent, rec = _agent(d, kind, game, device, horizon, monkeypatch)
    lines = []
    monkeypatch.setattr(agent, "log_train_return", lambda ret, at: lines.append((int(at), float(ret))))
    for _ in range(STEPS):
        agent.step()
    agent.drain_episodes()
    torch.cuda.synchronize()
    ring = getattr(agent.replay, "replay", agent.replay)
    out = dict(ring=[t.cpu().numpy().copy() for t in ring._ring.arrays()], pos=(ring.pos, ring.size()), drawn=drawn, lines=lines,
               tail=float(np.random.rand()), params=[p.detach().cpu().numpy().copy() for p in agent.network.parameters()],
               target=[p.detach().cpu().numpy().copy() for p in agent.target_network.parameters()],
               on_device=agent._fused_env() is not None, warnings=list(rec.warnings), total=agent.total_steps)
    if out["on_device"]:
        agent._fused_env().check()
    agent.close()
    return out


@pytest.mark.parametrize("game,horizon", [("classic-Pendulum-v0", 5), ("synthetic-continuous-HalfCheetah", 6)], ids=["pendulum", "synthetic"])
@pytest.mark.parametrize("kind", ["ddpg", "td3"])
def test_device_step_equals_host_step_bit_for_bit(dra, monkeypatch, kind, game, horizon):  # noqa: F811
    host = _run(dra, kind, game, False, horizon, monkeypatch)
    dev = _run(dra, kind, game, True, horizon, monkeypatch)
    assert not host["on_device"] and dev["on_device"] and not dev["warnings"], dev["warnings"]
    assert host["total"] == dev["total"] == STEPS and host["pos"] == dev["pos"] == (STEPS % CAP, CAP)
    for name, a, b in zip(("frames", "actions", "rewards", "masks"), host["ring"], dev["ring"]):
        assert np.array_equal(a, b), name
    assert len(host["drawn"]) == len(dev["drawn"]) > 0 and all(np.array_equal(a, b) for a, b in zip(host["drawn"], dev["drawn"]))
    assert host["lines"] == dev["lines"] and len(host["lines"]) >= 3
    assert host["tail"] == dev["tail"]
    for which in ("params", "target"):
        for i, (a, b) in enumerate(zip(host[which], dev[which])):
            assert np.array_equal(_bits(a), _bits(b)), (which, i, float(np.abs(a - b).max()))


def test_switch_on_but_ineligible_keeps_the_host_path_with_one_warning(dra, monkeypatch):  # noqa: F811
    """A MeanStdNormalizer on the states: the reason is logged once and the agent steps on the host."""
    agent, rec = _agent(dra, "ddpg", "classic-Pendulum-v0", True, 5, monkeypatch)
    agent.config.state_normalizer = dra.MeanStdNormalizer()
    for _ in range(3):
        agent.step()
    mine = [w for w in rec.warnings if "fused_dpg_env" in w]
    assert agent._fused_env() is None and len(mine) == 1 and "state normaliser" in mine[0] and agent.total_steps == 3
    agent.close()
