"""The reference's own DDPGAgent / TD3Agent over envs.Pendulum, replayed: tests/golden/dpg_pendulum/steps.npz
(tests/golden/make_golden_dpg_pendulum.py --steps) holds 20 recorded agent steps each -- warm_up 8, so a dozen updates and one more,
minibatches of 8, (32, 24) relu networks, episodes of 5 steps, td3_noise 0 -- from recorded initial weights.  The product's agents run
the same steps from the same weights and seeds with `fused_dpg_update` on, on the host step and on the device step
(`fused_dpg_env`): same total_steps and np.random consumption, the replay holds the reference's transitions (masks exactly; states,
actions and rewards within fp32 rounding of the actor: rtol 1e-5 / atol 1e-6, test_fused_agents_match_reference_run's bar), and
the online and target parameters land on the reference's within the tolerances tests/golden/ddpg_td3 uses (rtol 2e-4 / atol 2e-5).
It is what compares the one-dimensional action space (S = 3, A = 1) through the fused update with the reference."""
import os
import random

import numpy as np
import pytest
import torch
from parity_log import record_parity

from feature_kernel_harness import _Rec, dra  # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dpg_pendulum", "steps.npz")


def _agent(d, g, tag, device, monkeypatch):
    import deeprl_amd.agents as agents_mod
    steps, warm, batch, cap, h1, h2, horizon, task_seed = [int(x) for x in g["hyper"]]
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    c = d.Config()
    c.merge(dict(game="classic-Pendulum-v0", log_level=0, tag=tag, fused_dpg_update=True, fused_dpg_env=device))
    c.task_fn = lambda: d.Task(c.game, seed=task_seed, synthetic_done_period=horizon)
    c.eval_env = c.task_fn()
    adam = lambda p: torch.optim.Adam(p, lr=1e-3)
    body = lambda n: d.FCBody(n, (h1, h2), gate=torch.relu)
    if tag == "ddpg":
        c.network_fn = lambda: d.DeterministicActorCriticNet(3, 1, actor_body=body(3), critic_body=body(4), actor_opt_fn=adam,
                                                             critic_opt_fn=adam)
        c.replay_fn = lambda: d.UniformReplay(memory_size=cap, batch_size=batch)
        c.random_process_fn = lambda: d.OrnsteinUhlenbeckProcess(size=(1,), std=d.LinearSchedule(0.2))
        cls = d.DDPGAgent
    else:
        c.network_fn = lambda: d.TD3Net(1, actor_body_fn=lambda: body(3), critic_body_fn=lambda: body(4), actor_opt_fn=adam,
                                        critic_opt_fn=adam)
        c.replay_fn = lambda: d.ReplayWrapper(d.UniformReplay, dict(memory_size=cap, batch_size=batch), False)
        c.random_process_fn = lambda: d.GaussianProcess(size=(1,), std=d.LinearSchedule(0.1))
        c.td3_noise, c.td3_noise_clip, c.td3_delay = 0.0, 0.5, 2
        cls = d.TD3Agent
    c.discount, c.warm_up, c.target_network_mix, c.max_steps = 0.99, warm, 5e-3, int(1e6)
    torch.manual_seed(7)
    np.random.seed(17)
    random.seed(17)
    agent = cls(c)
    agent.network.load_state_dict({k: torch.from_numpy(g[tag + "_init_" + k]) for k in agent.network.state_dict().keys()})
    agent.target_network.load_state_dict(agent.network.state_dict())
    return agent, steps, warm


@pytest.mark.parametrize("device", [False, True], ids=["host_step", "device_step"])
@pytest.mark.parametrize("tag", ["ddpg", "td3"])
def test_recorded_reference_steps_replayed(dra, monkeypatch, tag, device):  # noqa: F811
    g = np.load(FIXTURE)
    agent, steps, warm = _agent(dra, g, tag, device, monkeypatch)
    for _ in range(steps):
        agent.step()
    torch.cuda.synchronize()
    k = tag + "_"
    fused = agent._fused_dpg()
    updates = steps - warm + 1
    assert (agent._fused_env() is not None) == device and fused is not None
    assert fused.t_critic == updates and fused.t_actor == (updates if tag == "ddpg" else sum(t % 2 for t in range(warm, steps + 1)))
    assert agent.total_steps == int(g[k + "total_steps"]) == steps
    assert np.array_equal(np.random.randint(0, 1 << 30, size=4), g[k + "rng_tail"])
    rp = getattr(agent.replay, "replay", agent.replay)
    n = rp.size()
    assert n == steps
    frames, actions, rewards, masks = [t.cpu().numpy() for t in rp._ring.arrays()]
    assert np.array_equal(masks[:n], g[k + "replay_mask"]) and (masks[:n] == 0).any()
    for name, got in (("state", frames.view(np.float64).reshape(-1, 3)[:n]), ("action", actions.view(np.float64).reshape(-1, 1)[:n]),
                      ("reward", rewards[:n])):
        np.testing.assert_allclose(got, g[k + "replay_" + name], rtol=1e-5, atol=1e-6, err_msg=name)
    # (the warm-up's transitions involve no network: the same bits)
    assert np.array_equal(actions.view(np.float64).reshape(-1, 1)[:warm], g[k + "replay_action"][:warm])
    assert np.array_equal(frames.view(np.float64).reshape(-1, 3)[:warm + 1], g[k + "replay_state"][:warm + 1])
    worst = 0.0
    for which, net in (("final_", agent.network), ("target_", agent.target_network)):
        for name, v in net.state_dict().items():
            got, want = v.cpu().numpy(), g[k + which + name]
            print("%s%s: max abs difference %.3e" % (which, name, float(np.abs(got - want).max())))
            np.testing.assert_allclose(got, want, rtol=2e-4, atol=2e-5, err_msg=which + name)
            worst = max(worst, float(np.max(np.abs(got - want) / (2e-5 + 2e-4 * np.abs(want)))))
    record_parity("dpg_env recorded reference steps %s %s (fraction of the bar)" % (tag, "device" if device else "host"), params=worst)
    agent.close()
