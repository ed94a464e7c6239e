"""CPU tests of the device-resident DDPG / TD3 step's host side (no GPU): envs.Pendulum against csrc/pendulum_env.h compiled into a
host program, its sine / cosine, clipping and wrapping, Task('classic-Pendulum-v0'), the ctypes mirror of dra_dpg_env_act_io, the
zoo's ddpg_continuous / td3_continuous against the reference's recorded Configs (tests/golden/crosscheck_dpg.json), dpg_env.why_not's
refusals and the default configuration."""
import ctypes
import json
import math
import os
import shutil
import subprocess
import types
import warnings

import numpy as np
import pytest

from golden import crosscheck_dpg_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_task_builds_the_pendulum_without_a_warning():
    from deeprl_amd.envs import Box, Pendulum, Task
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        task = Task('classic-Pendulum-v0', seed=4, synthetic_done_period=7)
    env = task.env.envs[0]
    assert type(env) is Pendulum and env.horizon == 7 and env.seed == 4 and task.env.num_envs == 1
    assert (task.state_dim, task.action_dim) == (3, 1) and isinstance(task.action_space, Box)
    assert (task.action_space.low, task.action_space.high, task.action_space.shape) == (-1.0, 1.0, (1,))
    assert Task('classic-Pendulum-v0', seed=4).env.envs[0].horizon == 200
    obs = task.reset()
    assert np.asarray(obs).shape == (1, 3) and np.asarray(obs).dtype == np.float64
    rets, total = [], 0.0
    for t in range(14):
        obs, r, done, info = task.step(np.asarray([[0.3]]))
        total += float(r[0])
        assert bool(done[0]) == (t % 7 == 6) and (info[0]['episodic_return'] is not None) == bool(done[0])
        if done[0]:
            rets.append(info[0]['episodic_return'])
    assert len(rets) == 2 and rets[0] < 0 and abs(sum(rets) - total) < 1e-9


def test_half_angle_sine_and_cosine_stay_within_4e15_of_libm():
    from deeprl_amd.envs import pendulum_sincos
    worst = 0.0
    for th in np.concatenate([np.linspace(-math.pi, math.pi, 20001), [-math.pi, math.pi, 0.0, 1e-9, -1e-9]]):
        s, c = pendulum_sincos(float(th))
        worst = max(worst, abs(s - math.sin(th)), abs(c - math.cos(th)))
    print("worst sine / cosine error %.3e" % worst)
    assert worst <= 4e-15


def test_velocity_is_clipped_and_the_angle_wraps():
    from deeprl_amd.envs import Pendulum
    env = Pendulum(0, horizon=10 ** 6)
    env.reset()
    env.s = np.asarray([1.5, 7.9])                   # falling with full torque: the velocity would pass 8
    env.step([1.0])
    assert env.s[1] == 8.0
    env.s = np.asarray([-1.5, -7.9])
    env.step([-5.0])                                 # (the action is clipped to -1)
    assert env.s[1] == -8.0
    env.s = np.asarray([3.1, 8.0])                   # over +pi: comes back in at -pi + ...
    obs, reward, _, _ = env.step([0.0])
    assert -Pendulum.PI <= env.s[0] < -2.7 and reward == -((3.1 * 3.1) + 0.1 * 64.0)
    env.s = np.asarray([-3.1, -8.0])
    env.step([0.0])
    assert 2.7 < env.s[0] < Pendulum.PI
    seen = []
    for _ in range(400):                             # spinning: the state stays wrapped, the observation on the unit circle
        obs, _, _, _ = env.step([1.0])
        seen.append(env.s[0])
        assert -Pendulum.PI <= env.s[0] < Pendulum.PI and abs(env.s[1]) <= 8.0 and abs(obs[0] ** 2 + obs[1] ** 2 - 1.0) < 1e-14
    assert min(seen) < -3.0 and max(seen) > 3.0


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_pendulum_header_host_build_equals_envs_pendulum_to_the_bit(tmp_path):
    """csrc/pendulum_env.h's __host__ __device__ functions in a host program: 1000 steps under two seeds and horizons 1, 3 and 200
    print the bits envs.Pendulum produces -- observation, reward, terminal, the finished episode's return, the state."""
    from deeprl_amd.envs import Pendulum
    src = tmp_path / "probe.cpp"
    src.write_text(r'''
#include "deeprl_amd/csrc/pendulum_env.h"
#include <stdio.h>
#include <string.h>
static unsigned long long bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }
int main() {
  const uint64_t seeds[2] = {3, 1234567};
  const int64_t horizons[3] = {1, 3, 200};
  for (int si = 0; si < 2; ++si)
    for (int hi = 0; hi < 3; ++hi) {
      PendulumState st; int64_t c = 0; int32_t steps = 0; double ret = 0.0;
      pendulum_reset(st, seeds[si], c);
      for (int t = 0; t < 1000; ++t) {
        const double a = (double)((t * 7 + si * 3) % 23) * 0.125 - 1.375;
        double reward = 0.0, ended = 0.0, obs[3];
        const bool done = pendulum_step(st, c, steps, ret, seeds[si], a, horizons[hi], reward, ended);
        pendulum_observe(st, obs);
        printf("%d %d %d %llx %llx %llx %llx %llx %llx %llx\n", si, hi, done ? 1 : 0, bits(reward), bits(ended), bits(obs[0]), bits(obs[1]),
               bits(obs[2]), bits(st.th), bits(st.thd));
      }
    }
  return 0;
}
''')
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "probe")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-ffp-contract=off", "-I", ROOT, str(src), "-o", exe],
                   check=True, capture_output=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(lines) == 6000
    bits = lambda x: int(np.asarray([x], dtype=np.float64).view(np.uint64)[0])
    it = iter(lines)
    for si, seed in enumerate((3, 1234567)):
        for hi, horizon in enumerate((1, 3, 200)):
            env = Pendulum(seed, horizon=horizon)
            env.reset()
            dones = 0
            for t in range(1000):
                a = float((t * 7 + si * 3) % 23) * 0.125 - 1.375
                obs, reward, done, info = env.step([a])
                ended = info['episodic_return'] if done else 0.0
                if done:
                    obs = env.reset()
                    dones += 1
                f = next(it).split()
                assert (int(f[0]), int(f[1]), int(f[2])) == (si, hi, int(done)), (seed, horizon, t)
                want = [reward, ended, obs[0], obs[1], obs[2], env.s[0], env.s[1]]
                assert [int(x, 16) for x in f[3:]] == [bits(x) for x in want], (seed, horizon, t)
            assert dones == 1000 // horizon


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_act_io_mirror_matches_the_header(tmp_path):
    from deeprl_amd import dpg_env
    names = [f[0] for f in dpg_env.ActIO._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "include/deeprl_amd.h"', 'int main(void) {',
           '  printf("%zu\\n", sizeof(dra_dpg_env_act_io));']
    src += ['  printf("%%zu\\n", offsetof(dra_dpg_env_act_io, %s));' % f for f in names]
    src += ['  return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", str(c), "-I", ROOT, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(dpg_env.ActIO)
    assert got[1:] == [getattr(dpg_env.ActIO, n).offset for n in names]


@pytest.mark.parametrize("name", sorted(D.DPG_GAMES))
def test_zoo_entry_equals_reference_example(name):
    import deeprl_amd as d
    from deeprl_amd import zoo
    with open(D.CROSSCHECK_DPG_JSON) as f:
        rec = json.load(f)["zoo"][name]
    d.select_device(-1)
    assert rec["agent"] == zoo.ZOO[name]["agent"]
    np.random.seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want, have = rec["config"], D.describe_dpg_config(zoo.config(name, game=D.DPG_GAMES[name]))
    assert set(want) == set(have), (sorted(set(want) ^ set(have)))
    for k in sorted(want):
        assert want[k] == have[k], "%s.%s: reference %s, zoo %s" % (name, k, want[k], have[k])
    assert callable(getattr(zoo, name))


# ------------------------------------------------------------------------------------------------ why_not
def _fake_agent(**over):
    """What dpg_env.why_not reads of an eligible DDPGAgent, without a device: the fused update's own check is replaced."""
    import torch

    from deeprl_amd import nets as N
    from deeprl_amd.envs import Task
    from deeprl_amd.normalizers import RescaleNormalizer
    from deeprl_amd.random_process import OrnsteinUhlenbeckProcess
    from deeprl_amd.replay import UniformReplay
    from deeprl_amd.support import LinearSchedule
    adam = lambda p: torch.optim.Adam(p, lr=1e-3)
    cfg = types.SimpleNamespace(fused_dpg_env=True, fused_dpg_update=True, state_normalizer=RescaleNormalizer(),
                                reward_normalizer=RescaleNormalizer(), device_env=True)
    agent = types.SimpleNamespace(
        config=cfg, task=Task('classic-Pendulum-v0', seed=1), state=None, total_steps=0,
        network=N.DeterministicActorCriticNet(3, 1, adam, adam, actor_body=N.FCBody(3, (32, 24)), critic_body=N.FCBody(4, (32, 24))),
        random_process=OrnsteinUhlenbeckProcess(size=(1,), std=LinearSchedule(0.2)), replay=UniformReplay(memory_size=24, batch_size=8))
    for k, v in over.items():
        setattr(cfg if hasattr(cfg, k) else agent, k, v)
    return agent


def _why(agent, monkeypatch, update=None, supported=True, device='cuda'):
    from deeprl_amd import device_env, dpg_env
    with monkeypatch.context() as m:        # (a device only while why_not looks: the fake agent's modules are built on the CPU)
        m.setattr(device_env.Config, "DEVICE", types.SimpleNamespace(type=device), raising=False)
        return dpg_env.why_not(agent, supported_fn=lambda *a: supported, update_why_not=lambda a: update)


def test_why_not_names_each_refusal(monkeypatch):
    from deeprl_amd.envs import Task
    from deeprl_amd.normalizers import MeanStdNormalizer, RescaleNormalizer
    from deeprl_amd.random_process import GaussianProcess, OrnsteinUhlenbeckProcess
    from deeprl_amd.replay import PrioritizedReplay, UniformReplay
    from deeprl_amd.support import LinearSchedule
    assert _why(_fake_agent(), monkeypatch) is None
    assert _why(_fake_agent(random_process=GaussianProcess(size=(1,), std=LinearSchedule(0.1))), monkeypatch) is None
    assert "fused_dpg_env is not on" in _why(_fake_agent(fused_dpg_env=False), monkeypatch)
    assert "fused_dpg_env is not on" in _why(_fake_agent(fused_dpg_env=1), monkeypatch)
    assert "fused update is not available (the optimisers" in _why(_fake_agent(), monkeypatch, update="the optimisers")
    assert "not one envs.Pendulum" in _why(_fake_agent(task=Task('classic-CartPole-v0', seed=1)), monkeypatch)
    assert "not one envs.Pendulum" in _why(_fake_agent(task=Task('classic-Pendulum-v0', num_envs=2, seed=1)), monkeypatch)
    assert "not one envs.Pendulum" in _why(_fake_agent(device_env=False), monkeypatch)
    stepped = Task('classic-Pendulum-v0', seed=1)
    stepped.reset()
    stepped.step(np.zeros((1, 1)))
    assert "already been stepped" in _why(_fake_agent(task=stepped), monkeypatch)
    assert "already been stepped" in _why(_fake_agent(state=np.zeros((1, 3))), monkeypatch)
    assert "state normaliser" in _why(_fake_agent(state_normalizer=MeanStdNormalizer()), monkeypatch)
    assert "state normaliser" in _why(_fake_agent(state_normalizer=RescaleNormalizer(0.5)), monkeypatch)
    assert "reward normaliser" in _why(_fake_agent(reward_normalizer=RescaleNormalizer(0.1)), monkeypatch)

    class Mine(OrnsteinUhlenbeckProcess):
        pass
    assert "random process is not exactly" in _why(_fake_agent(random_process=Mine(size=(1,), std=LinearSchedule(0.2))), monkeypatch)
    assert "one value per action dimension" in _why(_fake_agent(random_process=GaussianProcess(size=(2,), std=LinearSchedule(0.1))), monkeypatch)
    assert "one-step UniformReplay" in _why(_fake_agent(replay=PrioritizedReplay(memory_size=24, batch_size=8)), monkeypatch)
    assert "one-step UniformReplay" in _why(_fake_agent(replay=UniformReplay(memory_size=24, batch_size=8, n_step=2)), monkeypatch)
    assert "fewer than two slots" in _why(_fake_agent(replay=UniformReplay(memory_size=1, batch_size=1)), monkeypatch)
    assert "dra_dpg_env_act_supported refuses" in _why(_fake_agent(), monkeypatch, supported=False)
    assert "no device" in _why(_fake_agent(), monkeypatch, device='cpu')


def test_supported_table_needs_no_gpu():
    from deeprl_amd import dpg_env
    assert dpg_env.supported(dpg_env.ENV_PENDULUM, 3, 1, 400, 300, 1) and dpg_env.supported(dpg_env.ENV_SYNTHETIC, 17, 6, 400, 300, 2)
    assert not dpg_env.supported(dpg_env.ENV_PENDULUM, 17, 6, 400, 300, 1) and not dpg_env.supported(dpg_env.ENV_SYNTHETIC, 17, 6, 600, 300, 1)


def test_default_config_stays_on_the_host_path():
    import deeprl_amd as d
    from deeprl_amd import agents, zoo
    c = d.Config()
    assert getattr(c, 'fused_dpg_env', False) is False
    d.select_device(-1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = zoo.config("ddpg_continuous", game="classic-Pendulum-v0")
    assert getattr(cfg, 'fused_dpg_env', False) is False
    fake = types.SimpleNamespace(config=cfg)
    assert agents._DeterministicPolicyAgent._fused_env(fake) is None and fake._dpg_env is None
