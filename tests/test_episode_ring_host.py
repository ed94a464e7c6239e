"""device_env.EpisodeRing, the ONE host reader of the device cart-poles' episode ring (A2CAgent: a stamp per sampler step,
t_len + 1 per rollout; NStepDQNAgent: a stamp per rollout step), against a fake task whose drain() returns canned
(stamp, environment, return) rows.  No device, no library; everything is compared exactly."""
import types

import pytest

from deeprl_amd.device_env import EpisodeRing


class _Task:
    """What EpisodeRing reads of a DeviceCartPoleVec."""

    def __init__(self):
        self.pending, self.drains, self.loaded = [], 0, None

    def drain(self):
        self.drains += 1
        out, self.pending = self.pending, []
        return out

    def state_dict(self):
        return dict(env_state="arrays", drained=7)

    def load_state_dict(self, d):
        self.loaded = d


class _Agent:
    """What EpisodeRing reads of its agent."""

    def __init__(self, **cfg):
        self.task, self.total_steps, self.lines = _Task(), 0, []
        self.config = types.SimpleNamespace(**cfg)

    def log_train_return(self, ret, at):
        self.lines.append((at, ret))


def _rollout(agent, ring, t_len, n):
    """What an agent step does around the launch."""
    ring.begin(t_len)
    agent.total_steps += t_len * n
    ring.end()


@pytest.mark.parametrize("extra", [1, 0], ids=["stride_t_len_plus_1", "stride_t_len"])
def test_step_numbers_of_first_last_and_second_rollout_rows(extra):
    """total_steps at the start of the episode's rollout + t * N + environment, for a row at the first step, at the last step and
    at the first step of the second rollout; stamps start where the kernel's counter stood (100) and total_steps at 1000."""
    t_len, n, s0 = 5, 3, 100
    agent = _Agent(episode_drain_interval=1000)
    ring = EpisodeRing(agent, extra, n)
    ring.stamp, agent.total_steps = s0, 1000
    _rollout(agent, ring, t_len, n)
    _rollout(agent, ring, t_len, n)
    assert ring.stamp == s0 + 2 * (t_len + extra) and ring.anchor == (s0, 1000, t_len)
    stride = t_len + extra
    agent.task.pending = [(s0 + 0, 2, 11.0), (s0 + t_len - 1, 0, 12.0), (s0 + stride + 0, 1, 13.0)]
    out = ring.drain()
    assert out == [(1000 + 0 * n + 2, 11.0), (1000 + (t_len - 1) * n + 0, 12.0), (1000 + t_len * n + 1, 13.0)]
    assert agent.lines == out and list(ring.log) == out


def test_nothing_is_drained_before_the_first_rollout():
    agent = _Agent()
    ring = EpisodeRing(agent, 1, 4)
    agent.task.pending = [(0, 0, 1.0)]
    assert ring.drain() == [] and ring.episodes() == [] and agent.task.drains == 0 and agent.lines == []


def test_a_changed_rollout_length_drains_first_and_re_anchors():
    n = 2
    agent = _Agent(episode_drain_interval=1000)
    ring = EpisodeRing(agent, 1, n)
    _rollout(agent, ring, 5, n)                     # stamps 0..5, steps 0..9
    agent.task.pending = [(4, 1, 21.0)]             # appended under t_len 5
    ring.begin(3)                                   # drains under the OLD anchor, then anchors at (6, 10, 3)
    assert agent.lines == [(0 + 4 * n + 1, 21.0)] and ring.anchor == (6, 10, 3) and ring.stamp == 6 + 4
    agent.total_steps += 3 * n
    agent.task.pending = [(6 + 2, 0, 22.0)]
    assert ring.drain() == [(10 + 2 * n + 0, 22.0)]
    ring.begin(3)                                   # same length: no drain, the anchor stays
    assert ring.anchor == (6, 10, 3) and agent.task.drains == 2


def test_episodes_returns_each_pair_once():
    agent = _Agent(episode_drain_interval=1000)
    ring = EpisodeRing(agent, 0, 1)
    _rollout(agent, ring, 4, 1)
    agent.task.pending = [(1, 0, 5.0), (3, 0, 6.0)]
    assert ring.drain() == [(1, 5.0), (3, 6.0)]
    agent.task.pending = [(2, 0, 7.0)]              # (episodes() drains what is pending and adds it)
    assert ring.episodes() == [(1, 5.0), (3, 6.0), (2, 7.0)]
    assert ring.episodes() == [] and ring.drain() == []


def test_the_log_keeps_the_newest_16384():
    agent = _Agent(episode_drain_interval=1000)
    ring = EpisodeRing(agent, 0, 1)
    assert EpisodeRing.LOG == 16384
    _rollout(agent, ring, 20000, 1)
    agent.task.pending = [(s, 0, float(s)) for s in range(16384 + 10)]
    ring.drain()
    out = ring.episodes()
    assert len(out) == 16384 and out[0] == (10, 10.0) and out[-1] == (16384 + 9, 16384.0 + 9)


def test_the_drain_interval_fires_on_its_multiples_only():
    agent = _Agent(episode_drain_interval=3)
    ring = EpisodeRing(agent, 1, 1)
    fired = []
    for step in range(1, 11):
        before = agent.task.drains
        _rollout(agent, ring, 2, 1)
        if agent.task.drains != before:
            fired.append(step)
    assert fired == [3, 6, 9] and ring.steps == 10
    default = EpisodeRing(_Agent(), 1, 1)           # (no key in the config: every 64 steps)
    for _ in range(128):
        _rollout(default.agent, default, 2, 1)
    assert default.agent.task.drains == 2


@pytest.mark.parametrize("parent_file", [
    dict(seed=12345, step=42, envs=dict(env_state="saved", drained=3)),         # <file>.sampler as A2CAgent.save wrote it
    dict(envs=dict(env_state="saved", drained=3), step=42),                     # <file>.envs as NStepDQNAgent.save wrote it
    dict(seed=12345, step=42),                                                  # a .sampler from before the ring: no arrays
], ids=["sampler", "envs", "sampler_without_envs"])
def test_save_and_load_go_through_the_keys_the_side_files_have(parent_file):
    agent = _Agent(episode_drain_interval=1000)
    ring = EpisodeRing(agent, 1, 2)
    assert ring.state_dict() == dict(envs=dict(env_state="arrays", drained=7))
    _rollout(agent, ring, 5, 2)
    agent.task.pending = [(1, 1, 3.0)]
    ring.load_state_dict(parent_file)               # what was pending is logged under the old anchor first
    assert agent.lines == [(1 * 2 + 1, 3.0)]
    assert ring.stamp == 42 and ring.anchor is None and agent.task.loaded == parent_file.get("envs")
    agent.total_steps = 500
    _rollout(agent, ring, 5, 2)                     # the next rollout anchors at the loaded counter
    assert ring.anchor == (42, 500, 5)
    agent.task.pending = [(42 + 3, 0, 9.0)]
    assert ring.drain() == [(500 + 3 * 2 + 0, 9.0)]
