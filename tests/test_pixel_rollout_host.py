"""Host side of what the pixel rollouts and the staged uploads share (no GPU): pixel_rollout's trunk and head checks, support.StagedUpload
on the CPU device and the order of its reuse guard, and BaseAgent._account_rollout against the per-step loop it stands in for."""
import numpy as np
import pytest
import torch


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    import deeprl_amd as d
    device = d.Config.DEVICE
    d.select_device(-1)
    yield
    d.Config.DEVICE = device


def _body(rehome=True, **kw):
    """A NatureConvBody whose parameters one FusedOptimizer owns (conv weights K-major: FlatParams(koc=nature_conv_weights(...)))."""
    from deeprl_amd import nets, optim
    body = nets.NatureConvBody(**kw)
    if rehome:
        body._opt = optim.FusedOptimizer.adopt(torch.optim.RMSprop(body.parameters(), lr=1e-3))
    return body


def test_trunk_check_accepts_a_rehomed_nature_conv_body():
    from deeprl_amd import pixel_rollout as P
    body = _body()
    assert all(P.k_major(c) for c in (body.conv1, body.conv2, body.conv3))
    assert P.walkable_trunk(body)


def _noisy():
    return _body(noisy_linear=True)


def _conv_without_bias():
    body = _body()
    body.conv2.bias = None
    return body


def _fc4_of_another_shape():
    from deeprl_amd import nets
    body = _body()
    body.fc4 = nets.Linear(3136, 256)
    body.fc4.fused_act = "relu"
    return body


def _fc4_without_relu():
    body = _body()
    body.fc4.fused_act = None
    return body


def _not_k_major():
    return _body(rehome=False)      # torch's own [OC, C, KH, KW] storage


@pytest.mark.parametrize("make", [_noisy, _conv_without_bias, _fc4_of_another_shape, _fc4_without_relu, _not_k_major])
def test_trunk_check_rejects(make):
    from deeprl_amd import nets, pixel_rollout as P
    body = make()
    assert type(body) is nets.NatureConvBody
    assert not P.walkable_trunk(body)


def test_head_check():
    from deeprl_amd import nets, pixel_rollout as P
    head = nets.Linear(512, 6)
    assert P.plain_linear(head)
    head.fused_act = "relu"
    assert not P.plain_linear(head)
    head.fused_act = None
    head.bias = None
    assert not P.plain_linear(head)
    assert not P.plain_linear(torch.nn.Linear(512, 6))


@pytest.mark.parametrize("shape,dtype", [((3, 5), torch.uint8), ((7,), torch.int64)])
def test_staged_upload_round_trips_on_the_cpu_device(shape, dtype):
    from deeprl_amd.support import StagedUpload
    up = StagedUpload(shape, dtype, torch.device('cpu'))
    assert len(up.stages) == 1 and up.events == [None] and up.dev.dtype == dtype and tuple(up.dev.shape) == shape
    at = up.dev.data_ptr()
    rs = np.random.RandomState(3)
    for i in range(5):
        want = rs.randint(0, 200, size=shape)
        if i % 2:
            stage = up.stage()
            assert isinstance(stage, torch.Tensor) and stage.dtype == dtype
            stage.numpy()[...] = want
            got = up.send()
        else:
            got = up.put(want)
        assert got is up.dev and up.dev.data_ptr() == at
        assert np.array_equal(up.dev.numpy(), want.astype(up.dev.numpy().dtype))
    assert up.events == [None]


def test_staged_upload_waits_for_a_stage_only_when_it_comes_round_again():
    from deeprl_amd.support import StagedUpload
    log = []

    class Event:
        made = 0

        def __init__(self):
            self.slot = Event.made       # the stages get their events in slot order, one each
            Event.made += 1
            self.recorded = 0

        def record(self):
            self.recorded += 1
            log.append(("record", self.slot))

        def synchronize(self):
            assert self.recorded > 0
            log.append(("wait", self.slot))

    up = StagedUpload((3, 5), torch.int64, torch.device('cpu'), slots=4, event_cls=Event)
    assert len(up.stages) == 4
    waits = []
    for i in range(9):
        before = len(log)
        up.put(np.full((3, 5), i))
        waits.append([slot for what, slot in log[before:] if what == "wait"])
        assert log[-1] == ("record", i % 4) and log[before:].count(log[-1]) == 1      # wait (if any) first, one record last
        assert torch.equal(up.dev, torch.full((3, 5), i, dtype=torch.int64))
    assert waits == [[], [], [], [], [0], [1], [2], [3], [0]]
    assert Event.made == 4


class _Cfg:
    def __init__(self, freq):
        self.target_network_update_freq = freq


def _bare_agent(freq):
    from deeprl_amd.agents import BaseAgent
    agent = BaseAgent.__new__(BaseAgent)
    agent.config, agent.total_steps, agent.logged = _Cfg(freq), 0, []
    agent.log_train_return = lambda ret, at: agent.logged.append((at, ret))
    return agent


def _infos(t_len, n, ended=()):
    return [tuple({'episodic_return': 1.5 if (t, i) in ended else None} for i in range(n)) for t in range(t_len)]


def test_account_rollout_reports_a_target_sync_inside_the_rollout():
    agent = _bare_agent(3)
    assert agent._account_rollout(_infos(5, 4, ended={(2, 3)}), 4) is True
    assert agent.total_steps == 20 and agent.logged == [(2 * 4 + 3, 1.5)]      # record_online_return: total_steps + the env's index
    agent = _bare_agent(7)
    assert agent._account_rollout(_infos(5, 4), 4) is False and agent.total_steps == 20
    agent = _bare_agent(None)           # (A2C / PPO: no target network)
    assert agent._account_rollout(_infos(5, 4), 4) is False and agent.total_steps == 20


@pytest.mark.parametrize("freq", [3, 7, 11])
def test_account_rollout_agrees_with_the_per_step_loop(freq):
    """NStepDQNAgent.step (host path) advances total_steps by num_workers per rollout step and copies the target network wherever
    total_steps // num_workers % target_network_update_freq == 0."""
    stride, t_len = 4, 5
    agent = _bare_agent(freq)
    total, seen = 0, []
    for _ in range(20):
        copies = 0
        for _ in range(t_len):
            total += stride
            if total // stride % freq == 0:
                copies += 1
        assert agent._account_rollout(_infos(t_len, stride), stride) == (copies >= 1)
        assert agent.total_steps == total
        seen.append(copies >= 1)
    assert any(seen) and all(seen) == (freq <= t_len)       # (a multiple of freq falls in every run of t_len steps, or not)
