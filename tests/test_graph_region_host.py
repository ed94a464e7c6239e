"""The capture protocol of deeprl_amd.graphs.Region on the host (no GPU): stand-ins replace torch.cuda.CUDAGraph, torch.cuda.graph
and torch.cuda.synchronize, stub optimizers record what the region asks of them.  This is where a FAILED capture is covered: no
GPU test may make one fail."""
import gc
import warnings
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch.distributions import Distribution

from deeprl_amd import graphs
from deeprl_amd.graphs import Region

PHRASE = "the region under test"


class _Opt:
    """What a region asks of a FusedOptimizer, recorded in the shared log."""

    def __init__(self, log, name):
        self.log, self.name, self.graph_mode, self.prepared = log, name, False, 0

    def enable_graph_mode(self):
        self.graph_mode = True
        self.log.append(('graph_mode', self.name))

    def prepare_step(self):
        self.prepared += 1
        self.log.append(('prepare', self.name))

    def hyper_signature(self):
        return ('stub', self.name)


@pytest.fixture
def fake(monkeypatch):
    """-> the log and the recording flag of stand-ins for the three torch.cuda names the protocol uses.  As in a real capture
    the body's Python runs while it is being recorded."""
    state = SimpleNamespace(log=[], recording=False)

    class Graph:
        def replay(self):
            state.log.append(('replay', id(self)))

    class Recording:
        def __init__(self, graph):
            self.graph = graph

        def __enter__(self):
            state.log.append(('enter', id(self.graph)))
            state.recording = True

        def __exit__(self, *exc):
            state.recording = False
            state.log.append(('exit', id(self.graph)))
            return False

    monkeypatch.setattr(torch.cuda, 'CUDAGraph', Graph)
    monkeypatch.setattr(torch.cuda, 'graph', Recording)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: state.log.append(('synchronize',)))
    return state


def _config(**switches):
    return SimpleNamespace(**switches)


def _body(fake, fail=False, seen=None):
    """A body that logs whether it ran eagerly or was being recorded, notes what it saw while recorded, and may fail there."""
    def body():
        fake.log.append(('body', 'recorded' if fake.recording else 'eager'))
        if fake.recording:
            if seen is not None:
                seen.update(validate=Distribution._validate_args, gc=gc.isenabled())
            if fail:
                raise ValueError("host-side control flow")
        return 'out'
    return body


def _call(region, body, key=None):
    """One call of a site, as Region's docstring writes it."""
    if region.due(key) and (region.graph is not None or region.capture(body, key)):
        return region.replay()
    return body()


def _count(log, *entry):
    return sum(1 for e in log if e[:len(entry)] == entry)


@pytest.mark.parametrize("warmup", [0, 2, 4])
def test_warmup_then_one_recording_then_replays(fake, warmup):
    region = Region(PHRASE, _config(), warmup)
    body = _body(fake)
    for _ in range(warmup):
        assert _call(region, body) == 'out'
    assert fake.log == [('body', 'eager')] * warmup and region.graph is None and region.calls == warmup
    assert _call(region, body) == 'out'           # call W + 1 records once, and replays what it recorded
    g = id(region.graph)
    assert fake.log[warmup:] == [('synchronize',), ('enter', g), ('body', 'recorded'), ('exit', g), ('replay', g)]
    for _ in range(5):
        assert _call(region, body) == 'out'
    assert fake.log[warmup + 5:] == [('replay', g)] * 5 and region.calls == warmup + 6 and not region.failed


def test_changed_key_records_again_exactly_once(fake):
    region = Region(PHRASE, _config(), 1)
    body = _body(fake)
    for key in ['a', 'a', 'a', 'b', 'b', 'a']:     # (warm-up, record, replay, re-record, replay, re-record)
        _call(region, body, key)
    assert _count(fake.log, 'body', 'recorded') == 3 and _count(fake.log, 'replay') == 5 and region.key == 'a'
    first = region.graph
    _call(region, body, 'a')
    assert region.graph is first and _count(fake.log, 'enter') == 3


def test_graph_mode_and_synchronize_come_before_the_capture(fake):
    inside, outside = _Opt(fake.log, 'inside'), _Opt(fake.log, 'outside')
    region = Region(PHRASE, _config(), 0, opts=(inside,))
    _call(region, _body(fake))
    names = [e[0] for e in fake.log]
    assert names.index('graph_mode') < names.index('synchronize') < names.index('enter')
    assert names[names.index('enter') - 1] == 'synchronize', "nothing may come between the synchronisation and the capture"
    assert inside.graph_mode and not outside.graph_mode


def test_prepare_step_once_per_replay_on_the_inside_optimizers_only(fake):
    a, b, other = _Opt(fake.log, 'a'), _Opt(fake.log, 'b'), _Opt(fake.log, 'other')
    region = Region(PHRASE, _config(), 2)
    for _ in range(6):
        _call(region, _body(fake))
    assert _count(fake.log, 'prepare') == 0, "a region without optimizers prepares none"
    region = Region(PHRASE, _config(), 2, opts=(a,))
    for i in range(6):          # optimizers named at the capture take the constructor's place
        if region.due() and (region.graph is not None or region.capture(_body(fake), opts=(a, b))):
            region.replay()
            tail = fake.log[-3:]
            assert tail == [('prepare', 'a'), ('prepare', 'b'), ('replay', id(region.graph))]
    assert (a.prepared, b.prepared, other.prepared) == (4, 4, 0)


@pytest.mark.parametrize("fail", [False, True])
@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("validate_off", [False, True])
def test_validation_flag_during_and_after(fake, validate_off, prior, fail):
    before = Distribution._validate_args
    try:
        Distribution.set_default_validate_args(prior)
        seen = {}
        region = Region(PHRASE, _config(allow_eager_fallback=True), 0, validate_off=validate_off)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            _call(region, _body(fake, fail=fail, seen=seen))
        assert seen['validate'] == (False if validate_off else prior)
        assert Distribution._validate_args == prior
        assert region.failed == fail
    finally:
        Distribution.set_default_validate_args(before)


@pytest.mark.parametrize("fail", [False, True])
@pytest.mark.parametrize("prior", [False, True])
def test_collector_is_off_while_recording_and_as_before_afterwards(fake, prior, fail):
    was = gc.isenabled()
    try:
        gc.enable() if prior else gc.disable()
        seen = {}
        region = Region(PHRASE, _config(allow_eager_fallback=True), 0)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            _call(region, _body(fake, fail=fail, seen=seen))
        assert seen['gc'] is False
        assert gc.isenabled() == prior
    finally:
        gc.enable() if was else gc.disable()


def test_failure_without_the_switch_raises_chained(fake):
    opt = _Opt(fake.log, 'a')
    region = Region(PHRASE, _config(), 0, opts=(opt,), validate_off=True)
    prior = Distribution._validate_args
    with pytest.raises(RuntimeError, match=PHRASE) as err:
        _call(region, _body(fake, fail=True))
    assert isinstance(err.value.__cause__, ValueError) and "host-side control flow" in str(err.value.__cause__)
    assert "config.allow_eager_fallback = True" in str(err.value) and "config.graph_update = False" in str(err.value)
    assert Distribution._validate_args == prior and region.graph is None


def test_failure_with_the_switch_stays_eager(fake):
    opts = (_Opt(fake.log, 'a'), _Opt(fake.log, 'b'))
    region = Region(PHRASE, _config(allow_eager_fallback=True), 1, opts=opts)
    body = _body(fake, fail=True)
    _call(region, body)
    with pytest.warns(UserWarning, match=PHRASE + " could not be captured as a graph"):
        assert _call(region, body) == 'out'       # the failed recording, then the same call's eager run
    assert region.failed and region.graph is None and [o.graph_mode for o in opts] == [False, False]
    assert fake.log[-2:] == [('exit', fake.log[-2][1]), ('body', 'eager')]
    entered = _count(fake.log, 'enter')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for _ in range(10):
            assert _call(region, body) == 'out'
    assert fake.log[-10:] == [('body', 'eager')] * 10 and _count(fake.log, 'enter') == entered == 1
    assert _count(fake.log, 'replay') == 0 and _count(fake.log, 'prepare') == 0


def test_named_bodies_give_named_graphs(fake):
    region = Region(PHRASE, _config(), 0)
    assert region.due() and region.capture(dict(first=lambda: 1, second=lambda: 2))
    assert list(region.graph) == ['first', 'second'] and region.out == dict(first=1, second=2)
    assert [e[0] for e in fake.log] == ['synchronize', 'enter', 'exit', 'enter', 'exit']


# ---------------------------------------------------------------------------------------------------- the wrappers
Plan = namedtuple('Plan', ['counters', 't_len'])


class _RolloutAgent:
    """What _OnPolicyGraph reads of an on-policy agent; compute() advances _rollout_step as the agents' rollouts do."""

    def __init__(self, fake, config, fail):
        self.config, self.grad_hook, self._rollout_step = config, None, 0
        self._fused = _Opt(fake.log, 'fused')
        self.fake, self.fail = fake, fail

    def compute(self, plan):
        self._rollout_step += plan.t_len
        if self.fake.recording and self.fail:
            raise ValueError("host-side control flow")
        return self._rollout_step


def test_on_policy_graph_counts_rollout_steps_like_an_uncaptured_run(fake):
    plan = Plan(torch.zeros(4, dtype=torch.int64), 5)
    calls = graphs._OnPolicyGraph.WARMUP + 4
    steps = {}
    for name, cfg, fail in [('captured', _config(), False), ('failed', _config(allow_eager_fallback=True), True),
                            ('off', _config(graph_update=False), False)]:
        agent = _RolloutAgent(fake, cfg, fail)
        g = graphs._OnPolicyGraph(agent)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for _ in range(calls):
                g.run(plan, agent.compute)
        steps[name] = agent._rollout_step
        assert g.calls == calls and (g.graph is not None) == (name == 'captured') and g.failed == (name == 'failed')
        assert agent._fused.graph_mode == (name == 'captured')
    assert steps['off'] == calls * plan.t_len
    assert steps['failed'] == steps['off'], "the aborted recording's advance must not reach the eager fallback"
    assert steps['captured'] == steps['off']
    assert _count(fake.log, 'enter') == 2, "one recording each for 'captured' and 'failed', none with the switch off"


def test_graph_update_off_never_records(fake, monkeypatch):
    from deeprl_amd.normalizers import ImageNormalizer
    from deeprl_amd.support import Config
    monkeypatch.setattr(Config, 'DEVICE', torch.device('cuda'))     # (nothing below reaches the device)
    cfg = _config(graph_update=False, noisy_linear=False, state_normalizer=ImageNormalizer(), shared_repr=True)
    frame = np.zeros((1, 4, 84, 84), dtype=np.uint8)
    adam = SimpleNamespace(kind='adam')
    agent = SimpleNamespace(config=cfg, _network=None, network=None, target_network=None, _fused=adam, grad_hook=None,
                            dp=SimpleNamespace(active=False))
    uniform_replay = SimpleNamespace()
    assert not graphs._GraphedQ(agent).usable(frame)
    assert not graphs._GraphedUpdate(agent).usable(uniform_replay)
    assert not graphs._GraphedPPO(agent).usable()
    assert graphs._GraphedAct(agent)(np.zeros((2, 3))) is None
    region = Region(PHRASE, cfg, 0)         # as noisy_actor.NoisyActor holds it
    assert not any(region.due() for _ in range(5))
    cfg.graph_update = True                 # the same stubs with the switch on: it was the switch that said no
    assert graphs._GraphedQ(agent).usable(frame) and graphs._GraphedUpdate(agent).usable(uniform_replay)
    assert graphs._GraphedPPO(agent).usable() and region.due()
    cfg.graph_rollout = False               # _GraphedAct's own switch, which defaults to graph_update
    act = graphs._GraphedAct(agent)
    assert all(act(np.zeros((2, 3))) is None for _ in range(5)) and act.calls == 0
    assert fake.log == []
