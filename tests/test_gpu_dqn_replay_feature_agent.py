"""dqn_feature with an n-step window and / or a PrioritizedReplay on the device (deeprl_amd/dqn_replay_mlp.py's Steps under
config.fused_dqn_replay_feature), per kind, against the same agent with the switch off (the parent commit's path) and against the
fp64 restatement: a DQNAgent over VanillaNet with a replay of 32 slots that wraps, n_step 3 and episodes of at most 5 steps.
Everything discrete is equal -- actions, the ring, the drawn leaves and data indices, the pending set, the episode lines, the
generators' next draws, both schedules --; the sum tree and the parameters agree within the family's bars."""
import json
import os
import random

import numpy as np
import pytest
import torch
from feature_kernel_harness import GAME, dra, _Rec, _bits, _fraction, _line_events      # noqa: F401  (dra: the fixture)
from parity_log import record_parity

import dqn_replay_feature_cases as K

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
A = K.AGENT
KINDS = K.KINDS


def _replay_cls(kind):
    from deeprl_amd.replay import PrioritizedReplay, UniformReplay
    return PrioritizedReplay if kind == "per" else UniformReplay


def _config(d, kind, feature, graph=True, **extra):
    from deeprl_amd import zoo
    from deeprl_amd.replay import ReplayWrapper
    kw = dict(fused_dqn_replay_feature=True) if feature else {}
    if feature:
        extra.setdefault("fused_dqn_replay_update", True)      # (the runs name the update's form: the default is the measured one)
    cls = _replay_cls(kind)
    c = zoo.config("dqn_feature", game=GAME, tag="dqn_replay_feat_%s%d%d" % (kind, feature, graph), graph_update=graph,
                   n_step=A["n_step"], replay_cls=cls,
                   overrides=dict(dict(sgd_update_frequency=A["k"], batch_size=A["batch"], target_network_update_freq=A["target_freq"],
                                       exploration_steps=A["exploration_steps"], double_q=A["double_q"]), **extra), **kw)
    c.task_fn = lambda: d.Task(c.game, seed=K.AGENT_SEEDS[kind]["task_seed"], synthetic_done_period=A["horizon"])
    rk = dict(memory_size=A["capacity"], batch_size=A["batch"], n_step=A["n_step"], discount=A["discount"], history_length=1)
    c.replay_fn = lambda: ReplayWrapper(cls, rk, False)
    c.random_action_prob = d.LinearSchedule(*A["eps"])
    c.log_interval = 10 ** 9
    return c


def _make_agent(d, monkeypatch, kind, feature, graph=True, config=None, **kw):
    """-> (agent, its recording logger, the list every minibatch draw is appended to)."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import dqn_replay_mlp
    from deeprl_amd.device_env import DeviceCartPoleVec
    from deeprl_amd.replay import PrioritizedReplay, UniformReplay
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    draws = []
    finish = getattr(PrioritizedReplay._finish_draw, "plain", PrioritizedReplay._finish_draw)

    def recording(self, tree_idx, p, total, batch_size):
        out = finish(self, tree_idx, p, total, batch_size)
        self.recorded.append(dict(drawn=np.asarray(tree_idx).copy(), leaves=np.asarray(out[0]).copy(), prob=np.asarray(out[1]).copy(),
                                  data=np.asarray(out[2]).copy(), total=float(total), pending=sorted(self._pending)))
        return out
    recording.plain = finish
    monkeypatch.setattr(PrioritizedReplay, "_finish_draw", recording)
    plain_draw = getattr(UniformReplay.draw_indices, "plain", UniformReplay.draw_indices)

    def recording_indices(self, batch_size=None):
        idx = plain_draw(self, batch_size)
        self.recorded.append(dict(data=np.asarray(idx).copy()))
        return idx
    recording_indices.plain = plain_draw
    monkeypatch.setattr(UniformReplay, "draw_indices", recording_indices)
    seeds = K.AGENT_SEEDS[kind]
    d.random_seed(9)
    torch.manual_seed(9)
    agent = d.DQNAgent(config or _config(d, kind, feature, graph, **kw))
    agent._inner_replay().recorded = draws
    # the case's parameters (numpy-seeded: the same on every machine), copied into the optimiser's flat buffer through the views;
    # the target starts as their copy (DQN_agent.py:57)
    init = K.restated_agent_run(kind)["init"]
    with torch.no_grad():
        for k, p in agent.network.state_dict().items():
            p.copy_(torch.from_numpy(init[k]))
    agent.sync_target()
    np.random.seed(seeds["np_seed"])        # the exploration, index and leaf streams start here on both paths
    random.seed(seeds["random_seed"])
    want = dqn_replay_mlp.PerStep if kind == "per" else dqn_replay_mlp.Step
    if config is None:
        assert isinstance(agent.actor._task, DeviceCartPoleVec) == bool(feature), rec.warnings
        assert (type(agent._feature) is want) == bool(feature), rec.warnings
    return agent, rec, draws


def _snapshot(agent, rec, draws, kind):
    torch.cuda.synchronize()
    rp = agent._inner_replay()
    frames, acts, rewards, masks = rp._ring.arrays()
    feature = agent._feature is not None
    out = dict(params={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
               target={k: v.detach().cpu().numpy().copy() for k, v in agent.target_network.state_dict().items()},
               ring=dict(frames=frames.view(torch.float64).cpu().numpy().reshape(-1, 4), actions=acts.view(torch.int64).cpu().numpy(),
                         rewards=rewards.cpu().numpy(), masks=masks.cpu().numpy()),
               pos=rp.pos, size=rp.size(), total=agent.total_steps, actor_total=agent.actor._total_steps, draws=draws,
               events=agent.episodes(), lines=[ln for ln in rec.lines if 'episodic_return_train' in ln],
               beta=agent.config.replay_beta.current, epsilon=agent.config.random_action_prob.current,
               graphed={k: r.graph is not None for k, r in agent._feature.regions.items()} if feature else {},
               launches=agent._feature.launches if feature else 0)
    if kind == "per":
        out.update(tree=rp.tree.as_tensor().cpu().numpy().copy(), pending=sorted(rp._pending), write=rp._write,
                   max_priority=float(rp.max_priority))
    out["rng"] = (np.random.randint(0, 1 << 30, size=3), [random.random() for _ in range(3)], torch.rand(3).numpy())
    return out


def _run(d, monkeypatch, kind, feature, graph=True, steps=A["steps"], **kw):
    agent, rec, draws = _make_agent(d, monkeypatch, kind, feature, graph, **kw)
    actions = []
    if not feature:
        raw = agent.actor._task.step

        def step(a):
            actions.append(int(np.asarray(a).reshape(-1)[0]))
            return raw(a)
        agent.actor._task.step = step
    for _ in range(steps):
        agent.step()
        if feature:
            actions += list(agent._feature.out_action.cpu().numpy())
    if feature:
        agent._feature.check()
    out = _snapshot(agent, rec, draws, kind)
    out["actions"] = np.asarray(actions, dtype=np.int64).reshape(steps, A["k"])
    agent.close()
    return out


_RUNS = {}


def _shared(dra, kind):
    """Ten steps of the kind's device path with graph replay and the update kernel: shared by the tests below, left unchanged."""
    if kind not in _RUNS:
        mp = pytest.MonkeyPatch()
        try:
            _RUNS[kind] = _run(dra, mp, kind, True)
        finally:
            mp.undo()
    return _RUNS[kind]


def _same_discrete(a, b, kind, updates=A["steps"] - 1):
    assert a['total'] == b['total'] == a['actor_total'] == b['actor_total'] == A["steps"] * A["k"]
    assert np.array_equal(a['actions'], b['actions'])
    for k in ("frames", "rewards"):
        assert np.array_equal(_bits(a['ring'][k]), _bits(b['ring'][k])), k
    for k in ("actions", "masks"):
        assert np.array_equal(a['ring'][k], b['ring'][k]), k
    assert (a['pos'], a['size']) == (b['pos'], b['size'])
    assert len(a['draws']) == len(b['draws']) == updates
    for x, y in zip(a['draws'], b['draws']):
        assert np.array_equal(x['data'], y['data'])
        if kind == "per":
            assert np.array_equal(x['drawn'], y['drawn']) and np.array_equal(x['leaves'], y['leaves']) and x['pending'] == y['pending']
    if kind == "per":
        assert (a['write'], a['pending']) == (b['write'], b['pending'])
    assert a['lines'] == b['lines'] and a['lines']
    assert a['events'] == _line_events(b['lines']) and b['events'] in ([], a['events'])      # (the host loop keeps no device ring)
    assert a['beta'] == b['beta'] and a['epsilon'] == b['epsilon']
    for x, y in zip(a['rng'], b['rng']):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def _params_fraction(a, b, bar=2e-4):
    worst = 0.0
    for k in b:
        scale = max(np.abs(b[k]).max(), 1e-2)
        worst = max(worst, float(np.max(np.abs(a[k] - b[k])) / (bar * scale)))
    return worst


def _tree_fractions(a, b, what):
    return dict(tree=_fraction(a['tree'], b['tree'], "sum tree " + what),
                prob=max(_fraction(x['prob'], y['prob'], "sampling probabilities " + what) for x, y in zip(a['draws'], b['draws'])),
                total=max(_fraction([x['total']], [y['total']], "tree total " + what) for x, y in zip(a['draws'], b['draws'])),
                max_priority=_fraction([a['max_priority']], [b['max_priority']], "max_priority " + what))


@pytest.mark.parametrize("kind", KINDS)
def test_agent_device_path_equals_host_loop_and_restatement(dra, monkeypatch, kind):
    """Ten agent steps of four transitions with config.fused_dqn_replay_feature -- eager steps, then graph replays -- against the
    same agent with the switch off and against the fp64 restatement: actions, the replay ring's four arrays, its cursors, every
    update's data indices (per: the drawn leaves, the leaves after the validity check and the padding, the pending set after every
    draw and at the end), total_steps, the episodic-return lines, the next draws of np.random, python's random and torch's
    generator and both schedules equal; per: the sum tree, every draw's probabilities and total and max_priority within 1e-5 of
    scale; online and target parameters within 2e-4 of each tensor's largest magnitude (floor 1e-2), the family's bar.  The run
    itself meets what it is there for: a terminal inside a sampled window and, per, an update that pads an invalid draw and one
    that draws a leaf twice."""
    from deeprl_amd.dqn_mlp import Step
    per = kind == "per"
    a, b = _shared(dra, kind), _run(dra, monkeypatch, kind, False)
    assert a['graphed'] == dict(act=False, learn=True) and a['launches'] == 1 + Step.WARMUP + 1      # eager steps and the capture pass
    _same_discrete(a, b, kind)
    cap = A["capacity"]
    assert (b['ring']['masks'][:cap] == 0).any()      # (that a SAMPLED window holds one: the restatement's record, below)
    f = {}
    if per:
        padded = sum(not np.array_equal(x['drawn'], x['leaves']) for x in b['draws'])
        twice = sum(len(set(x['leaves'].tolist())) < A["batch"] for x in b['draws'])
        print("updates that padded an invalid draw: %d, that drew a leaf twice: %d" % (padded, twice))
        assert padded >= 1 and twice >= 1
        f = _tree_fractions(a, b, "vs host loop")
    params = max(_params_fraction(a['params'], b['params']), _params_fraction(a['target'], b['target']))
    record_parity("dqn_replay_feature %s device path vs host loop (fraction of the bars)" % kind, params=params, **f)
    assert all(v <= 1.0 for v in f.values()), f
    assert params <= 1.0, params
    # ... and against the fp64 restatement of the agent step
    r = K.restated_agent_run(kind)
    ups = [u for u in r['updates'] if u is not None]
    assert np.array_equal(a['actions'], r['actions']) and len(ups) == len(a['draws'])
    assert any(u['window_terminal'] for u in ups)
    for x, u in zip(a['draws'], ups):
        assert np.array_equal(x['data'], u['data'])
        if per:
            assert np.array_equal(x['drawn'], u['drawn']) and np.array_equal(x['leaves'], u['leaves'])
    for k in ("frames", "rewards"):
        assert np.array_equal(_bits(a['ring'][k][:cap]), _bits(np.asarray(r['ring'][k], dtype=np.float64))), k
    assert np.array_equal(a['ring']['actions'][:cap], r['ring']['actions']) and np.array_equal(a['ring']['masks'][:cap], r['ring']['masks'])
    assert (a['pos'], a['size'], a['total']) == (r['pos'], r['size'], r['total'])
    assert np.array_equal(a['rng'][0], r['rng_tail']) and a['rng'][1] == r['random_tail'] and a['epsilon'] == r['epsilon']
    assert [(s, v) for s, v in a['events']] == [(s, v) for s, _, v in r['events']]
    g = {}
    if per:
        assert a['pending'] == r['pending'] and a['beta'] == r['beta']
        g = dict(tree=_fraction(a['tree'][:len(r['tree'])], r['tree'], "sum tree vs restatement"),
                 total=max(_fraction([x['total']], [u['total']], "tree total vs restatement") for x, u in zip(a['draws'], ups)),
                 prob=max(_fraction(x['prob'], u['prob'], "probabilities vs restatement") for x, u in zip(a['draws'], ups)),
                 max_priority=_fraction([a['max_priority']], [r['max_priority']], "max_priority vs restatement"))
    params = max(_params_fraction(a['params'], r['params'][-1]), _params_fraction(a['target'], r['target']))
    record_parity("dqn_replay_feature %s device path vs restatement (fraction of the bars)" % kind, params=params, **g)
    assert all(v <= 1.0 for v in g.values()), g
    assert params <= 1.0, params


@pytest.mark.parametrize("kind", KINDS)
def test_module_update_form_matches_the_fused_one(dra, monkeypatch, kind):
    """config.fused_dqn_replay_update False (device acting, ring, draw and commit; ring.gather, the modules and ops.td_loss on the
    same staged indices, probabilities and beta) over the same ten steps: everything discrete equal, the sum tree within 1e-5 of
    scale, parameters within the agent test's bar."""
    a, b = _shared(dra, kind), _run(dra, monkeypatch, kind, True, fused_dqn_replay_update=False)
    assert b['graphed'] == dict(act=False, learn=True)
    _same_discrete(a, b, kind)
    f = _tree_fractions(a, b, "vs module form") if kind == "per" else {}
    params = max(_params_fraction(a['params'], b['params']), _params_fraction(a['target'], b['target']))
    record_parity("dqn_replay_feature %s fused update vs module update on the device (fraction of the bars)" % kind, params=params, **f)
    assert all(v <= 1.0 for v in f.values()) and params <= 1.0, (f, params)


@pytest.mark.parametrize("fused", [True, False], ids=["kernel", "modules"])
@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_equals_eager(dra, monkeypatch, kind, fused):
    """exploration_steps 18: four acting-only steps (two eager, the capture, a replay), then six learning steps (two eager, the
    capture, three replays) with commits and target copies between replays.  config.graph_update False keeps every step eager:
    everything discrete equal and every parameter and the tree equal to the bit -- for both forms of the update."""
    kw = dict(exploration_steps=18, fused_dqn_replay_update=fused)
    a, b = _run(dra, monkeypatch, kind, True, graph=True, **kw), _run(dra, monkeypatch, kind, True, graph=False, **kw)
    assert a['graphed'] == dict(act=True, learn=True) and b['graphed'] == dict(act=False, learn=False)
    assert a['launches'] == 3 + 3 and b['launches'] == A["steps"]
    _same_discrete(a, b, kind, updates=6)
    if kind == "per":
        assert np.array_equal(_bits(a['tree']), _bits(b['tree']))
    for which in ('params', 'target'):
        for k in a[which]:
            assert np.array_equal(_bits(a[which][k]), _bits(b[which][k])), (which, k)


@pytest.mark.parametrize("kind", KINDS)
def test_save_load_continues_the_run(dra, monkeypatch, tmp_path, kind):
    """5 steps, save() + the replay's save_full() (the ring and, per, the sum tree, the pending set, the write cursor, the stat
    pair), a fresh agent, load() + load_full(), 5 more steps == 10 uninterrupted steps, bit for bit.  The optimiser's running
    averages, the target network, the step counters, both schedules and the generators' states are no part of a checkpoint, so the
    test carries them over by hand."""
    whole = _shared(dra, kind)
    first, rec, draws = _make_agent(dra, monkeypatch, kind, True)
    for _ in range(5):
        first.step()
    name = str(tmp_path / "ckpt")
    first.save(name)
    first._inner_replay().save_full(name)
    assert os.path.isfile(name + ".envs") and os.path.isfile(name + ".model") and os.path.isfile(name + ".replay")
    rng = np.random.get_state(), random.getstate(), torch.get_rng_state()
    second, rec2, draws2 = _make_agent(dra, monkeypatch, kind, True)
    assert int(second._feature.step_dev.item()) == 0
    second.load(name)
    second._inner_replay().load_full(name)
    assert int(second._feature.step_dev.item()) == 5 * A["k"] == second._feature.episodes.stamp
    for key in ("env_state", "env_counter", "ep_steps", "ep_return"):
        assert torch.equal(getattr(second.actor._task, key), getattr(first.actor._task, key)), key
    second._fused.state1.copy_(first._fused.state1)
    second._fused.state2.copy_(first._fused.state2)
    second._target_flat.flat.copy_(first._target_flat.flat)
    second._fused.steps, second.total_steps, second.actor._total_steps = first._fused.steps, first.total_steps, first.actor._total_steps
    second.config.replay_beta.current = first.config.replay_beta.current
    second.config.random_action_prob.current = first.config.random_action_prob.current
    np.random.set_state(rng[0])
    random.setstate(rng[1])
    torch.set_rng_state(rng[2])
    for _ in range(5):
        second.step()
    second.drain_episodes()
    got = _snapshot(second, rec2, draws2, kind)
    first.close()
    second.close()
    keys = ("total", "pos", "size", "beta", "epsilon") + (("write", "pending") if kind == "per" else ())
    assert [got[k] for k in keys] == [whole[k] for k in keys]
    assert [ln for ln in rec.lines if 'episodic_return_train' in ln] + got['lines'] == whole['lines']
    for x, y in zip(got['rng'], whole['rng']):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert len(draws) == 4 and len(draws2) == 5
    for x, y in zip(draws + draws2, whole['draws']):
        assert np.array_equal(x['data'], y['data'])
        if kind == "per":
            assert np.array_equal(x['leaves'], y['leaves']) and np.array_equal(_bits(x['prob']), _bits(y['prob']))
    for k in got['ring']:
        assert np.array_equal(_bits(got['ring'][k]), _bits(whole['ring'][k])), k
    if kind == "per":
        assert np.array_equal(_bits(got['tree']), _bits(whole['tree']))
    for k in got['params']:
        assert np.array_equal(_bits(got['params'][k]), _bits(whole['params'][k])), k


@pytest.mark.parametrize("kind", KINDS)
def test_switches(dra, monkeypatch, kind):
    """With the default configuration and with config.fused_dqn_feature alone the agent stays on the host -- silently without a
    switch, with the old path's reason under the old switch; with the new switch on and a setup the path does not take (a
    DuelingNet) it is told why, once, and runs on the host."""
    import deeprl_amd.agents as agents_mod
    d = dra
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    agent = d.DQNAgent(_config(d, kind, False))
    assert agent._feature is None and type(agent.actor._task) is d.Task and rec.warnings == []
    agent.step()
    assert agent.total_steps == A["k"]
    agent.close()
    c = _config(d, kind, False)
    c.fused_dqn_feature = True
    agent = d.DQNAgent(c)
    assert agent._feature is None and type(agent.actor._task) is d.Task and len(rec.warnings) == 1
    assert ("the replay is a PrioritizedReplay" if kind == "per" else "n_step is not 1") in rec.warnings[0]
    agent.close()
    del rec.warnings[:]
    c = _config(d, kind, True)
    c.network_fn = lambda: d.DuelingNet(c.action_dim, d.FCBody(c.state_dim))
    agent = d.DQNAgent(c)
    assert agent._feature is None and type(agent.actor._task) is d.Task
    assert len(rec.warnings) == 1 and "the network is not VanillaNet" in rec.warnings[0]
    agent.step()
    assert agent.total_steps == A["k"]
    agent.close()
    del rec.warnings[:]
    c = _config(d, kind, True)      # both switches: the old one refuses and says so, the new one takes the agent
    c.fused_dqn_feature = True
    agent = d.DQNAgent(c)
    assert agent._feature is not None and agent._feature.KIND.PRIORITIZED == (kind == "per") and len(rec.warnings) == 1
    agent.close()


def test_fused_eval_on_a_prioritized_agent(dra, monkeypatch):
    """config.fused_eval on a PerKind agent (tests/eval_cases.py's dqn_feature weights and evaluation environment, 24 acting steps
    below exploration_steps): eval_episodes() is ONE launch of dra_dqn_mlp_eval and ONE copy back and returns what the host
    evaluation of the same agent with fused_eval off returns -- the restatement's first three episodes."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import dqn_replay_mlp, zoo
    from deeprl_amd.replay import PrioritizedReplay
    import eval_cases as C
    d = dra
    got = C.restated(C.AGENT_CASES["dqn_feature"])
    out = {}
    for fused_eval in (True, False):
        rec = _Rec()
        monkeypatch.setattr(agents_mod, "get_logger", lambda *a, rec=rec, **k: rec)
        d.random_seed(21)
        torch.manual_seed(21)
        random.seed(21)
        c = zoo.config("dqn_feature", game=GAME, tag="dqn_replay_eval_%d" % fused_eval, n_step=3, replay_cls=PrioritizedReplay,
                       overrides=dict(eval_episodes=3, exploration_steps=100, fused_eval=fused_eval, fused_dqn_replay_feature=True))
        c.task_fn = lambda: d.Task(GAME, seed=3, synthetic_done_period=C.HORIZON)
        c.eval_env = d.Task(GAME, seed=C.ENV_SEED, synthetic_done_period=C.HORIZON)
        c.log_interval = 10 ** 9
        agent = d.DQNAgent(c)
        assert type(agent._feature) is dqn_replay_mlp.PerStep, rec.warnings
        with torch.no_grad():
            state = agent.network.state_dict()
            for k, v in got["params"].items():
                state[k].copy_(torch.from_numpy(v))
        agent.sync_target()
        np.random.seed(21)
        for _ in range(24):
            agent.step()
        step = agent._feature
        first = agent.eval_episodes()
        out[fused_eval] = (first, (step.eval_launches, step.eval_copies), [ln for ln in rec.lines if 'episodic_return_test' in ln],
                           None if step.eval_lengths is None else list(step.eval_lengths), list(rec.warnings))
        agent.close()
    want = got["runs"]["five"]
    assert out[True][1] == (1, 1) and out[False][1] == (0, 0) and out[True][4] == out[False][4] == []
    assert out[True][0] == out[False][0] == {'episodic_return_test': want["returns"][:3].mean()}
    assert out[True][2] == out[False][2] and len(out[True][2]) == 1 and out[True][3] == list(want["lengths"][:3])


@pytest.mark.parametrize("kind", KINDS)
def test_closed_loop_learns(dra, monkeypatch, kind):
    """The dqn_feature entry itself (zoo: hidden 64, a replay of 10^4, minibatches of 10, exploration_steps 1000, epsilon 1.0 -> 0.1
    over 10^4, a target copy every 200 updates) with n_step 3, the kind's replay and config.fused_dqn_replay_feature for the number
    of environment steps at which the REFERENCE's own median over five seeds reaches 2 x the bar
    (tests/golden/dqn_replay_feature/learning_reference.json: n_learn = 15 000 for both kinds, where its medians are 106.4 for the
    uniform and 110.3 for the prioritized replay): the median over three seeds of the mean return of the last 100 training
    episodes reaches the bar, 2 x the random policy's mean (44.157)."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    from deeprl_amd.device_env import DeviceCartPoleVec
    d = dra
    ref = json.load(open(os.path.join(GOLDEN, "dqn_replay_feature", "learning_reference.json")))
    bar, n_learn = ref["bar"], ref["n_learn"][kind]
    assert bar == 2.0 * json.load(open(os.path.join(GOLDEN, "dqn_feature", "random_policy.json")))["mean"] and abs(bar - 44.157) < 1e-3
    assert n_learn == 15000
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    means = []
    for seed in K.LEARN_SEEDS:
        d.random_seed(seed)
        torch.manual_seed(seed)
        random.seed(seed)
        c = zoo.config("dqn_feature", game=GAME, tag="dqn_replay_feat_learn_%s%d" % (kind, seed), n_step=3, replay_cls=_replay_cls(kind),
                       fused_dqn_replay_feature=True)
        c.task_fn = lambda seed=seed, c=c: d.Task(c.game, seed=seed)
        c.log_interval = 10 ** 9
        agent = d.DQNAgent(c)
        assert isinstance(agent.actor._task, DeviceCartPoleVec) and agent._feature.KIND.PRIORITIZED == (kind == "per")
        returns = []
        while agent.total_steps < n_learn:
            agent.step()
            if agent.total_steps % 4096 == 0:
                returns += [r for _, r in agent.episodes()]
        returns += [r for _, r in agent.episodes()]
        agent._feature.check()
        agent.close()
        means.append(float(np.mean(returns[-K.LAST_EPISODES:])))
        print("seed %d: %d episodes, last-%d mean %.2f" % (seed, len(returns), K.LAST_EPISODES, means[-1]))
    median = float(np.median(means))
    record_parity("dqn_replay_feature %s closed loop: last-100 mean returns per seed, median, bar" % kind, median=median, bar=bar,
                  **{"seed%d" % s: m for s, m in zip(K.LEARN_SEEDS, means)})
    assert median >= bar, (means, bar)
