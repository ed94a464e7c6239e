"""rainbow_feature's agent step on the device (deeprl_amd/rainbow_mlp.py's Step under config.fused_rainbow_feature) against the same
agent with the switch off (the parent commit's path): a CategoricalDQNAgent over RainbowNet(noisy FCBody) with an n-step
PrioritizedReplay small enough to wrap, episodes of at most 5 steps, double_q.  Everything discrete is equal -- actions, the ring,
the drawn leaves and data indices, the pending set, the episode lines, the four generators' next draws, the schedules -- and so are
the noise vectors both networks are left with; the sum tree and the parameters agree within the family's bars."""
import json
import os
import random

import numpy as np
import pytest
import torch
from feature_kernel_harness import GAME, dra, _Rec, _bits, _fraction, _line_events      # noqa: F401  (dra: the fixture)
from parity_log import record_parity

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEARN_SEEDS, LAST_EPISODES = (1, 2, 3), 100
NOISE = ("noise_in", "noise_out_weight", "noise_out_bias")

# 10 agent steps of 4 transitions; exploration_steps 6 (crossed inside the second step); minibatches of 8 from a replay of 32
# slots (it wraps in the ninth step) with n_step 3; a target copy every 3 steps; the entry's own network (hidden 64, 50 atoms)
A = dict(k=4, batch=8, capacity=32, exploration_steps=6, target_freq=3, horizon=5, steps=10, task_seed=3, seed=11, n_step=3)


def _config(d, feature, graph=True, **extra):
    from deeprl_amd import zoo
    from deeprl_amd.replay import PrioritizedReplay, ReplayWrapper
    kw = dict(fused_rainbow_feature=True) if feature else {}
    if feature:
        extra.setdefault("fused_rainbow_update", True)      # (the runs name the update's form: the default is the measured one)
    c = zoo.config("rainbow_feature", game=GAME, tag="rainbow_feat_%d%d" % (feature, graph), graph_update=graph, n_step=A["n_step"],
                   overrides=dict(dict(sgd_update_frequency=A["k"], batch_size=A["batch"], target_network_update_freq=A["target_freq"],
                                       exploration_steps=A["exploration_steps"]), **extra), **kw)
    c.task_fn = lambda: d.Task(c.game, seed=A["task_seed"], synthetic_done_period=A["horizon"])
    rk = dict(memory_size=A["capacity"], batch_size=A["batch"], n_step=A["n_step"], discount=c.discount, history_length=1)
    c.replay_fn = lambda: ReplayWrapper(PrioritizedReplay, rk, False)
    c.log_interval = 10 ** 9
    return c


def _make_agent(d, monkeypatch, feature, graph=True, **kw):
    """-> (agent, its recording logger, the list every prioritised draw is appended to)."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd.device_env import DeviceCartPoleVec
    from deeprl_amd.rainbow_mlp import Step
    from deeprl_amd.replay import PrioritizedReplay
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
    d.random_seed(A["seed"])
    torch.manual_seed(A["seed"])
    random.seed(A["seed"])
    agent = d.CategoricalDQNAgent(_config(d, feature, graph, **kw))
    agent._inner_replay().recorded = draws
    np.random.seed(A["seed"])
    assert isinstance(agent.actor._task, DeviceCartPoleVec) == bool(feature), rec.warnings
    assert (type(agent._feature) is Step) == bool(feature), rec.warnings
    return agent, rec, draws


def _snapshot(agent, rec, draws):
    torch.cuda.synchronize()
    rp = agent._inner_replay()
    frames, acts, rewards, masks = rp._ring.arrays()
    feature = agent._feature is not None
    return dict(state={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
                target={k: v.detach().cpu().numpy().copy() for k, v in agent.target_network.state_dict().items()},
                ring=dict(frames=frames.view(torch.float64).cpu().numpy().reshape(-1, 4), actions=acts.view(torch.int64).cpu().numpy(),
                          rewards=rewards.cpu().numpy(), masks=masks.cpu().numpy()),
                tree=rp.tree.as_tensor().cpu().numpy().copy(), pending=sorted(rp._pending), write=rp._write, pos=rp.pos, size=rp.size(),
                max_priority=float(rp.max_priority), total=agent.total_steps, actor_total=agent.actor._total_steps, draws=draws,
                events=agent.episodes(), lines=[ln for ln in rec.lines if 'episodic_return_train' in ln],
                beta=agent.config.replay_beta.current,
                rng=(np.random.randint(0, 1 << 30, size=3), [random.random() for _ in range(3)], torch.rand(3).numpy()),
                graphed={k: r.graph is not None for k, r in agent._feature.regions.items()} if feature else {},
                launches=agent._feature.launches if feature else 0)


def _run(d, monkeypatch, feature, graph=True, steps=A["steps"], **kw):
    agent, rec, draws = _make_agent(d, monkeypatch, feature, graph, **kw)
    actions, noise_log = [], dict(online=[], target=[])
    start = dict(init={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
                 random=random.getstate(), noise=noise_log)
    if not feature:
        from deeprl_amd.nets import _NoiseBlock
        blocks = {id(agent.network.noise_block()): "online", id(agent.target_network.noise_block()): "target"}
        draw_into = _NoiseBlock._draw_into

        def recording_draw(self, host):      # every draw of the host loop's two networks, per network in its order
            draw_into(self, host)
            if id(self) in blocks:
                row = host.numpy().copy()
                noise_log[blocks[id(self)]].append({"%s.%s" % ln_b: row[o:o + n] for ln_b, (o, n) in self.slices.items()})
        monkeypatch.setattr(_NoiseBlock, "_draw_into", recording_draw)
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
    out = _snapshot(agent, rec, draws)
    out["actions"] = np.asarray(actions, dtype=np.int64).reshape(steps, A["k"])
    out["start"] = start
    agent.close()
    return out


_RUNS = {}


def _shared(dra, key, feature, graph=True):
    if key not in _RUNS:
        mp = pytest.MonkeyPatch()
        try:
            _RUNS[key] = _run(dra, mp, feature, graph)
        finally:
            mp.undo()
    return _RUNS[key]


def _restated(b):
    """rainbow_feature_restatement.agent_run from the host loop's initial parameters, under the noise its reset_noise() calls
    drew (in their order) and its generators' states, over the same environment."""
    import rainbow_feature_cases as K
    import rainbow_feature_restatement as R
    from deeprl_amd import zoo
    c = zoo.config("rainbow_feature", game=GAME, tag="rainbow_feat_restated")
    log = {which: iter(rows) for which, rows in b['start']['noise'].items()}
    noise_fn = lambda which: next(log[which])
    cfg = dict(k=A["k"], batch=A["batch"], capacity=A["capacity"], exploration_steps=A["exploration_steps"],
               target_freq=A["target_freq"], discount=c.discount, n_step=A["n_step"], gradient_clip=c.gradient_clip, lr=0.001,
               double_q=True, gate="relu", spec=dict(n=50, v_min=-100.0, v_max=100.0), hidden=64, std=None, beta=(0.4, 1.0, c.max_steps),
               replay_eps=c.replay_eps, replay_alpha=c.replay_alpha)
    env, _ = K.make_env(A["task_seed"], A["horizon"])
    rnd = random.Random()
    rnd.setstate(b['start']['random'])
    state = np.random.get_state()
    np.random.seed(A["seed"])
    try:
        out = R.agent_run({k: b['start']['init'][k] for k in R.KEYS}, env, cfg, rnd, A["steps"], noise_fn=noise_fn)
        out["np_tail"] = np.random.randint(0, 1 << 30, size=3)
    finally:
        np.random.set_state(state)
    assert all(next(it, None) is None for it in log.values())
    return out


def _same_discrete(a, b, updates=A["steps"] - 1):
    assert a['total'] == b['total'] == a['actor_total'] == b['actor_total'] == A["steps"] * A["k"]
    assert np.array_equal(a['actions'], b['actions'])
    for k in ("frames", "rewards"):
        assert np.array_equal(_bits(a['ring'][k]), _bits(b['ring'][k])), k
    for k in ("actions", "masks"):
        assert np.array_equal(a['ring'][k], b['ring'][k]), k
    assert (a['pos'], a['size'], a['write'], a['pending']) == (b['pos'], b['size'], b['write'], b['pending'])
    assert len(a['draws']) == len(b['draws']) == updates
    for x, y in zip(a['draws'], b['draws']):
        for k in ("drawn", "leaves", "data"):
            assert np.array_equal(x[k], y[k]), k
        assert x['pending'] == y['pending']
    assert a['lines'] == b['lines'] and a['lines']
    assert a['events'] == _line_events(b['lines']) and b['events'] in ([], a['events'])      # (the host loop keeps no device ring)
    assert a['beta'] == b['beta']
    for x, y in zip(a['rng'], b['rng']):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    # the noise both networks are left with: the update's draws (the online network's last one after the last acting row)
    for which in ('state', 'target'):
        for k in a[which]:
            if k.endswith(NOISE):
                assert np.array_equal(_bits(a[which][k]), _bits(b[which][k])), (which, k)


def _params_fraction(a, b, bar=2e-4):
    worst = 0.0
    for k in a:
        if k.endswith(("_mu", "_sigma")):
            scale = max(np.abs(b[k]).max(), 1e-2)
            worst = max(worst, float(np.max(np.abs(a[k] - b[k])) / (bar * scale)))
    return worst


def test_agent_device_path_equals_host_loop(dra, monkeypatch):
    """Ten agent steps with config.fused_rainbow_feature -- eager steps, then graph replays -- against the same agent with the
    switch off: actions, the replay ring's four arrays, its cursors, every update's drawn leaves, the leaves and data indices
    after the validity check and the padding, the pending set after every draw and at the end, total_steps, the episodic-return
    lines, the next draws of np.random, python's random and torch's generator, beta's schedule and both networks' noise vectors
    equal; the sum tree (leaves and totals) and every draw's probabilities and total within 1e-5 of scale; online and target
    parameters within 2e-4 of each tensor's largest magnitude (floor 1e-2), the family's bar.  The run itself meets what it is
    there for: an update that pads an invalid draw, one that draws a leaf twice, and a terminal inside a sampled window."""
    from deeprl_amd.rainbow_mlp import Step
    a, b = _shared(dra, "device", True), _run(dra, monkeypatch, False)
    assert a['graphed'] == dict(act=False, learn=True) and a['launches'] == 1 + Step.WARMUP + 1      # eager steps and the capture pass
    _same_discrete(a, b)
    cap, n = A["capacity"], A["n_step"]
    padded = sum(not np.array_equal(x['drawn'], x['leaves']) for x in b['draws'])
    twice = sum(len(set(x['leaves'].tolist())) < A["batch"] for x in b['draws'])
    print("updates that padded an invalid draw: %d, that drew a leaf twice: %d" % (padded, twice))
    assert padded >= 1 and twice >= 1
    assert (b['ring']['masks'][:cap] == 0).any()
    f = dict(tree=_fraction(a['tree'], b['tree'], "sum tree"),
             prob=max(_fraction(x['prob'], y['prob'], "sampling probabilities") for x, y in zip(a['draws'], b['draws'])),
             total=max(_fraction([x['total']], [y['total']], "tree total") for x, y in zip(a['draws'], b['draws'])),
             max_priority=_fraction([a['max_priority']], [b['max_priority']], "max_priority"))
    params = max(_params_fraction(a['state'], b['state']), _params_fraction(a['target'], b['target']))
    record_parity("rainbow_feature device path vs host loop (fraction of the bars)", params=params, **f)
    assert all(v <= 1.0 for v in f.values()), f
    assert params <= 1.0, params
    # ... and against the fp64 restatement of the agent step under the host loop's noise draws
    r = _restated(b)
    ups = [u for u in r['updates'] if u is not None]
    assert np.array_equal(a['actions'], r['actions']) and min(r['margin'], r['argmax_margin']) >= 1e-4
    assert len(ups) == len(a['draws'])
    for x, u in zip(a['draws'], ups):
        assert np.array_equal(x['drawn'], u['drawn']) and np.array_equal(x['leaves'], u['leaves']) and np.array_equal(x['data'], u['data'])
    assert a['pending'] == r['pending']
    for k in ("frames", "rewards"):
        assert np.array_equal(_bits(a['ring'][k][:cap]), _bits(np.asarray(r['ring'][k], dtype=np.float64))), k
    assert np.array_equal(a['ring']['actions'][:cap], r['ring']['actions']) and np.array_equal(a['ring']['masks'][:cap], r['ring']['masks'])
    assert (a['pos'], a['size'], a['total']) == (r['pos'], r['size'], r['total']) and np.array_equal(a['rng'][0], r['np_tail'])
    g = dict(tree=_fraction(a['tree'][:len(r['tree'])], r['tree'], "sum tree vs restatement"),
             total=max(_fraction([x['total']], [u['total']], "tree total vs restatement") for x, u in zip(a['draws'], ups)),
             prob=max(_fraction(x['prob'], u['prob'], "probabilities vs restatement") for x, u in zip(a['draws'], ups)),
             max_priority=_fraction([a['max_priority']], [r['max_priority']], "max_priority vs restatement"))
    want = dict(state=r['params'][-1], target=r['target'])
    params = max(_params_fraction({k: a[w][k] for k in want[w]}, want[w]) for w in want)
    record_parity("rainbow_feature device path vs restatement (fraction of the bars)", params=params, **g)
    assert all(v <= 1.0 for v in g.values()), g
    assert params <= 1.0, params


def test_module_update_form_matches_the_fused_one(dra, monkeypatch):
    """config.fused_rainbow_update False (device acting, ring, draw and commit; ring.gather and the modules, ops.per_weights_dev and
    ops.c51_loss on the same staged indices, probabilities and beta) over the same ten steps: everything discrete equal, the sum
    tree within 1e-5 of scale, parameters within the agent test's bar."""
    a, b = _shared(dra, "device", True), _run(dra, monkeypatch, True, fused_rainbow_update=False)
    assert b['graphed'] == dict(act=False, learn=True)
    _same_discrete(a, b)
    tree = _fraction(a['tree'], b['tree'], "sum tree")
    prob = max(_fraction(x['prob'], y['prob'], "sampling probabilities") for x, y in zip(a['draws'], b['draws']))
    params = max(_params_fraction(a['state'], b['state']), _params_fraction(a['target'], b['target']))
    record_parity("rainbow_feature fused update vs module update on the device (fraction of the bars)", params=params, tree=tree, prob=prob)
    assert tree <= 1.0 and prob <= 1.0 and params <= 1.0, (tree, prob, params)


@pytest.mark.parametrize("fused", [True, False], ids=["kernel", "modules"])
def test_graph_replay_equals_eager(dra, monkeypatch, fused):
    """exploration_steps 18: four acting-only steps (two eager, the capture, a replay whose noise rows come from the static rows
    block), then six learning steps (two eager, the capture, three replays) with commits and target copies between replays.
    config.graph_update False keeps every step eager: everything discrete equal and every parameter, the tree and the noise
    equal to the bit -- for both forms of the update."""
    kw = dict(exploration_steps=18, fused_rainbow_update=fused)
    a, b = _run(dra, monkeypatch, True, graph=True, **kw), _run(dra, monkeypatch, True, graph=False, **kw)
    assert a['graphed'] == dict(act=True, learn=True) and b['graphed'] == dict(act=False, learn=False)
    assert a['launches'] == 3 + 3 and b['launches'] == A["steps"]
    _same_discrete(a, b, updates=6)
    assert np.array_equal(_bits(a['tree']), _bits(b['tree']))
    for which in ('state', 'target'):
        for k in a[which]:
            assert np.array_equal(_bits(a[which][k]), _bits(b[which][k])), (which, k)


def test_save_load_continues_the_run(dra, monkeypatch, tmp_path):
    """5 steps, save() + the replay's save_full() (the ring, the sum tree, the pending set, the write cursor, the stat pair), a
    fresh agent, load() + load_full(), 5 more steps == 10 uninterrupted steps, bit for bit.  The optimiser's running averages, the
    target network, the step counters, beta's schedule and the three generators' states are no part of a checkpoint, so the test
    carries them over by hand."""
    import os
    whole = _shared(dra, "device", True)
    first, rec, draws = _make_agent(dra, monkeypatch, True)
    for _ in range(5):
        first.step()
    name = str(tmp_path / "ckpt")
    first.save(name)
    first._inner_replay().save_full(name)
    assert os.path.isfile(name + ".envs") and os.path.isfile(name + ".model") and os.path.isfile(name + ".replay")
    rng = np.random.get_state(), random.getstate(), torch.get_rng_state()
    second, rec2, draws2 = _make_agent(dra, monkeypatch, True)
    assert int(second._feature.step_dev.item()) == 0
    second.load(name)
    second._inner_replay().load_full(name)
    assert int(second._feature.step_dev.item()) == 5 * A["k"] == second._feature.episodes.stamp
    for key in ("env_state", "env_counter", "ep_steps", "ep_return"):
        assert torch.equal(getattr(second.actor._task, key), getattr(first.actor._task, key)), key
    second._fused.state1.copy_(first._fused.state1)
    second._fused.state2.copy_(first._fused.state2)
    second._target_flat.flat.copy_(first._target_flat.flat)
    for tb, b in zip(second.target_network.buffers(), first.target_network.buffers()):
        tb.copy_(b)
    second._fused.steps, second.total_steps, second.actor._total_steps = first._fused.steps, first.total_steps, first.actor._total_steps
    second.config.replay_beta.current = first.config.replay_beta.current
    np.random.set_state(rng[0])
    random.setstate(rng[1])
    torch.set_rng_state(rng[2])
    for _ in range(5):
        second.step()
    second.drain_episodes()
    got = _snapshot(second, rec2, draws2)
    first.close()
    second.close()
    assert (got['total'], got['pos'], got['size'], got['write'], got['pending'], got['beta']) == (
        whole['total'], whole['pos'], whole['size'], whole['write'], whole['pending'], whole['beta'])
    assert [ln for ln in rec.lines if 'episodic_return_train' in ln] + got['lines'] == whole['lines']
    for x, y in zip(got['rng'], whole['rng']):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert len(draws) == 4 and len(draws2) == 5
    for x, y in zip(draws + draws2, whole['draws']):
        assert np.array_equal(x['leaves'], y['leaves']) and np.array_equal(_bits(x['prob']), _bits(y['prob']))
    for k in got['ring']:
        assert np.array_equal(_bits(got['ring'][k]), _bits(whole['ring'][k])), k
    assert np.array_equal(_bits(got['tree']), _bits(whole['tree']))
    for k in got['state']:
        assert np.array_equal(_bits(got['state'][k]), _bits(whole['state'][k])), k


def test_default_config_stays_on_the_host_and_a_wrong_setup_is_told_why(dra, monkeypatch):
    """Without the switch the agent keeps the host loop silently; with it, a UniformReplay is refused with the reason, once, and
    the agent runs on the host."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd.replay import ReplayWrapper, UniformReplay
    d = dra
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    agent = d.CategoricalDQNAgent(_config(d, False))
    assert agent._feature is None and not rec.warnings
    agent.close()
    c = _config(d, True)
    c.replay_fn = lambda: ReplayWrapper(UniformReplay, dict(memory_size=32, batch_size=8, n_step=3, discount=0.99, history_length=1), False)
    agent = d.CategoricalDQNAgent(c)
    assert agent._feature is None and len(rec.warnings) == 1 and "the replay is not a PrioritizedReplay" in rec.warnings[0]
    agent.step()
    agent.close()


def test_closed_loop_learns(dra, monkeypatch):
    """The zoo entry itself (hidden 64, 50 atoms on [-100, 100], a PrioritizedReplay of 10^4 with n_step 3, minibatches of 32,
    exploration_steps 1000, a target copy every 200 updates) with config.fused_rainbow_feature and the update kernel for the
    number of environment steps at which the REFERENCE's own median over five seeds reaches 2 x the bar
    (tests/golden/rainbow_feature/learning_reference.json: n_learn = 25 000, where its median is 166.9): the median over three
    seeds of the mean return of the last 100 training episodes reaches the bar, 2 x the random policy's mean (44.2)."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    from deeprl_amd.device_env import DeviceCartPoleVec
    d = dra
    ref = json.load(open(os.path.join(GOLDEN, "rainbow_feature", "learning_reference.json")))
    bar, n_learn = ref["bar"], ref["n_learn"]
    assert bar == 2.0 * json.load(open(os.path.join(GOLDEN, "dqn_feature", "random_policy.json")))["mean"] and abs(bar - 44.2) < 0.1
    assert n_learn == 25000
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    means = []
    for seed in LEARN_SEEDS:
        d.random_seed(seed)
        torch.manual_seed(seed)
        random.seed(seed)
        c = zoo.config("rainbow_feature", game=GAME, tag="rainbow_feat_learn_%d" % seed, async_replay=False, fused_rainbow_feature=True,
                       fused_rainbow_update=True)
        c.task_fn = lambda seed=seed, c=c: d.Task(c.game, seed=seed)
        c.log_interval = 10 ** 9
        agent = d.CategoricalDQNAgent(c)
        assert isinstance(agent.actor._task, DeviceCartPoleVec)
        returns = []
        while agent.total_steps < n_learn:
            agent.step()
            if agent.total_steps % 4096 == 0:
                returns += [r for _, r in agent.episodes()]
        returns += [r for _, r in agent.episodes()]
        agent._feature.check()
        agent.close()
        means.append(float(np.mean(returns[-LAST_EPISODES:])))
        print("seed %d: %d episodes, last-%d mean %.2f" % (seed, len(returns), LAST_EPISODES, means[-1]))
    median = float(np.median(means))
    record_parity("rainbow_feature closed loop: last-100 mean returns per seed, median, bar", median=median, bar=bar,
                  **{"seed%d" % s: m for s, m in zip(LEARN_SEEDS, means)})
    assert median >= bar, (means, bar)
