"""Seeds of dqn_feature as lanes of the same launches (deeprl_amd/seed_batch.py, zoo.run_seeds): lane k of a DQNFeatureSeeds batch
against the single config.fused_dqn_feature agent of seed k, bit for bit; graph replay against eager steps; the refusals by name;
the closed loop of the three learning seeds in one batch against the reference-derived bar.

The small configuration is tests/test_gpu_dqn_feature.py's, restated: one cart-pole with episodes of at most 5 steps, 4
transitions per step, minibatches of 10 from a replay of 24 slots that wraps (in the seventh step), a target copy every 3 steps,
epsilon from 0.8 to 0.1 over 30 calls; exploration_steps 14, so that both regions are captured and replayed within 10 steps."""
import json
import os

import numpy as np
import pytest
import torch
from feature_kernel_harness import GAME, dra, _Rec, _bits      # noqa: F401  (dra: the fixture)

import dqn_feature_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dqn_feature")

A = dict(k=4, batch=10, capacity=24, target_freq=3, horizon=5, eps=(0.8, 0.1, 30), discount=0.99, exploration_steps=14, steps=10)
SEEDS = (3, 11, 12)


def _maker(d, graph=True, n_step=1, replay_cls=None, per_seed=None, **extra):
    """make_config(seed) over the small configuration; per_seed(seed, config) may change one lane's."""
    from deeprl_amd import zoo
    from deeprl_amd.replay import ReplayWrapper, UniformReplay

    def make_config(seed):
        c = zoo.config("dqn_feature", game=GAME, tag="dqn_lanes%d" % seed, graph_update=graph, n_step=n_step, fused_dqn_feature=True,
                       overrides=dict(sgd_update_frequency=A["k"], batch_size=A["batch"], target_network_update_freq=A["target_freq"],
                                      exploration_steps=A["exploration_steps"], double_q=False, **extra))
        c.task_fn = lambda: d.Task(c.game, seed=seed, synthetic_done_period=A["horizon"])
        rk = dict(memory_size=A["capacity"], batch_size=A["batch"], n_step=n_step, discount=A["discount"], history_length=1)
        c.replay_fn = lambda: ReplayWrapper(replay_cls or UniformReplay, rk, False)
        c.random_action_prob = d.LinearSchedule(*A["eps"])
        c.log_interval = 10 ** 9
        if per_seed is not None:
            per_seed(seed, c)
        return c
    return make_config


def _quiet(monkeypatch):
    import deeprl_amd.agents as agents_mod
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())


def _lane_state(agent):
    """What a run leaves in `agent`, as host arrays."""
    torch.cuda.synchronize()
    rp = agent._inner_replay()
    frames, actions, rewards, masks = rp._ring.arrays()
    return dict(params={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
                target={k: v.detach().cpu().numpy().copy() for k, v in agent.target_network.state_dict().items()},
                flat=agent._fused.flat.flat.cpu().numpy(), target_flat=agent._target_flat.flat.cpu().numpy(),
                state1=agent._fused.state1.cpu().numpy(), state2=agent._fused.state2.cpu().numpy(), opt_steps=agent._fused.steps,
                ring=dict(frames=frames.view(torch.float64).cpu().numpy(), actions=actions.view(torch.int64).cpu().numpy(),
                          rewards=rewards.cpu().numpy(), masks=masks.cpu().numpy()),
                pos=rp.pos, size=rp.size(), total=agent.total_steps, actor_total=agent.actor._total_steps,
                epsilon=agent.config.random_action_prob.current, step_dev=int(agent._feature.step_dev.item()),
                lines=[ln for ln in agent.logger.lines if 'episodic_return_train' in ln])


def _single(d, seed, steps=A["steps"], **kw):
    """The single agent of `seed`, built as DQNFeatureSeeds builds a lane, stepped `steps` times."""
    d.random_seed(seed)
    torch.manual_seed(seed)
    agent = d.DQNAgent(_maker(d, **kw)(seed))
    assert type(agent._feature).__name__ == "Step"
    actions, indices = [], []
    for _ in range(steps):
        agent.step()
        actions.append(agent._feature.out_action.cpu().numpy().copy())
        indices.append(agent._feature.last_draws[3])
    events = agent.episodes()
    out = _lane_state(agent)
    out.update(actions=np.asarray(actions), indices=indices, events=events, rng=np.random.randint(0, 1 << 30, size=3),
               graphed={k: r.graph is not None for k, r in agent._feature.regions.items()})
    agent.close()
    return out


def _batched(d, seeds, steps=A["steps"], **kw):
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    batch = DQNFeatureSeeds(_maker(d, **kw), seeds)
    built = np.random.get_state()
    actions, indices = [[] for _ in seeds], [[] for _ in seeds]
    for _ in range(steps):
        batch.step()
        for k in range(len(seeds)):
            actions[k].append(batch.lane(k)._feature.out_action.cpu().numpy().copy())
            indices[k].append(batch.lane(k)._feature.last_draws[3])
    assert batch.total_steps == steps * A["k"]
    after = np.random.get_state()
    assert built[0] == after[0] and np.array_equal(built[1], after[1]) and built[2:] == after[2:]      # the global stream stayed put
    lanes = []
    for k in range(len(seeds)):
        events = batch.episodes(k)
        out = _lane_state(batch.lane(k))
        out.update(actions=np.asarray(actions[k]), indices=indices[k], events=events, rng=batch.rng_tail(k).randint(0, 1 << 30, size=3))
        lanes.append(out)
    graphed = {k: r.graph is not None for k, r in batch.regions.items()}
    launches = batch.launches
    batch.close()
    return dict(lanes=lanes, graphed=graphed, launches=launches)


def _assert_lane_is(got, want, what):
    for k in ("flat", "target_flat", "state1", "state2"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)
    for name in want["params"]:
        assert np.array_equal(_bits(got["params"][name]), _bits(want["params"][name])), (what, name)
        assert np.array_equal(_bits(got["target"][name]), _bits(want["target"][name])), (what, "target " + name)
    for k in want["ring"]:
        assert np.array_equal(_bits(got["ring"][k]), _bits(want["ring"][k])), (what, "ring " + k)
    for k in ("pos", "size", "total", "actor_total", "epsilon", "step_dev", "opt_steps", "events", "lines"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["actions"], want["actions"]), what
    assert len(got["indices"]) == len(want["indices"])
    assert all((i is None and j is None) or np.array_equal(i, j) for i, j in zip(got["indices"], want["indices"])), what
    assert np.array_equal(got["rng"], want["rng"]), (what, "np.random tail")


@pytest.fixture(scope="module")
def singles(dra):
    """The three single runs, one after another: shared by the tests below, left unchanged."""
    mp = pytest.MonkeyPatch()
    try:
        _quiet(mp)
        return {s: _single(dra, s) for s in SEEDS}
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def lanes(dra):
    """The batch over the same seeds with graph replay."""
    mp = pytest.MonkeyPatch()
    try:
        _quiet(mp)
        return _batched(dra, SEEDS)
    finally:
        mp.undo()


def test_lanes_equal_the_single_agents(dra, singles, lanes):
    """DQNFeatureSeeds over seeds (3, 11, 12) for 10 agent steps -- three acting steps (two eager, the capture with its replay),
    then seven learning steps (two eager, the capture, replays) with target copies between replays -- against the three single
    agents: per lane the online and target parameters, the optimiser's two state buffers and its step count, the ring's four
    arrays and cursor, the sampled indices, the actions, total_steps, the kernel's step counter, the schedule's position, the
    episode (step, return) pairs and log lines, and three randint draws of rng_tail(k) against the single run's np.random tail are
    equal to the bit.  (_batched asserts that the global np.random state is what it was when construction finished.)"""
    assert lanes["graphed"] == dict(act=True, learn=True) and lanes["launches"] == 3 + 3
    assert all(s["graphed"] == dict(act=True, learn=True) for s in singles.values())
    for k, seed in enumerate(SEEDS):
        _assert_lane_is(lanes["lanes"][k], singles[seed], "seed %d" % seed)
        assert len(singles[seed]["events"]) >= 8 and singles[seed]["size"] == A["capacity"]      # (episodes ended; the ring wrapped)
    a, b = (singles[s] for s in SEEDS[:2])
    assert not np.array_equal(a["flat"], b["flat"]) and not np.array_equal(a["actions"], b["actions"])      # (the seeds differ)


def test_lanes_graph_replay_equals_eager(dra, monkeypatch, lanes):
    """config.graph_update False on the lanes keeps every step eager: the same bits as graph replay, per lane."""
    _quiet(monkeypatch)
    eager = _batched(dra, SEEDS, graph=False)
    assert eager["graphed"] == dict(act=False, learn=False) and eager["launches"] == A["steps"]
    for k, seed in enumerate(SEEDS):
        _assert_lane_is(eager["lanes"][k], lanes["lanes"][k], "eager seed %d" % seed)


def test_one_lane_batch_equals_the_single_agent(dra, monkeypatch, singles):
    _quiet(monkeypatch)
    one = _batched(dra, (11,))
    assert one["graphed"] == dict(act=True, learn=True)
    _assert_lane_is(one["lanes"][0], singles[11], "a batch of one")


def test_lane_surface_sees_live_buffers(dra, monkeypatch, tmp_path):
    """lane(k) is the underlying agent: its save() writes the lane's live parameters and environment, and what drain_episodes()
    returns per lane is what episodes(k) would have."""
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    _quiet(monkeypatch)
    batch = DQNFeatureSeeds(_maker(dra), (3, 11))
    for _ in range(6):
        batch.step()
    drained = batch.drain_episodes()
    assert len(drained) == 2 and all(len(x) >= 3 for x in drained)
    assert batch.episodes(1) == drained[1] and batch.episodes(1) == []
    name = str(tmp_path / "lane1")
    batch.lane(1).save(name)
    weights = torch.load(name + ".model")
    for k, v in batch.lane(1).network.state_dict().items():
        assert torch.equal(weights[k], v.detach().cpu())
    assert os.path.isfile(name + ".envs")
    batch.close()
    batch.close()      # (a second close is a no-op)


def _one_lane_differs(seed, change):
    return lambda s, c: change(c) if s == seed else None


def test_refusals_name_their_reason(dra, monkeypatch):
    from deeprl_amd import zoo
    from deeprl_amd.replay import PrioritizedReplay
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    d = dra
    _quiet(monkeypatch)

    def clip(c):
        c.gradient_clip = 4

    def dueling(c):
        c.network_fn = lambda: d.DuelingNet(c.action_dim, d.FCBody(c.state_dim))

    def module_update(c):
        c.fused_dqn_update = False

    def fused_eval(c):
        c.fused_eval = True

    def adam(c):
        c.optimizer_fn = lambda p: torch.optim.Adam(p, 0.001)
    cases = ((dict(per_seed=_one_lane_differs(11, clip)), SEEDS, r"lane 1 differs from lane 0 in gradient_clip \(4, lane 0: 5\)"),
             (dict(per_seed=_one_lane_differs(11, dueling)), SEEDS, "seed 11 cannot run as a lane: the network is not VanillaNet"),
             (dict(n_step=3), SEEDS, "seed 3 cannot run as a lane: n_step is not 1"),
             (dict(replay_cls=PrioritizedReplay), SEEDS, "seed 3 cannot run as a lane: the replay is a PrioritizedReplay"),
             (dict(per_seed=_one_lane_differs(12, module_update)), SEEDS, "seed 12 cannot run as a lane: config.fused_dqn_update is off"),
             (dict(per_seed=_one_lane_differs(3, fused_eval)), SEEDS, "seed 3 cannot run as a lane: config.fused_eval is on"),
             (dict(per_seed=_one_lane_differs(3, adam)), SEEDS, "seed 3 cannot run as a lane: the optimizer is not RMSprop"),
             (dict(), range(65), "runs 1 to 64 seeds as lanes, not 65"))
    for kw, seeds, why in cases:
        with pytest.raises(ValueError, match=why):
            DQNFeatureSeeds(_maker(d, **kw), seeds)
    with pytest.raises(ValueError, match="a2c_feature has no lane form"):
        zoo.run_seeds("a2c_feature", SEEDS, game=GAME)
    with pytest.raises(ValueError, match="n_step is not 1"):
        zoo.run_seeds("dqn_feature", SEEDS, game=GAME, tag="lanes_refused", n_step=3)
    with pytest.raises(ValueError, match="the replay is a PrioritizedReplay"):
        zoo.run_seeds("dqn_feature", SEEDS, game=GAME, tag="lanes_refused", replay_cls=PrioritizedReplay)


def test_run_seeds_learns(dra, monkeypatch):
    """zoo.run_seeds("dqn_feature", K.LEARN_SEEDS) at the zoo configuration up to n_learn of
    tests/golden/dqn_feature/learning_reference.json: the median over the lanes of the mean return of the last 100 training
    episodes reaches that file's bar -- tests/test_gpu_dqn_feature.py::test_closed_loop_learns' condition on the same seeds, one
    batch instead of three runs."""
    from parity_log import record_parity
    from deeprl_amd import zoo
    ref = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))
    bar, n_learn = ref["bar"], ref["n_learn"]
    assert n_learn is not None and abs(bar - 44.2) < 0.1
    _quiet(monkeypatch)
    runs = zoo.run_seeds("dqn_feature", K.LEARN_SEEDS, game=GAME, tag="dqn_lanes_learn", max_steps=n_learn)
    assert len(runs) == len(K.LEARN_SEEDS)
    means = []
    for seed, pairs in zip(K.LEARN_SEEDS, runs):
        assert all(0 < s <= n_learn for s, _ in pairs) and [s for s, _ in pairs] == sorted(s for s, _ in pairs)
        means.append(float(np.mean([r for _, r in pairs][-K.LAST_EPISODES:])))
        print("seed %d: %d episodes, last-%d mean %.2f" % (seed, len(pairs), K.LAST_EPISODES, means[-1]))
    median = float(np.median(means))
    record_parity("dqn_feature seed lanes closed loop: last-100 mean returns per seed, median, bar", median=median, bar=bar,
                  **{"seed%d" % s: m for s, m in zip(K.LEARN_SEEDS, means)})
    assert median >= bar, (means, bar)
