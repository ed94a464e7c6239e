"""Seeds of categorical_dqn_feature / quantile_regression_dqn_feature as lanes of the same launches (deeprl_amd/seed_batch.py,
zoo.run_seeds): lane k of a batch against the single config.fused_dist_feature agent of seed k with config.fused_dist_update True
(the form the lanes always run), bit for bit; graph replay against eager steps; the refusals by name; the closed loop of the three
learning seeds in one batch against the reference-derived bar.

The small configuration is dist_feature_cases.AGENT (one cart-pole with episodes of at most 5 steps, 4 transitions per step,
minibatches of 10 from a replay of 24 slots that wraps in the seventh step, a target copy every 3 steps, epsilon from 0.8 to 0.1
over 30 calls, 20 atoms on [-10, 10] / 20 quantiles) with exploration_steps 14 and 10 steps, so that both regions are captured and
replayed (tests/test_gpu_dist_feature.py::test_graph_replay_equals_eager's variant)."""
import json
import os

import numpy as np
import pytest
import torch
from feature_kernel_harness import GAME, dra, _Rec, _bits      # noqa: F401  (dra: the fixture)

import dist_feature_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dist_feature")
ENTRY = {"c51": "categorical_dqn_feature", "qr": "quantile_regression_dqn_feature"}

A = dict(K.AGENT, exploration_steps=14, steps=10)
SEEDS = (3, 11, 12)


def _seeds_cls(head):
    from deeprl_amd import seed_batch
    return seed_batch.CategoricalDQNFeatureSeeds if head == "c51" else seed_batch.QuantileRegressionDQNFeatureSeeds


def _agent_cls(d, head):
    return d.CategoricalDQNAgent if head == "c51" else d.QuantileRegressionDQNAgent


def _atoms(head, n):
    return dict(categorical_n_atoms=n) if head == "c51" else dict(num_quantiles=n)


def _maker(d, head, graph=True, per_seed=None, **extra):
    """make_config(seed) over the small configuration; per_seed(seed, config) may change one lane's.  No switch is set here: the
    batch sets its own, the single agent's are passed in `extra`."""
    from deeprl_amd import zoo
    from deeprl_amd.replay import ReplayWrapper, UniformReplay
    shape = dict(_atoms(head, A["n"]), **(dict(categorical_v_min=A["v_min"], categorical_v_max=A["v_max"]) if head == "c51" else {}))

    def make_config(seed):
        c = zoo.config(ENTRY[head], game=GAME, tag="dist_lanes_%s%d" % (head, seed), graph_update=graph,
                       overrides=dict(sgd_update_frequency=A["k"], batch_size=A["batch"], target_network_update_freq=A["target_freq"],
                                      exploration_steps=A["exploration_steps"], double_q=A["double_q"], **shape, **extra))
        c.task_fn = lambda: d.Task(c.game, seed=seed, synthetic_done_period=A["horizon"])
        rk = dict(memory_size=A["capacity"], batch_size=A["batch"])
        c.replay_fn = lambda: ReplayWrapper(UniformReplay, rk, False)
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
                loss=agent._feature.loss.cpu().numpy(),
                lines=[ln for ln in agent.logger.lines if 'episodic_return_train' in ln])


def _single(d, head, seed, steps=A["steps"], **kw):
    """The single agent of `seed` on the update kernel, built as the batch builds a lane, stepped `steps` times."""
    from deeprl_amd.dist_mlp import Step
    d.random_seed(seed)
    torch.manual_seed(seed)
    agent = _agent_cls(d, head)(_maker(d, head, fused_dist_feature=True, fused_dist_update=True, **kw)(seed))
    assert type(agent._feature) is Step
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


def _batched(d, head, seeds, steps=A["steps"], **kw):
    batch = _seeds_cls(head)(_maker(d, head, **kw), seeds)
    assert all(batch.lane(k).config.fused_dist_update is True and batch.lane(k).config.fused_dist_feature is True for k in range(len(seeds)))
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
    for k in ("flat", "target_flat", "state1", "state2", "loss"):
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


_SINGLES, _LANES = {}, {}


def _shared(cache, head, make):
    """Computed once per head kind, shared by the tests below, left unchanged."""
    if head not in cache:
        mp = pytest.MonkeyPatch()
        try:
            _quiet(mp)
            cache[head] = make()
        finally:
            mp.undo()
    return cache[head]


@pytest.fixture
def singles(dra, request):
    """The three single runs, one after another."""
    head = request.node.callspec.params["head"]
    return _shared(_SINGLES, head, lambda: {s: _single(dra, head, s) for s in SEEDS})


@pytest.fixture
def lanes(dra, request):
    """The batch over the same seeds with graph replay."""
    head = request.node.callspec.params["head"]
    return _shared(_LANES, head, lambda: _batched(dra, head, SEEDS))


@pytest.mark.parametrize("head", K.HEADS)
def test_lanes_equal_the_single_agents(dra, head, singles, lanes):
    """A batch over seeds (3, 11, 12) for 10 agent steps -- three acting steps (two eager, the capture with its replay), then seven
    learning steps (two eager, the capture, replays) with target copies between replays -- against the three single agents with
    config.fused_dist_update True: per lane the online and target parameters, the optimiser's two state buffers and its step count,
    the last loss, the ring's four arrays and cursor, the sampled indices, the actions, total_steps, the kernel's step counter, the
    schedule's position, the episode (step, return) pairs and log lines, and three randint draws of rng_tail(k) against the single
    run's np.random tail are equal to the bit.  (_batched asserts that the global np.random state is what it was when construction
    finished, and that the batch set both switches.)"""
    assert lanes["graphed"] == dict(act=True, learn=True) and lanes["launches"] == 3 + 3
    assert all(s["graphed"] == dict(act=True, learn=True) for s in singles.values())
    for k, seed in enumerate(SEEDS):
        _assert_lane_is(lanes["lanes"][k], singles[seed], "seed %d" % seed)
        assert len(singles[seed]["events"]) >= 8 and singles[seed]["size"] == A["capacity"]      # (episodes ended; the ring wrapped)
        assert singles[seed]["opt_steps"] >= 1 and np.isfinite(singles[seed]["loss"]).all()
    a, b = (singles[s] for s in SEEDS[:2])
    assert not np.array_equal(a["flat"], b["flat"]) and not np.array_equal(a["actions"], b["actions"])      # (the seeds differ)


@pytest.mark.parametrize("head", K.HEADS)
def test_lanes_graph_replay_equals_eager(dra, monkeypatch, head, lanes):
    """config.graph_update False on the lanes keeps every step eager: the same bits as graph replay, per lane."""
    _quiet(monkeypatch)
    eager = _batched(dra, head, SEEDS, graph=False)
    assert eager["graphed"] == dict(act=False, learn=False) and eager["launches"] == A["steps"]
    for k, seed in enumerate(SEEDS):
        _assert_lane_is(eager["lanes"][k], lanes["lanes"][k], "eager seed %d" % seed)


@pytest.mark.parametrize("head", K.HEADS)
def test_one_lane_batch_equals_the_single_agent(dra, monkeypatch, head, singles):
    _quiet(monkeypatch)
    one = _batched(dra, head, (11,))
    assert one["graphed"] == dict(act=True, learn=True)
    _assert_lane_is(one["lanes"][0], singles[11], "a batch of one")


def _one_lane_differs(seed, change):
    return lambda s, c: change(c) if s == seed else None


@pytest.mark.parametrize("head", K.HEADS)
def test_refusals_name_their_reason(dra, monkeypatch, head):
    from deeprl_amd import zoo
    d = dra
    _quiet(monkeypatch)
    cls = _seeds_cls(head)

    def atoms(c):
        for k, v in _atoms(head, A["n"] + 1).items():
            setattr(c, k, v)

    def module_update(c):
        c.fused_dist_update = False

    def fused_eval(c):
        c.fused_eval = True

    def adam(c):
        c.optimizer_fn = lambda p: torch.optim.Adam(p, 0.001)
    cases = ((dict(per_seed=_one_lane_differs(11, atoms)), SEEDS, r"lane 1 differs from lane 0 in n_atoms \(21, lane 0: 20\)"),
             (dict(per_seed=_one_lane_differs(12, module_update)), SEEDS,
              "seed 12 cannot run as a lane: config.fused_dist_update is off: the module-path update has no lane form"),
             (dict(per_seed=_one_lane_differs(3, fused_eval)), SEEDS, "seed 3 cannot run as a lane: config.fused_eval is on"),
             (dict(per_seed=_one_lane_differs(3, adam)), SEEDS, "seed 3 cannot run as a lane: the optimizer is not RMSprop"),
             (dict(), range(65), "%s runs 1 to 64 seeds as lanes, not 65" % cls.__name__))
    for kw, seeds, why in cases:
        with pytest.raises(ValueError, match=why):
            cls(_maker(d, head, **kw), seeds)
    with pytest.raises(ValueError, match="rainbow_feature has no lane form"):
        zoo.run_seeds("rainbow_feature", SEEDS, game=GAME)
    with pytest.raises(ValueError, match="config.fused_dist_update is off"):
        zoo.run_seeds(ENTRY[head], SEEDS, game=GAME, tag="dist_lanes_refused", fused_dist_update=False)


@pytest.mark.parametrize("head", K.HEADS)
def test_run_seeds_learns(dra, monkeypatch, head):
    """zoo.run_seeds(entry, K.LEARN_SEEDS) at the zoo configuration up to n_learn of
    tests/golden/dist_feature/learning_reference.json: the median over the lanes of the mean return of the last 100 training
    episodes reaches that file's bar -- tests/test_gpu_dist_feature.py::test_closed_loop_learns' condition on the same seeds, one
    batch instead of three runs."""
    from parity_log import record_parity
    from deeprl_amd import zoo
    ref = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))[head]
    bar, n_learn = ref["bar"], ref["n_learn"]
    assert n_learn is not None and abs(bar - 44.2) < 0.1
    _quiet(monkeypatch)
    runs = zoo.run_seeds(ENTRY[head], K.LEARN_SEEDS, game=GAME, tag="dist_lanes_learn_%s" % head, max_steps=n_learn)
    assert len(runs) == len(K.LEARN_SEEDS)
    means = []
    for seed, pairs in zip(K.LEARN_SEEDS, runs):
        assert all(0 < s <= n_learn for s, _ in pairs) and [s for s, _ in pairs] == sorted(s for s, _ in pairs)
        means.append(float(np.mean([r for _, r in pairs][-K.LAST_EPISODES:])))
        print("seed %d: %d episodes, last-%d mean %.2f" % (seed, len(pairs), K.LAST_EPISODES, means[-1]))
    median = float(np.median(means))
    record_parity("dist_feature %s seed lanes closed loop: last-100 mean returns per seed, median, bar" % head, median=median, bar=bar,
                  **{"seed%d" % s: m for s, m in zip(K.LEARN_SEEDS, means)})
    assert median >= bar, (means, bar)
