"""Seeds of dqn_feature with an n-step window as lanes of the same launches (deeprl_amd/seed_batch.py: DQNReplayFeatureSeeds;
zoo.run_seeds(..., fused_dqn_replay_feature=True, n_step=N)): lane k of a batch against the single config.fused_dqn_replay_feature
agent of seed k, bit for bit -- with host draws, with device_draws, with eval_lanes; graph replay against eager steps; the new class
at n_step 1 against DQNFeatureSeeds' lanes; the refusals by name; the closed loop of the three learning seeds in one batch against
the reference-derived bar.

The small configuration is tests/test_gpu_dqn_lanes_agent.py's (4 transitions per step, minibatches of 10 from a replay of 24 slots
that wraps, episodes of at most 5 steps, exploration_steps 14, 10 agent steps: both regions are captured and replayed), with n_step 3
and 8.  At n_step 8 the first update draws from a ring of 16 rows of which 8 are valid, and after the wrap (pos 4) the low range of
valid indices is empty."""
import json
import os

import numpy as np
import pytest
import torch
from feature_kernel_harness import GAME, dra, _Rec, _bits      # noqa: F401  (dra: the fixture)

import dqn_replay_feature_cases as K
import test_gpu_dqn_lanes_agent as DQN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dqn_replay_feature")
A, SEEDS = DQN.A, DQN.SEEDS
N_STEPS = (3, 8)
EVAL_AFTER, EPISODES, EVAL_HORIZON = (0, 2, 6, 10), 3, 12      # tests/test_gpu_eval_lanes_agent.py's evaluation points


def _maker(d, n_step, single, graph=True, replay_cls=None, per_seed=None, **extra):
    """make_config(seed) over the small configuration with a window of n_step.  single: the switch as the single agent needs it (a
    batch sets its own)."""
    from deeprl_amd import zoo
    from deeprl_amd.replay import ReplayWrapper, UniformReplay
    switch = dict(fused_dqn_replay_feature=True) if single else {}
    overrides = dict(sgd_update_frequency=A["k"], batch_size=A["batch"], target_network_update_freq=A["target_freq"],
                     exploration_steps=A["exploration_steps"], double_q=False)
    overrides.update(extra)

    def make_config(seed):
        c = zoo.config("dqn_feature", game=GAME, tag="dqn_replay_lanes%d" % seed, graph_update=graph, n_step=n_step,
                       overrides=dict(overrides), **switch)
        c.task_fn = lambda: d.Task(c.game, seed=seed, synthetic_done_period=A["horizon"])
        rk = dict(memory_size=A["capacity"], batch_size=A["batch"], n_step=n_step, discount=A["discount"], history_length=1)
        c.replay_fn = lambda: ReplayWrapper(replay_cls or UniformReplay, rk, False)
        c.random_action_prob = d.LinearSchedule(*A["eps"])
        c.log_interval = 10 ** 9
        if per_seed is not None:
            per_seed(seed, c)
        return c
    return make_config


def _eval_env(d):
    def per_seed(seed, c):
        c.eval_env = d.Task(GAME, seed=1000 + seed, synthetic_done_period=EVAL_HORIZON)
    return per_seed


def _test_lines(agent):
    return [ln for ln in agent.logger.lines if 'episodic_return_test' in ln]


def _single(d, seed, n_step, evaluate=False, steps=A["steps"]):
    """The single agent of `seed`, built as DQNReplayFeatureSeeds builds a lane, stepped `steps` times; evaluate: with
    config.fused_eval, evaluated (agent.eval_episodes()) behind the agent steps of EVAL_AFTER."""
    from deeprl_amd import dqn_replay_mlp
    d.random_seed(seed)
    torch.manual_seed(seed)
    kw = dict(per_seed=_eval_env(d), eval_episodes=EPISODES, fused_eval=True) if evaluate else {}
    agent = d.DQNAgent(_maker(d, n_step, True, **kw)(seed))
    step = agent._feature
    assert type(step) is dqn_replay_mlp.Step, agent.logger.warnings
    returns, report = [], agent._report_eval

    def watched(r):
        returns.append(np.asarray(r, dtype=np.float64).copy())
        return report(r)
    agent._report_eval = watched
    actions, indices, evals = [], [], []
    for s in range(steps + 1):
        if evaluate and s in EVAL_AFTER:
            got = agent.eval_episodes()
            evals.append(dict(returns=returns[-1], lengths=step.eval_lengths.copy(), steps=int(step.eval_steps), total=agent.total_steps,
                              report=got))
        if s < steps:
            agent.step()
            actions.append(step.out_action.cpu().numpy().copy())
            indices.append(step.last_draws[3])
    step.check()
    events = agent.episodes()
    out = DQN._lane_state(agent)
    out.update(actions=np.asarray(actions), indices=indices, events=events, rng=np.random.randint(0, 1 << 30, size=3), evals=evals,
               test_lines=_test_lines(agent), graphed={k: r.graph is not None for k, r in step.regions.items()},
               eval_counts=(step.eval_launches, step.eval_copies))
    agent.close()
    return out


def _batched(d, seeds, n_step, graph=True, device_draws=False, eval_lanes=False, cls=None, maker=None, steps=A["steps"]):
    from deeprl_amd import seed_batch
    cls = cls or seed_batch.DQNReplayFeatureSeeds
    kw = dict(per_seed=_eval_env(d), eval_episodes=EPISODES) if eval_lanes else {}
    batch = cls(maker or _maker(d, n_step, False, graph=graph, **kw), seeds, device_draws=device_draws, eval_lanes=eval_lanes)
    assert batch.n_step == n_step
    assert cls is not seed_batch.DQNReplayFeatureSeeds or all(a.config.fused_dqn_replay_feature is True for a in batch.agents)
    built = np.random.get_state()
    n = len(seeds)
    actions, indices, evals, draws = [[] for _ in seeds], [[] for _ in seeds], [[] for _ in seeds], [[] for _ in seeds]
    for s in range(steps + 1):
        if eval_lanes and s in EVAL_AFTER:
            reports = batch.eval_episodes()
            for k in range(n):
                evals[k].append(dict(returns=batch.eval_returns[k].copy(), lengths=batch.eval_lengths[k].copy(), steps=int(batch.eval_steps[k]),
                                     total=batch.lane(k).total_steps, report=reports[k]))
        if s < steps:
            batch.step()
            for k in range(n):
                actions[k].append(batch.lane(k)._feature.out_action.cpu().numpy().copy())
                draws[k].append(batch.fetch_draws(k))
                indices[k].append(draws[k][-1][3])
    assert batch.total_steps == steps * A["k"]
    batch.check()
    after = np.random.get_state()
    assert built[0] == after[0] and np.array_equal(built[1], after[1]) and built[2:] == after[2:]      # the global stream stayed put
    lanes = []
    for k in range(n):
        events = batch.episodes(k)
        out = DQN._lane_state(batch.lane(k))
        out.update(actions=np.asarray(actions[k]), indices=indices[k], events=events, rng=batch.rng_tail(k).randint(0, 1 << 30, size=3),
                   evals=evals[k], test_lines=_test_lines(batch.lane(k)), draws=draws[k])
        lanes.append(out)
    out = dict(lanes=lanes, graphed={k: r.graph is not None for k, r in batch.regions.items()}, launches=batch.launches,
               eval_counts=(batch.eval_launches, batch.eval_copies) if eval_lanes else None)
    batch.close()
    return out


_RUNS = {}


def _cached(key, make):
    """Runs shared by the tests below: computed once on first use under a quiet logger, left unchanged."""
    if key not in _RUNS:
        mp = pytest.MonkeyPatch()
        try:
            DQN._quiet(mp)
            _RUNS[key] = make()
        finally:
            mp.undo()
    return _RUNS[key]


def _singles(d, n_step, evaluate=False):
    return _cached(("single", n_step, evaluate), lambda: {s: _single(d, s, n_step, evaluate) for s in SEEDS})


def _lanes(d, n_step):
    return _cached(("lanes", n_step), lambda: _batched(d, SEEDS, n_step))


def _assert_draws_equal(got, want, what):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2], (what, s)
        assert (g[3] is None and w[3] is None) or np.array_equal(g[3], w[3]), (what, s)


@pytest.mark.parametrize("n_step", N_STEPS)
def test_lanes_equal_the_single_agents(dra, n_step):
    """DQNReplayFeatureSeeds over seeds (3, 11, 12) for 10 agent steps -- three acting steps, then seven learning steps with target
    copies between replays -- against the three single config.fused_dqn_replay_feature agents: per lane the online and target
    parameters, the optimiser's two state buffers and its step count, the ring's four arrays and cursor, the sampled indices (all
    valid over the window), the actions, total_steps, the kernel's step counter, the schedule's position, the episode (step,
    return) pairs and log lines, and three randint draws of rng_tail(k) against the single run's np.random tail, to the bit."""
    singles, lanes = _singles(dra, n_step), _lanes(dra, n_step)
    assert lanes["graphed"] == dict(act=True, learn=True) and lanes["launches"] == 3 + 3
    assert all(s["graphed"] == dict(act=True, learn=True) for s in singles.values())
    for k, seed in enumerate(SEEDS):
        DQN._assert_lane_is(lanes["lanes"][k], singles[seed], "n_step %d seed %d" % (n_step, seed))
        assert len(singles[seed]["events"]) >= 8 and singles[seed]["size"] == A["capacity"] and singles[seed]["opt_steps"] == 7
        assert sum(i is not None for i in singles[seed]["indices"]) == 7
    a, b = (singles[s] for s in SEEDS[:2])
    assert not np.array_equal(a["flat"], b["flat"]) and not np.array_equal(a["actions"], b["actions"])      # (the seeds differ)
    one = _singles(dra, N_STEPS[0])[SEEDS[0]]
    other = _singles(dra, N_STEPS[1])[SEEDS[0]]
    assert not np.array_equal(one["flat"], other["flat"])      # (the window matters)


@pytest.mark.parametrize("n_step", N_STEPS)
def test_lanes_with_device_draws_equal_the_single_agents(dra, monkeypatch, n_step):
    """The same with device_draws=True: every lane's indices drawn valid over the window by dra_np_mt_draw_window_lanes.  What
    fetch_draws(k) copies back after every step equals the host-draw batch's last_draws; the lanes end where the single runs end,
    rng_tail included."""
    DQN._quiet(monkeypatch)
    singles, host = _singles(dra, n_step), _lanes(dra, n_step)
    device = _batched(dra, SEEDS, n_step, device_draws=True)
    assert device["graphed"] == dict(act=True, learn=True) and device["launches"] == 2 * (3 + 3)      # (a draw launch per acting launch)
    for k, seed in enumerate(SEEDS):
        DQN._assert_lane_is(device["lanes"][k], singles[seed], "device draws, n_step %d seed %d" % (n_step, seed))
        _assert_draws_equal(device["lanes"][k]["draws"], host["lanes"][k]["draws"], (n_step, seed))


def test_lanes_evaluate_as_the_single_agents(dra, monkeypatch):
    """eval_lanes=True (with host draws and with device_draws) at n_step 3 against the three single agents with
    config.fused_eval: at each of the four evaluations the returns, lengths, steps and the reported dict, the logged
    'episodic_return_test' lines, one launch and one copy per evaluation for the three lanes; at the end everything the test above
    compares."""
    DQN._quiet(monkeypatch)
    singles = _singles(dra, 3, evaluate=True)
    for device_draws in (False, True):
        got = _batched(dra, SEEDS, 3, device_draws=device_draws, eval_lanes=True)
        assert got["eval_counts"] == (len(EVAL_AFTER),) * 2 and got["graphed"] == dict(act=True, learn=True)
        for k, seed in enumerate(SEEDS):
            lane, want = got["lanes"][k], singles[seed]
            what = "eval lanes, device_draws %d, seed %d" % (device_draws, seed)
            assert want["eval_counts"] == (len(EVAL_AFTER),) * 2 and len(lane["evals"]) == len(want["evals"]) == len(EVAL_AFTER)
            for i, (g, w) in enumerate(zip(lane["evals"], want["evals"])):
                assert g["total"] == w["total"] == EVAL_AFTER[i] * A["k"], (what, i)
                assert g["returns"].dtype == np.float64 and np.array_equal(_bits(g["returns"]), _bits(w["returns"])), (what, i)
                assert np.array_equal(g["lengths"], w["lengths"]) and g["steps"] == w["steps"] == int(w["lengths"].sum()), (what, i)
                assert g["report"] == w["report"], (what, i)
            assert lane["test_lines"] == want["test_lines"] and len(want["test_lines"]) == len(EVAL_AFTER)
            DQN._assert_lane_is(lane, want, what)


def test_lanes_graph_replay_equals_eager(dra, monkeypatch):
    """config.graph_update False on the lanes keeps every step eager: the same bits as graph replay, per lane."""
    DQN._quiet(monkeypatch)
    lanes = _lanes(dra, 3)
    eager = _batched(dra, SEEDS, 3, graph=False)
    assert eager["graphed"] == dict(act=False, learn=False) and eager["launches"] == A["steps"]
    for k, seed in enumerate(SEEDS):
        DQN._assert_lane_is(eager["lanes"][k], lanes["lanes"][k], "eager seed %d" % seed)


@pytest.mark.parametrize("device_draws", [False, True])
def test_window_of_one_equals_the_one_step_lanes(dra, monkeypatch, device_draws):
    """n_step 1 under DQNReplayFeatureSeeds against DQNFeatureSeeds' lanes on the same seeds: to the bit, draws included."""
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    DQN._quiet(monkeypatch)
    new = _batched(dra, SEEDS, 1, device_draws=device_draws)
    old = _batched(dra, SEEDS, 1, device_draws=device_draws, cls=DQNFeatureSeeds, maker=DQN._maker(dra))
    assert new["graphed"] == old["graphed"] == dict(act=True, learn=True) and new["launches"] == old["launches"]
    for k, seed in enumerate(SEEDS):
        DQN._assert_lane_is(new["lanes"][k], old["lanes"][k], "n_step 1 seed %d" % seed)
        _assert_draws_equal(new["lanes"][k]["draws"], old["lanes"][k]["draws"], seed)


def test_refusals_name_their_reason(dra, monkeypatch):
    from deeprl_amd import zoo
    from deeprl_amd.replay import PrioritizedReplay
    from deeprl_amd.seed_batch import DQNReplayFeatureSeeds
    d = dra
    DQN._quiet(monkeypatch)

    def module_update(c):
        c.fused_dqn_replay_update = False

    def fused_eval(c):
        c.fused_eval = True

    def adam(c):
        c.optimizer_fn = lambda p: torch.optim.Adam(p, 0.001)

    def window_of_two(seed):
        return _maker(d, 2 if seed == 12 else 3, False)(seed)
    one = DQN._one_lane_differs
    per = "seed 3 cannot run as a lane: the replay is a PrioritizedReplay: the prioritised draw and the priorities' commit have no lane form"
    cases = ((_maker(d, 3, False, replay_cls=PrioritizedReplay), SEEDS, per),
             (_maker(d, 3, False, per_seed=one(12, module_update)), SEEDS,
              "seed 12 cannot run as a lane: config.fused_dqn_replay_update is off: the module-path update has no lane form"),
             (_maker(d, 3, False, per_seed=one(3, fused_eval)), SEEDS, "seed 3 cannot run as a lane: config.fused_eval is on"),
             (_maker(d, 3, False, per_seed=one(3, adam)), SEEDS, "seed 3 cannot run as a lane: the optimizer is not RMSprop"),
             (window_of_two, SEEDS, r"lane 2 differs from lane 0 in n_step \(2, lane 0: 3\)"),
             (_maker(d, 9, False), SEEDS, "seed 3 cannot run as a lane: n_step is not between 1 and 8"),
             (_maker(d, 3, False), range(65), "runs 1 to 64 seeds as lanes, not 65"))
    for maker, seeds, why in cases:
        for device_draws in (False, True):
            with pytest.raises(ValueError, match=why):
                DQNReplayFeatureSeeds(maker, seeds, device_draws=device_draws)
    with pytest.raises(ValueError, match=per[len("seed 3 cannot run as a lane: "):]):
        zoo.run_seeds("dqn_feature", SEEDS, game=GAME, tag="replay_lanes_refused", fused_dqn_replay_feature=True, n_step=3,
                      replay_cls=PrioritizedReplay)
    with pytest.raises(ValueError, match="n_step is not 1"):      # (without the keyword nothing changes)
        zoo.run_seeds("dqn_feature", SEEDS, game=GAME, tag="replay_lanes_refused", n_step=3)


def test_a_ring_without_a_window_valid_index_is_refused_before_the_step(dra, monkeypatch):
    """exploration_steps 0 at n_step 8: the first agent step would update from a ring of 4 rows, none of which has 8 rows behind it.
    With device_draws the batch refuses the step by name on the host -- the kernel is never launched over such a ring -- and no
    lane has advanced."""
    from deeprl_amd.seed_batch import DQNReplayFeatureSeeds
    DQN._quiet(monkeypatch)
    batch = DQNReplayFeatureSeeds(_maker(dra, 8, False, exploration_steps=0), SEEDS, device_draws=True)
    try:
        with pytest.raises(ValueError, match="device_draws: a replay ring of size 4 at pos 4 holds no valid index over an n-step window "
                                             "of 8, the minibatch's rejection loop could not end"):
            batch.step()
        assert batch.total_steps == 0 and batch.launches == 0 and all(a._inner_replay().size() == 0 for a in batch.agents)
        batch.check()
    finally:
        batch.close()


RUN = dict(max_steps=24, overrides=dict(eval_interval=8, eval_episodes=EPISODES, exploration_steps=12, save_interval=0, log_interval=10 ** 9))


def test_run_seeds_gives_the_single_runs(dra, monkeypatch):
    """zoo.run_seeds("dqn_feature", seeds, fused_dqn_replay_feature=True, n_step=3, max_steps=...) at the zoo's configuration
    against support.run_steps over the single agent of each seed: per seed the same (step, return) list; with evaluate=True the
    same list again and the single fused_eval run's (step, returns) at zoo.eval_points' steps; device_draws changes neither."""
    from deeprl_amd import dqn_replay_mlp, zoo
    from deeprl_amd.support import run_steps
    DQN._quiet(monkeypatch)
    d = dra
    kw = dict(fused_dqn_replay_feature=True, n_step=3, game=GAME, tag="replay_lanes_run")
    plain = zoo.run_seeds("dqn_feature", SEEDS, max_steps=1500, **kw)
    assert zoo.run_seeds("dqn_feature", SEEDS, device_draws=True, max_steps=1500, **kw) == plain
    assert len(plain) == len(SEEDS) and all(len(pairs) >= 10 for pairs in plain)
    episodes, evaluations = zoo.run_seeds("dqn_feature", SEEDS, evaluate=True, **kw, **RUN)
    points = zoo.eval_points(RUN["max_steps"], RUN["overrides"]["eval_interval"], 4)
    assert points == [0, 8, 16, 24]
    for k, seed in enumerate(SEEDS):
        for evaluate in (False, True):
            d.random_seed(seed)
            torch.manual_seed(seed)
            if evaluate:
                c = zoo.config("dqn_feature", max_steps=RUN["max_steps"], overrides=dict(RUN["overrides"], fused_eval=True), **kw)
            else:
                c = zoo.config("dqn_feature", max_steps=1500, overrides=dict(eval_interval=0, save_interval=0, log_interval=10 ** 9), **kw)
            c.task_fn = lambda c=c: d.Task(c.game, seed=seed)
            agent = d.DQNAgent(c)
            step = agent._feature
            assert type(step) is dqn_replay_mlp.Step and c.n_step == 3
            want, report = [], agent._report_eval

            def watched(r, agent=agent, want=want, report=report):
                want.append((agent.total_steps, np.asarray(r, dtype=np.float64).copy()))
                return report(r)
            agent._report_eval = watched
            run_steps(agent)
            if evaluate:
                got = evaluations[k]
                assert [s for s, _ in got] == [s for s, _ in want] == points and step.eval_launches == len(points)
                for (_, g), (_, w) in zip(got, want):
                    assert g.shape == (EPISODES,) and np.array_equal(_bits(g), _bits(w)), (seed, g, w)
                assert episodes[k] == list(step.episodes.log)
            else:
                assert plain[k] == list(step.episodes.log) and want == []


def test_run_seeds_learns(dra, monkeypatch):
    """zoo.run_seeds("dqn_feature", K.LEARN_SEEDS, fused_dqn_replay_feature=True, n_step=3) at the zoo configuration up to
    n_learn["window"] of tests/golden/dqn_replay_feature/learning_reference.json (15 000 environment steps): the median over the
    lanes of the mean return of the last 100 training episodes reaches that file's bar (44.157, twice the random policy's mean) --
    tests/test_gpu_dqn_replay_feature_agent.py::test_closed_loop_learns' condition on the same seeds, one batch instead of three
    runs."""
    from parity_log import record_parity
    from deeprl_amd import zoo
    ref = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))
    bar, n_learn = ref["bar"], ref["n_learn"]["window"]
    assert n_learn == 15000 and abs(bar - 44.157) < 1e-3
    DQN._quiet(monkeypatch)
    runs = zoo.run_seeds("dqn_feature", K.LEARN_SEEDS, game=GAME, tag="dqn_replay_lanes_learn", max_steps=n_learn,
                         fused_dqn_replay_feature=True, n_step=3)
    assert len(runs) == len(K.LEARN_SEEDS)
    means = []
    for seed, pairs in zip(K.LEARN_SEEDS, runs):
        assert all(0 < s <= n_learn for s, _ in pairs) and [s for s, _ in pairs] == sorted(s for s, _ in pairs)
        means.append(float(np.mean([r for _, r in pairs][-K.LAST_EPISODES:])))
        print("seed %d: %d episodes, last-%d mean %.2f" % (seed, len(pairs), K.LAST_EPISODES, means[-1]))
    median = float(np.median(means))
    record_parity("dqn_feature n-step seed lanes closed loop: last-100 mean returns per seed, median, bar", median=median, bar=bar,
                  **{"seed%d" % s: m for s, m in zip(K.LEARN_SEEDS, means)})
    assert median >= bar, (means, bar)
