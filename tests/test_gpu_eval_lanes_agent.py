"""Evaluation of seed lanes on the device (deeprl_amd/seed_batch.py: FeatureSeeds(..., eval_lanes=True), evaluate, eval_episodes;
zoo.run_seeds(..., evaluate=True)): lane k of a batch against the single agent of seed k with the entry's switch and
config.fused_eval = True, evaluated at the same points, bit for bit -- what every evaluation returns and leaves, and at the end
everything tests/test_gpu_dqn_lanes_agent.py and tests/test_gpu_dist_lanes_agent.py compare, which shows that evaluation disturbs
nothing.

The small configurations are those two files' (4 transitions per agent step, exploration_steps 14, 10 agent steps), with
eval_episodes 3 over an evaluation cart-pole of the lane's own seed and episodes of at most 12 steps.  Evaluations happen ahead of
agent step 0, after agent step 2 (8 environment steps: inside exploration_steps), and after agent steps 6 and 10 (learning began
with agent step 4)."""
import numpy as np
import pytest
import torch
from feature_kernel_harness import GAME, dra, _Rec, _bits      # noqa: F401  (dra: the fixture)

import test_gpu_dist_lanes_agent as DIST
import test_gpu_dqn_lanes_agent as DQN

pytestmark = pytest.mark.gpu

SEEDS = DQN.SEEDS
HEADS = ("dqn", "c51", "qr")
STEPS, EVAL_AFTER = DQN.A["steps"], (0, 2, 6, 10)      # evaluations behind this many agent steps
EPISODES, EVAL_HORIZON = 3, 12
assert DQN.A["steps"] == DIST.A["steps"] == 10 and DQN.A["exploration_steps"] == DIST.A["exploration_steps"] == 14
assert DQN.A["k"] == DIST.A["k"] == 4 and DQN.SEEDS == DIST.SEEDS


def _eval_env(d, stepped=()):
    """per_seed hook: the lane's evaluation environment, of the lane's own seed; for the seeds in `stepped`, stepped once on the
    host."""
    def per_seed(seed, c):
        c.eval_env = d.Task(GAME, seed=1000 + seed, synthetic_done_period=EVAL_HORIZON)
        if seed in stepped:
            c.eval_env.reset()
            c.eval_env.step([0])
    return per_seed


def _maker(d, head, single, per_seed=None, **extra):
    """make_config(seed) of `head` over the other two files' makers.  single: the entry's switches and fused_eval, as the single
    agent needs them (the batch sets its own switches, and evaluation is the batch's property)."""
    per_seed = per_seed or _eval_env(d)
    if head == "dqn":
        return DQN._maker(d, per_seed=per_seed, eval_episodes=EPISODES, **(dict(fused_eval=True) if single else {}), **extra)
    switches = dict(fused_dist_feature=True, fused_dist_update=True, fused_eval=True) if single else {}
    return DIST._maker(d, head, per_seed=per_seed, eval_episodes=EPISODES, **switches, **extra)


def _lane_state(head, agent):
    return (DQN if head == "dqn" else DIST)._lane_state(agent)


def _env_words(vec):
    state = vec.state_dict()
    return {k: np.asarray(v).copy() for k, v in state.items()}


def _test_lines(agent):
    return [ln for ln in agent.logger.lines if 'episodic_return_test' in ln]


def _single(d, head, seed):
    """The single agent of `seed` with fused_eval, stepped STEPS times and evaluated (agent.eval_episodes()) at EVAL_AFTER."""
    d.random_seed(seed)
    torch.manual_seed(seed)
    cls = d.DQNAgent if head == "dqn" else DIST._agent_cls(d, head)
    agent = cls(_maker(d, head, True)(seed))
    step = agent._feature
    assert type(step).__name__ == "Step"
    returns, report = [], agent._report_eval

    def watched(r):
        returns.append(np.asarray(r, dtype=np.float64).copy())
        return report(r)
    agent._report_eval = watched
    actions, indices, evals = [], [], []

    def evaluate():
        got = agent.eval_episodes()
        assert step._eval_vec not in (None, False)
        evals.append(dict(returns=returns[-1], lengths=step.eval_lengths.copy(), steps=int(step.eval_steps), env=_env_words(step._eval_vec),
                          total=agent.total_steps, report=got))
    for s in range(STEPS + 1):
        if s in EVAL_AFTER:
            evaluate()
        if s < STEPS:
            agent.step()
            actions.append(step.out_action.cpu().numpy().copy())
            indices.append(step.last_draws[3])
    assert (step.eval_launches, step.eval_copies) == (len(EVAL_AFTER),) * 2 and not agent.logger.warnings
    events = agent.episodes()
    out = _lane_state(head, agent)
    out.update(actions=np.asarray(actions), indices=indices, events=events, rng=np.random.randint(0, 1 << 30, size=3), evals=evals,
               test_lines=_test_lines(agent))
    agent.close()
    return out


def _seeds_cls(head):
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    return DQNFeatureSeeds if head == "dqn" else DIST._seeds_cls(head)


def _batched(d, head, seeds, device_draws=False):
    batch = _seeds_cls(head)(_maker(d, head, False), seeds, device_draws=device_draws, eval_lanes=True)
    assert all(getattr(batch.lane(k).config, "fused_eval", False) is not True for k in range(len(seeds)))
    n = len(seeds)
    actions, indices, evals = [[] for _ in seeds], [[] for _ in seeds], [[] for _ in seeds]

    def evaluate():
        rng = np.random.get_state()
        reports = batch.eval_episodes()
        after = np.random.get_state()
        assert rng[0] == after[0] and np.array_equal(rng[1], after[1]) and rng[2:] == after[2:]      # (evaluation draws nothing)
        assert batch.eval_returns.shape == (n, EPISODES) and batch.eval_returns.dtype == np.float64
        assert batch.eval_lengths.shape == (n, EPISODES) and batch.eval_steps.shape == (n,)
        for k in range(n):
            evals[k].append(dict(returns=batch.eval_returns[k].copy(), lengths=batch.eval_lengths[k].copy(), steps=int(batch.eval_steps[k]),
                                 env=_env_words(batch.eval_vecs[k]), total=batch.lane(k).total_steps, report=reports[k]))
    for s in range(STEPS + 1):
        if s in EVAL_AFTER:
            evaluate()
        if s < STEPS:
            batch.step()
            for k in range(n):
                actions[k].append(batch.lane(k)._feature.out_action.cpu().numpy().copy())
                indices[k].append(batch.fetch_draws(k)[3])
    counts = (batch.eval_launches, batch.eval_copies)
    lanes = []
    for k in range(n):
        events = batch.episodes(k)
        out = _lane_state(head, batch.lane(k))
        out.update(actions=np.asarray(actions[k]), indices=indices[k], events=events, rng=batch.rng_tail(k).randint(0, 1 << 30, size=3),
                   evals=evals[k], test_lines=_test_lines(batch.lane(k)), single_launches=batch.lane(k)._feature.eval_launches)
        lanes.append(out)
    with pytest.raises(RuntimeError, match="call the batch's eval_episodes"):
        batch.lane(0).eval_episodes()
    with pytest.raises(RuntimeError, match="call the batch's eval_episodes"):
        batch.lane(n - 1).eval_episode()
    graphed = {k: r.graph is not None for k, r in batch.regions.items()}
    batch.close()
    return dict(lanes=lanes, counts=counts, graphed=graphed)


def _assert_evals_equal(got, want, what):
    assert len(got) == len(want) == len(EVAL_AFTER)
    for i, (g, w) in enumerate(zip(got, want)):
        at = (what, "evaluation %d" % i)
        assert g["total"] == w["total"] == EVAL_AFTER[i] * DQN.A["k"], at
        assert g["returns"].dtype == w["returns"].dtype == np.float64 and np.array_equal(_bits(g["returns"]), _bits(w["returns"])), at
        assert g["lengths"].dtype == w["lengths"].dtype and np.array_equal(g["lengths"], w["lengths"]), at
        assert g["steps"] == w["steps"] == int(w["lengths"].sum()) and EPISODES <= g["steps"] <= EPISODES * EVAL_HORIZON, at
        assert set(g["env"]) == set(w["env"]), at
        for k in w["env"]:
            assert g["env"][k].dtype == w["env"][k].dtype and np.array_equal(_bits(g["env"][k]), _bits(w["env"][k])), at + (k,)
        assert g["report"] == w["report"], at


@pytest.fixture(scope="module")
def singles(dra):
    """The single runs with fused_eval, per head and seed: computed once on first use, left unchanged."""
    cache = {}

    def get(head, seed):
        if (head, seed) not in cache:
            mp = pytest.MonkeyPatch()
            try:
                DQN._quiet(mp)
                cache[head, seed] = _single(dra, head, seed)
            finally:
                mp.undo()
        return cache[head, seed]
    return get


def _check(head, got, singles, seeds):
    assert_lane = (DQN if head == "dqn" else DIST)._assert_lane_is
    assert got["counts"] == (len(EVAL_AFTER), len(EVAL_AFTER))       # one launch and one copy per evaluation, whatever the lane count
    assert got["graphed"] == dict(act=True, learn=True)
    for k, seed in enumerate(seeds):
        want, lane = singles(head, seed), got["lanes"][k]
        _assert_evals_equal(lane["evals"], want["evals"], "%s seed %d" % (head, seed))
        assert lane["test_lines"] == want["test_lines"] and len(want["test_lines"]) == len(EVAL_AFTER)
        assert lane["single_launches"] == 0                           # (no lane went through the single launch)
        assert_lane(lane, want, "%s seed %d" % (head, seed))
        assert want["opt_steps"] > 0 and len(want["events"]) >= 8     # (learning steps ran, training episodes ended)


@pytest.mark.parametrize("head", HEADS)
def test_lanes_evaluate_as_the_single_agents(dra, monkeypatch, singles, head):
    """Three seeds as lanes with eval_lanes=True against the three single fused_eval agents: at each of the four evaluations the
    returns, eval_lengths, eval_steps, the evaluation environment's state_dict(), the reported dict and the logged
    'episodic_return_test' lines; at the end the parameters, target, optimiser state, ring, episodes, actions, indices and
    rng_tail, all to the bit.  eval_launches == eval_copies == 4 for the three lanes; evaluation leaves np.random where it was;
    a lane agent's own eval_episodes() / eval_episode() raise and point to the batch's."""
    DQN._quiet(monkeypatch)
    got = _batched(dra, head, SEEDS)
    _check(head, got, singles, SEEDS)
    a, b = (singles(head, s)["evals"] for s in SEEDS[:2])
    assert any(not np.array_equal(x["env"]["env_state"], y["env"]["env_state"]) for x, y in zip(a, b))      # (the lanes differ)


def test_one_lane_evaluates_as_the_single_agent(dra, monkeypatch, singles):
    """A batch of one: the same counts -- one launch and one copy per evaluation."""
    DQN._quiet(monkeypatch)
    _check("dqn", _batched(dra, "dqn", (11,)), singles, (11,))


def test_lanes_evaluate_with_device_draws(dra, monkeypatch, singles):
    """The same once more with device_draws=True for dqn_feature: evaluation touches no generator state, on the host or on the
    device, so the lanes still end where the single runs end."""
    DQN._quiet(monkeypatch)
    _check("dqn", _batched(dra, "dqn", SEEDS, device_draws=True), singles, SEEDS)


def test_refusals(dra, monkeypatch):
    """A lane whose eval_env has been stepped on the host is refused by name (lanes have no host evaluation); a lane whose config
    sets fused_eval itself keeps today's message, with eval_lanes or without; lanes that differ in eval_episodes are named by
    first_mismatch; evaluate() on a batch without eval_lanes raises."""
    from deeprl_amd.dqn_mlp import DraError
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    d = dra
    DQN._quiet(monkeypatch)
    with pytest.raises(ValueError, match="seed 11 cannot run as a lane: fused evaluation: the evaluation environment has already been "
                                         "stepped on the host"):
        DQNFeatureSeeds(_maker(d, "dqn", False, per_seed=_eval_env(d, stepped=(11,))), SEEDS, eval_lanes=True)

    def fused_eval(seed, c):
        _eval_env(d)(seed, c)
        if seed == 3:
            c.fused_eval = True
    for eval_lanes in (True, False):
        with pytest.raises(ValueError, match="seed 3 cannot run as a lane: config.fused_eval is on: the evaluation launch has no lane form"):
            DQNFeatureSeeds(_maker(d, "dqn", False, per_seed=fused_eval), SEEDS, eval_lanes=eval_lanes)

    def more_episodes(seed, c):
        _eval_env(d)(seed, c)
        if seed == 12:
            c.eval_episodes = 4
    with pytest.raises(ValueError, match=r"lane 2 differs from lane 0 in eval_episodes \(4, lane 0: 3\)"):
        DQNFeatureSeeds(_maker(d, "dqn", False, per_seed=more_episodes), SEEDS, eval_lanes=True)
    DQNFeatureSeeds(_maker(d, "dqn", False, per_seed=more_episodes), SEEDS).close()      # (without eval_lanes it is no mismatch)
    plain = DQNFeatureSeeds(_maker(d, "dqn", False), SEEDS[:2])
    with pytest.raises(DraError, match="needs a batch built with eval_lanes=True"):
        plain.evaluate(1)
    plain.close()


def test_evaluate_takes_other_episode_counts(dra, monkeypatch):
    """evaluate(n) with n other than config.eval_episodes (one block per episode count): shapes, and each lane's lengths add up to
    its steps; the next evaluate() goes on from the environment's counter."""
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    DQN._quiet(monkeypatch)
    batch = DQNFeatureSeeds(_maker(dra, "dqn", False), SEEDS, eval_lanes=True)
    counter = 0
    for n in (1, 4, 4):
        r = batch.evaluate(n)
        assert r.shape == (3, n) and batch.eval_lengths.shape == (3, n) and np.array_equal(batch.eval_lengths.sum(axis=1), batch.eval_steps)
        assert np.array_equal(r, batch.eval_lengths.astype(np.float64))      # (the cart-pole pays 1 per step)
        counter += int(batch.eval_steps[0])
        assert int(batch.eval_vecs[0].env_counter.item()) == counter
    assert (batch.eval_launches, batch.eval_copies) == (3, 3)
    batch.close()


RUN = dict(max_steps=24, overrides=dict(eval_interval=8, eval_episodes=EPISODES, exploration_steps=12, save_interval=0, log_interval=10 ** 9))


def test_run_seeds_evaluates_as_run_steps(dra, monkeypatch):
    """zoo.run_seeds("dqn_feature", seeds, evaluate=True, ...) against support.run_steps over the single fused_eval agent of each
    seed (its (step, returns) gathered by wrapping _report_eval): per seed the same list, at zoo.eval_points' steps; the training
    episodes are the single run's; with evaluate=False the return value is the plain list, as before."""
    from deeprl_amd import zoo
    from deeprl_amd.support import run_steps
    DQN._quiet(monkeypatch)
    d = dra
    episodes, evaluations = zoo.run_seeds("dqn_feature", SEEDS, evaluate=True, game=GAME, tag="eval_lanes_run", **RUN)
    points = zoo.eval_points(RUN["max_steps"], RUN["overrides"]["eval_interval"], 4)
    assert points == [0, 8, 16, 24] and len(episodes) == len(evaluations) == len(SEEDS)
    for k, seed in enumerate(SEEDS):
        d.random_seed(seed)
        torch.manual_seed(seed)
        c = zoo.config("dqn_feature", fused_dqn_feature=True, game=GAME, tag="eval_lanes_run", max_steps=RUN["max_steps"],
                       overrides=dict(RUN["overrides"], fused_eval=True))
        c.task_fn = lambda: d.Task(c.game, seed=seed)
        agent = d.DQNAgent(c)
        assert c.sgd_update_frequency == 4
        want, report = [], agent._report_eval

        def watched(r, agent=agent, want=want, report=report):
            want.append((agent.total_steps, np.asarray(r, dtype=np.float64).copy()))
            return report(r)
        agent._report_eval = watched
        step = agent._feature
        run_steps(agent)
        assert step.eval_launches == len(points) and not agent.logger.warnings
        got = evaluations[k]
        assert [s for s, _ in got] == [s for s, _ in want] == points
        for (_, g), (_, w) in zip(got, want):
            assert g.dtype == np.float64 and g.shape == (EPISODES,) and np.array_equal(_bits(g), _bits(w)), (seed, g, w)
        assert episodes[k] == list(step.episodes.log)      # (run_steps closed the agent: everything is drained, nothing was read out)
    plain = zoo.run_seeds("dqn_feature", SEEDS, game=GAME, tag="eval_lanes_run", **RUN)
    assert isinstance(plain, list) and len(plain) == len(SEEDS) and plain == episodes

