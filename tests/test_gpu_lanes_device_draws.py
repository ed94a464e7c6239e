"""The seed lanes with device_draws=True (deeprl_amd/seed_batch.py, csrc/np_mt.hip: every lane's np.random stream drawn by a kernel
in front of the act and update lane launches) against the single agents of the same seeds, bit for bit, for the three heads:
dqn_feature ("dqn"), categorical_dqn_feature ("c51") and quantile_regression_dqn_feature ("qr").

The small configurations, the single runs and the full comparison are the existing lane tests' (test_gpu_dqn_lanes_agent.py,
test_gpu_dist_lanes_agent.py: capacity 24, batch 10, k 4, seeds (3, 11, 12)); the batch is built here with the flag on and read
through fetch_draws, since last_draws is None in this mode.  40 agent steps: about a thousand words per lane, so every lane's key
is regenerated on the device at least once."""
import numpy as np
import pytest
import torch
from feature_kernel_harness import GAME, dra      # noqa: F401  (dra: the fixture)

import test_gpu_dist_lanes_agent as D
import test_gpu_dqn_lanes_agent as Q

pytestmark = pytest.mark.gpu

HEADS = ("dqn", "c51", "qr")
SEEDS = (3, 11, 12)
STEPS, MID = 40, 17
EXPLORATION_STEPS, K = Q.A["exploration_steps"], Q.A["k"]
assert D.A["exploration_steps"] == EXPLORATION_STEPS and D.A["k"] == K and D.A["capacity"] == Q.A["capacity"] == 24


def _cls(head):
    from deeprl_amd import seed_batch
    return seed_batch.DQNFeatureSeeds if head == "dqn" else D._seeds_cls(head)


def _maker(d, head, **kw):
    return Q._maker(d, **kw) if head == "dqn" else D._maker(d, head, **kw)


def _single(d, head, seed, steps):
    return Q._single(d, seed, steps) if head == "dqn" else D._single(d, head, seed, steps)


def _lane_state(head, agent):
    return (Q if head == "dqn" else D)._lane_state(agent)


def _assert_lane_is(head, got, want, what):
    (Q if head == "dqn" else D)._assert_lane_is(got, want, what)


def _tail(rs):
    return rs.randint(0, 1 << 30, size=3)


def _batched(d, head, seeds, steps=STEPS, mid=None, **kw):
    """The batch with device_draws=True, stepped `steps` times: per lane what _lane_state and the single run's record hold, the
    indices through fetch_draws; `mid`: rng_tail(k) is also read (and drawn from) after that many steps."""
    batch = _cls(head)(_maker(d, head, **kw), seeds, device_draws=True)
    uploaded = batch._uploaded.copy()
    built = np.random.get_state()
    actions, indices, mid_tails = [[] for _ in seeds], [[] for _ in seeds], None
    for s in range(steps):
        batch.step()
        learned = batch.total_steps > EXPLORATION_STEPS
        for k in range(len(seeds)):
            assert batch.lane(k)._feature.last_draws is None
            explore, rand, slot0, idx = batch.fetch_draws(k, learned)
            assert explore.dtype == np.bool_ and explore.shape == rand.shape == (K,) and slot0 == (s * K) % Q.A["capacity"]
            actions[k].append(batch.lane(k)._feature.out_action.cpu().numpy().copy())
            indices[k].append(idx)
        if mid == s + 1:
            mid_tails = [_tail(batch.rng_tail(k)) for k in range(len(seeds))]
    assert batch.total_steps == steps * K
    after = np.random.get_state()
    assert built[0] == after[0] and np.array_equal(built[1], after[1]) and built[2:] == after[2:]      # the global stream stayed put
    regenerated = [not np.array_equal(batch.mt_words(k)[:624], uploaded[k][:624]) for k in range(len(seeds))]
    lanes = []
    for k in range(len(seeds)):
        events = batch.episodes(k)
        out = _lane_state(head, batch.lane(k))
        out.update(actions=np.asarray(actions[k]), indices=indices[k], events=events, rng=_tail(batch.rng_tail(k)))
        lanes.append(out)
    graphed = {k: r.graph is not None for k, r in batch.regions.items()}
    launches = batch.launches
    batch.close()
    return dict(lanes=lanes, graphed=graphed, launches=launches, regenerated=regenerated, mid_tails=mid_tails)


_SINGLES, _LANES = {}, {}


@pytest.fixture
def singles(dra, request):
    """The three single runs of a head, one after another: shared by the tests below, left unchanged."""
    head = request.node.callspec.params["head"]
    return D._shared(_SINGLES, head, lambda: {s: _single(dra, head, s, STEPS) for s in SEEDS})


@pytest.fixture
def lanes(dra, request):
    """The device-draw batch of a head over the same seeds with graph replay, rng_tail read mid-run as well."""
    head = request.node.callspec.params["head"]
    return D._shared(_LANES, head, lambda: _batched(dra, head, SEEDS, mid=MID))


@pytest.mark.parametrize("head", HEADS)
def test_device_draw_lanes_equal_the_single_agents(dra, head, singles, lanes):
    """40 agent steps (3 acting, 37 learning; both regions captured and replayed, target copies between replays) with the draws
    taken on the device: per lane everything _assert_lane_is compares -- parameters, target, optimiser state, ring, indices (read
    back through fetch_draws), actions, counters, the schedule's position, episodes and log lines, and three randint draws of
    rng_tail(k) against the single run's np.random tail.  Every lane's key was regenerated on the device, and the global np.random
    state did not move (_batched)."""
    # per region: the draw launch and the acting launch count (2 eager steps + the capture)
    assert lanes["graphed"] == dict(act=True, learn=True) and lanes["launches"] == 2 * (3 + 3)
    for k, seed in enumerate(SEEDS):
        _assert_lane_is(head, lanes["lanes"][k], singles[seed], "%s seed %d" % (head, seed))
    assert any(lanes["regenerated"]), "no lane's key was regenerated: the run says nothing about the twist"
    assert all(lanes["regenerated"])


@pytest.mark.parametrize("head", HEADS)
def test_device_draw_lanes_graph_replay_equals_eager(dra, monkeypatch, head, lanes):
    Q._quiet(monkeypatch)
    eager = _batched(dra, head, SEEDS, graph=False)
    assert eager["graphed"] == dict(act=False, learn=False) and eager["launches"] == 2 * STEPS
    for k, seed in enumerate(SEEDS):
        _assert_lane_is(head, eager["lanes"][k], lanes["lanes"][k], "eager %s seed %d" % (head, seed))


@pytest.mark.parametrize("head", HEADS)
def test_one_device_draw_lane_equals_the_single_agent(dra, monkeypatch, head, singles):
    Q._quiet(monkeypatch)
    one = _batched(dra, head, (11,))
    assert one["graphed"] == dict(act=True, learn=True)
    _assert_lane_is(head, one["lanes"][0], singles[11], "a batch of one")


@pytest.mark.parametrize("head", ("dqn",))
def test_rng_tail_mid_run_and_at_the_end(dra, monkeypatch, head, singles, lanes):
    """rng_tail(k) read -- and drawn from -- after 17 steps gives the tail of the single run stopped there, and the lanes go on
    from the device's state: the tails at the end (the fixture's run is the one that was read mid-run) are the 40-step single
    runs'."""
    Q._quiet(monkeypatch)
    for k, seed in enumerate(SEEDS):
        assert np.array_equal(lanes["mid_tails"][k], _single(dra, head, seed, MID)["rng"]), seed
        assert np.array_equal(lanes["lanes"][k]["rng"], singles[seed]["rng"]), seed
        assert not np.array_equal(lanes["mid_tails"][k], lanes["lanes"][k]["rng"])


def test_fetch_draws_is_the_host_lanes_last_draws(dra, monkeypatch):
    """The whole tuple -- explore flags, random actions, first slot, indices -- of every lane and step against a host-draw batch of
    the same seeds stepped beside it."""
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    Q._quiet(monkeypatch)
    host = DQNFeatureSeeds(Q._maker(dra), SEEDS)
    device = DQNFeatureSeeds(Q._maker(dra), SEEDS, device_draws=True)
    try:
        for s in range(12):
            host.step()
            device.step()
            for k in range(len(SEEDS)):
                want = host.lane(k)._feature.last_draws
                got = device.fetch_draws(k)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (s, k)
                assert (got[3] is None and want[3] is None) or np.array_equal(got[3], want[3]), (s, k)
                assert host.fetch_draws(k) is want
        device.check()
    finally:
        host.close()
        device.close()


def test_device_draw_refusals_name_their_reason(dra, monkeypatch):
    from deeprl_amd import zoo
    from deeprl_amd._lib import lib
    from deeprl_amd.replay import PrioritizedReplay
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    d = dra
    Q._quiet(monkeypatch)

    cases =((dict(n_step=3), SEEDS, "seed 3 cannot run as a lane: n_step is not 1"),
             (dict(replay_cls=PrioritizedReplay), SEEDS, "seed 3 cannot run as a lane: the replay is a PrioritizedReplay"),
             (dict(), range(65), "runs 1 to 64 seeds as lanes, not 65"))
    for kw, seeds, why in cases:
        with pytest.raises(ValueError, match=why):
            DQNFeatureSeeds(Q._maker(d, **kw), seeds, device_draws=True)
    lib.dra_np_mt_lanes_supported      # (the cached entry, whose answer the next construction is made to see as a refusal)
    with monkeypatch.context() as m:
        m.setattr(lib.dra_np_mt_lanes_supported, "raw", lambda *a: -22)
        with pytest.raises(ValueError, match="device_draws: dra_np_mt_draw_lanes is not built for 3 lanes of k 4, batch 10, 2 actions"):
            DQNFeatureSeeds(Q._maker(d), SEEDS, device_draws=True)
    with pytest.raises(ValueError, match="n_step is not 1"):
        zoo.run_seeds("dqn_feature", SEEDS, device_draws=True, game=GAME, tag="lanes_refused", n_step=3)


def test_a_cached_gaussian_is_refused(dra, monkeypatch):
    """A lane whose np.random state holds a cached Gaussian when the lane takes it over cannot be carried to the device."""
    from deeprl_amd import seed_batch
    Q._quiet(monkeypatch)
    real = seed_batch.np_mt_words
    seen = []

    def with_gauss(rs):
        if len(seen) == 1:
            rs.standard_normal()
        seen.append(rs)
        return real(rs)
    monkeypatch.setattr(seed_batch, "np_mt_words", with_gauss)
    with pytest.raises(ValueError, match="device_draws: the lane's np.random state holds a cached Gaussian"):
        seed_batch.DQNFeatureSeeds(Q._maker(dra), SEEDS, device_draws=True)
    assert len(seen) == 2


def test_run_seeds_with_device_draws_returns_the_same_episodes(dra, monkeypatch):
    from deeprl_amd import zoo
    Q._quiet(monkeypatch)
    host = zoo.run_seeds("dqn_feature", SEEDS, game=GAME, tag="lanes_host_draws", max_steps=1500)
    device = zoo.run_seeds("dqn_feature", SEEDS, device_draws=True, game=GAME, tag="lanes_device_draws", max_steps=1500)
    assert host == device and len(host) == len(SEEDS) and all(len(pairs) >= 10 for pairs in host)
