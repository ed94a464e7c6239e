"""The host side of the distributional seed lanes (deeprl_amd/seed_batch.py), without a GPU: what the lanes' signature holds on top
of dqn_feature's and how a mismatch is named, the classes zoo.run_seeds picks, the switches a batch sets on a lane's Config, the
refusals that need no lane."""
import types

import pytest
import torch


def _fake_agent(head="c51", n=20, hidden=16, support=(-10.0, 10.0), **over):
    from deeprl_amd import nets
    from deeprl_amd.support import Config, LinearSchedule
    c = Config()
    c.sgd_update_frequency, c.exploration_steps, c.target_network_update_freq = 4, 6, 3
    c.gradient_clip, c.discount, c.double_q = 5, 0.99, False
    c.categorical_v_min, c.categorical_v_max = support
    c.random_action_prob = LinearSchedule(0.8, 0.1, 30)
    for k, v in over.items():
        setattr(c, k, v)
    net = (nets.CategoricalNet if head == "c51" else nets.QuantileNet)(2, n, nets.FCBody(4, (hidden, hidden)))
    rp = types.SimpleNamespace(batch_size=10, memory_size=24)
    return types.SimpleNamespace(config=c, network=net, optimizer=torch.optim.RMSprop(net.parameters(), 0.001), _inner_replay=lambda: rp)


def test_signature_holds_head_atoms_and_support():
    from deeprl_amd import dist_mlp
    from deeprl_amd.seed_batch import dist_lane_signature, lane_signature
    sig = dist_lane_signature(_fake_agent())
    assert sig["shape"] == (4, 2, 16, 1) and sig["head"] == dist_mlp.CATEGORICAL and sig["n_atoms"] == 20 and sig["support"] == (-10.0, 10.0)
    assert list(sig)[-3:] == ["head", "n_atoms", "support"]      # (behind the common fields: first_mismatch names those first)
    common = dict(sig)
    for k in ("shape", "head", "n_atoms", "support"):
        common.pop(k)
    assert set(common) == set(lane_signature(_fake_agent(), shape=(4, 2, 16, 1))) - {"shape"}
    qr = dist_lane_signature(_fake_agent("qr"))
    assert qr["head"] == dist_mlp.QUANTILE and qr["support"] == (0.0, 0.0)


@pytest.mark.parametrize("field, kw", [("n_atoms", dict(n=21)), ("head", dict(head="qr")), ("support", dict(support=(-10.0, 20.0))),
                                       ("shape", dict(hidden=32)), ("double_q", dict(double_q=True)), ("discount", dict(discount=0.9))])
def test_mismatch_detector_names_the_field(field, kw):
    from deeprl_amd.seed_batch import dist_lane_signature, first_mismatch
    same = [dist_lane_signature(_fake_agent()) for _ in range(3)]
    assert first_mismatch(same) is None
    why = first_mismatch(same[:2] + [dist_lane_signature(_fake_agent(**kw))])
    assert why.startswith("lane 2 differs from lane 0 in %s " % field), why


def test_run_seeds_picks_the_class_per_entry():
    from deeprl_amd import dist_mlp, dqn_mlp, seed_batch, zoo
    assert set(seed_batch.SEED_CLASSES) == {"dqn_feature", "categorical_dqn_feature", "quantile_regression_dqn_feature"}
    c51, qr = seed_batch.SEED_CLASSES["categorical_dqn_feature"], seed_batch.SEED_CLASSES["quantile_regression_dqn_feature"]
    assert (c51.AGENT, qr.AGENT) == ("CategoricalDQNAgent", "QuantileRegressionDQNAgent")
    assert c51.MODULE is dist_mlp and qr.MODULE is dist_mlp and seed_batch.SEED_CLASSES["dqn_feature"].MODULE is dqn_mlp
    assert issubclass(c51, seed_batch.FeatureSeeds) and issubclass(seed_batch.DQNFeatureSeeds, seed_batch.FeatureSeeds)
    assert all(zoo.ZOO[name]["agent"] == getattr(cls, "AGENT", "DQNAgent") for name, cls in seed_batch.SEED_CLASSES.items())
    for name in ("rainbow_feature", "categorical_dqn_pixel", "n_step_dqn_feature"):
        with pytest.raises(ValueError, match="%s has no lane form" % name):
            zoo.run_seeds(name, (1, 2))


@pytest.mark.parametrize("given, want", [(None, True), (True, True), (False, False)])
def test_switches_a_batch_sets(given, want):
    """config.fused_dist_feature is set; config.fused_dist_update becomes True only where it is unset (an explicit False stays, and
    the lane is then refused by name on the device)."""
    from deeprl_amd.seed_batch import CategoricalDQNFeatureSeeds
    from deeprl_amd.support import Config
    c = Config()
    if given is not None:
        c.fused_dist_update = given
    CategoricalDQNFeatureSeeds.switch_on(CategoricalDQNFeatureSeeds.__new__(CategoricalDQNFeatureSeeds), c)
    assert c.fused_dist_feature is True and c.fused_dist_update is want


@pytest.mark.parametrize("name", ["CategoricalDQNFeatureSeeds", "QuantileRegressionDQNFeatureSeeds"])
def test_more_than_64_seeds_are_refused_before_anything_is_built(name):
    from deeprl_amd import seed_batch

    def make_config(seed):
        raise AssertionError("no lane may be built")
    for seeds in (range(65), ()):
        with pytest.raises(ValueError, match="%s runs 1 to 64 seeds as lanes, not %d" % (name, len(seeds))):
            getattr(seed_batch, name)(make_config, seeds)
