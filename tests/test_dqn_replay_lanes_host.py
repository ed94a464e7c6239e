"""The host side of dqn_feature's window lanes (deeprl_amd/seed_batch.py: DQNReplayFeatureSeeds), without a GPU: the table
zoo.run_seeds picks the class from and the keyword that makes it, the switch a batch sets on a lane's Config, what the lanes'
signature holds on top of dqn_feature's and how a mismatch is named, the names FeatureSeeds reads from the class's MODULE, the
arguments of the class's *_supported entry, the refusals that need no lane."""
import types

import pytest
import torch


def _fake_agent(n_step=3, replay_discount=0.99, hidden=16, **over):
    from deeprl_amd import nets
    from deeprl_amd.support import Config, LinearSchedule
    c = Config()
    c.sgd_update_frequency, c.exploration_steps, c.target_network_update_freq = 4, 6, 3
    c.gradient_clip, c.discount, c.double_q, c.n_step = 5, 0.99, False, n_step
    c.random_action_prob = LinearSchedule(0.8, 0.1, 30)
    for k, v in over.items():
        setattr(c, k, v)
    net = nets.VanillaNet(2, nets.FCBody(4, (hidden, hidden)))
    rp = types.SimpleNamespace(batch_size=10, memory_size=24, n_step=n_step, discount=replay_discount)
    return types.SimpleNamespace(config=c, network=net, optimizer=torch.optim.RMSprop(net.parameters(), 0.001), _inner_replay=lambda: rp)


def test_the_class_is_registered_beside_the_one_step_table():
    from deeprl_amd import dqn_mlp, dqn_replay_mlp, seed_batch
    cls = seed_batch.DQNReplayFeatureSeeds
    assert seed_batch.REPLAY_SEED_CLASSES == {"dqn_feature": cls}
    assert set(seed_batch.SEED_CLASSES) == {"dqn_feature", "categorical_dqn_feature", "quantile_regression_dqn_feature"}
    assert seed_batch.SEED_CLASSES["dqn_feature"] is seed_batch.DQNFeatureSeeds and seed_batch.DQNFeatureSeeds.MODULE is dqn_mlp
    assert issubclass(cls, seed_batch.FeatureSeeds) and not issubclass(cls, seed_batch.DQNFeatureSeeds)
    assert cls.ENTRY == "dqn_feature" and cls.WINDOW is True and seed_batch.DQNFeatureSeeds.WINDOW is False
    # acting and evaluation are dqn_mlp's own lane entries; the update and the shape table are the window's
    assert (cls.ACT_LANES, cls.EVAL_LANES) == (seed_batch.DQNFeatureSeeds.ACT_LANES, seed_batch.DQNFeatureSeeds.EVAL_LANES)
    assert (cls.UPDATE_LANES, cls.LANES_SUPPORTED) == ("dra_dqn_replay_mlp_update_lanes", "dra_dqn_replay_mlp_lanes_supported")
    m = cls.MODULE
    assert m.Step is dqn_replay_mlp.Step and m.UpdateIO is dqn_replay_mlp.UpdateIO and m.Kind is dqn_replay_mlp.WindowKind
    assert m.Net is dqn_mlp.Net and m.ActIO is dqn_mlp.ActIO and m.why_not is dqn_replay_mlp.why_not
    assert cls.agent_class(cls.__new__(cls)).__name__ == "DQNAgent"


def test_switch_on_sets_the_replay_switch_alone():
    from deeprl_amd.seed_batch import DQNReplayFeatureSeeds
    from deeprl_amd.support import Config
    c = Config()
    DQNReplayFeatureSeeds.switch_on(DQNReplayFeatureSeeds.__new__(DQNReplayFeatureSeeds), c)
    assert c.fused_dqn_replay_feature is True
    assert getattr(c, "fused_dqn_feature", False) is not True and getattr(c, "fused_dqn_replay_update", None) is None


def test_signature_names_the_window_and_the_folds_discount():
    from deeprl_amd.seed_batch import DQNReplayFeatureSeeds, first_mismatch, lane_signature, replay_lane_signature
    sig = replay_lane_signature(_fake_agent())
    assert sig["n_step"] == 3 and sig["replay_discount"] == 0.99 and sig["shape"] == (4, 2, 16, 1)
    assert list(sig)[-2:] == ["n_step", "replay_discount"]      # (behind the common fields: first_mismatch names those first)
    assert set(sig) - {"n_step", "replay_discount"} == set(lane_signature(_fake_agent()))
    batch = DQNReplayFeatureSeeds.__new__(DQNReplayFeatureSeeds)
    assert batch.signature(_fake_agent()) == sig
    same = [replay_lane_signature(_fake_agent()) for _ in range(3)]
    assert first_mismatch(same) is None
    for field, kw, text in (("n_step", dict(n_step=8), "(8, lane 0: 3)"), ("replay_discount", dict(replay_discount=0.9), "(0.9, lane 0: 0.99)"),
                            ("double_q", dict(double_q=True), "(True, lane 0: False)"), ("shape", dict(hidden=32), "")):
        why = first_mismatch(same[:2] + [replay_lane_signature(_fake_agent(**kw))])
        assert why.startswith("lane 2 differs from lane 0 in %s " % field) and why.endswith(text), why


def test_supported_arguments_carry_the_window():
    """(state_dim, n_actions, hidden, t_len, batch, gate, n_step, n_lanes) for the window's table, the 1-step classes' as before."""
    from deeprl_amd.seed_batch import DQNFeatureSeeds, DQNReplayFeatureSeeds
    new, old = DQNReplayFeatureSeeds.__new__(DQNReplayFeatureSeeds), DQNFeatureSeeds.__new__(DQNFeatureSeeds)
    for b in (new, old):
        b.k, b.batch, b.n_step = 4, 10, 3
    assert new.lanes_supported_args((4, 2, 16, 1), 5) == (4, 2, 16, 4, 10, 1, 3, 5)
    assert old.lanes_supported_args((4, 2, 16, 1), 5) == (4, 2, 16, 4, 10, 1, 5)


class _Picked(Exception):
    pass


def _recording(base, seen):
    class Recording(base):
        def __init__(self, make_config, seeds, device_draws=False, eval_lanes=False):
            seen.append((base.__name__, tuple(seeds), device_draws, eval_lanes, make_config(seeds[0])))
            raise _Picked()
    return Recording


def test_run_seeds_picks_the_class_only_with_the_keyword(monkeypatch):
    from deeprl_amd import seed_batch, zoo
    seen = []
    monkeypatch.setitem(seed_batch.SEED_CLASSES, "dqn_feature", _recording(seed_batch.DQNFeatureSeeds, seen))
    monkeypatch.setitem(seed_batch.REPLAY_SEED_CLASSES, "dqn_feature", _recording(seed_batch.DQNReplayFeatureSeeds, seen))
    for kw, want in ((dict(n_step=3), "DQNFeatureSeeds"), (dict(n_step=3, fused_dqn_replay_feature=False), "DQNFeatureSeeds"),
                     (dict(n_step=3, fused_dqn_replay_feature=1), "DQNFeatureSeeds"),
                     (dict(n_step=3, fused_dqn_replay_feature=True), "DQNReplayFeatureSeeds"),
                     (dict(fused_dqn_replay_feature=True), "DQNReplayFeatureSeeds")):
        with pytest.raises(_Picked):
            zoo.run_seeds("dqn_feature", (3, 11), device_draws=True, game="CartPole-v0", tag="picked", max_steps=40, **kw)
        name, seeds, device_draws, eval_lanes, cfg = seen.pop()
        assert (name, seeds, device_draws, eval_lanes) == (want, (3, 11), True, False) and not seen
        # n_step and the keyword travel to config() as they do for a single agent; run_seeds sets the class's own switch
        assert cfg.n_step == kw.get("n_step", 1) and cfg.replay_kwargs["n_step"] == cfg.n_step and cfg.max_steps == 40
        if want == "DQNReplayFeatureSeeds":
            assert cfg.fused_dqn_replay_feature is True and getattr(cfg, "fused_dqn_feature", False) is not True
        else:
            assert cfg.fused_dqn_feature is True and getattr(cfg, "fused_dqn_replay_feature", False) is not True
    for name in ("categorical_dqn_feature", "quantile_regression_dqn_feature"):
        with pytest.raises(ValueError, match="fused_dqn_replay_feature is dqn_feature's switch, %s has no lane form under it" % name):
            zoo.run_seeds(name, (1, 2), fused_dqn_replay_feature=True)
    with pytest.raises(ValueError, match="rainbow_feature has no lane form"):
        zoo.run_seeds("rainbow_feature", (1, 2), fused_dqn_replay_feature=True)


def test_more_than_64_seeds_are_refused_before_anything_is_built():
    from deeprl_amd import seed_batch

    def make_config(seed):
        raise AssertionError("no lane may be built")
    for seeds in (range(65), ()):
        with pytest.raises(ValueError, match="DQNReplayFeatureSeeds runs 1 to 64 seeds as lanes, not %d" % len(seeds)):
            seed_batch.DQNReplayFeatureSeeds(make_config, seeds)
