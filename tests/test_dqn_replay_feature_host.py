"""dqn_feature with an n-step window and / or a PrioritizedReplay on the device path, the part that needs no GPU
(deeprl_amd/dqn_replay_mlp.py, dra_dqn_replay_mlp_update's host checks): the ctypes mirror against the header, the supported-shape
table, the refusal of bad arguments before any launch, the eligibility list for both kinds, what the Step overrides, the restatement
(tests/dqn_replay_feature_restatement.py) against the reference's own recorded steps and replay, and what the case tables cover."""
import ctypes
import inspect
import json
import os
import shutil

import numpy as np
import pytest
import torch

import dqn_replay_feature_cases as K
import dqn_replay_feature_restatement as R
from test_dqn_feature_host import _stub

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dqn_replay_feature")


# ------------------------------------------------------------------------------------------ C ABI mirror, shapes, arguments
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirror_matches_the_header(tmp_path):
    from deeprl_amd import dqn_replay_mlp
    from test_struct_layouts import _c_layout
    mirror = dqn_replay_mlp.UpdateIO
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, "dra_dqn_replay_mlp_update_io", names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_io_is_the_one_step_io_plus_the_window_and_the_priorities():
    from deeprl_amd import dqn_mlp, dqn_replay_mlp
    old, new = [f[0] for f in dqn_mlp.UpdateIO._fields_], [f[0] for f in dqn_replay_mlp.UpdateIO._fields_]
    assert set(new) - set(old) == {"prob", "beta", "out_prio", "out_weights", "step_discount", "replay_eps", "replay_alpha", "n_step",
                                   "reserved"} and set(old) <= set(new)
    assert dict(dqn_replay_mlp.UpdateIO._fields_)["step_discount"] is ctypes.c_double


def test_supported_shapes():
    from deeprl_amd import dqn_replay_mlp
    up = dqn_replay_mlp.update_supported
    for h in (8, 16, 32, 48, 64, 128):
        for gate in (0, 1, 2, 3):
            for b in (0, 1, 10, 64, 65, 256, 257):
                for n in (0, 1, 3, 8, 9):
                    assert up(4, 2, h, b, gate, n) == (h in (16, 32, 64) and gate in (1, 2) and 1 <= b <= K.MAX_B and 1 <= n <= K.MAX_N_STEP)
    assert not up(3, 2, 64, 10, 1, 3) and not up(4, 1, 64, 10, 1, 3)
    assert dqn_replay_mlp.MAX_B == K.MAX_B and dqn_replay_mlp.MAX_N_STEP == K.MAX_N_STEP


def test_kernel_refuses_bad_arguments_before_any_launch():
    """dra_dqn_replay_mlp_update validates on the host: a NULL the mode needs, a ring that cannot hold the window, n_step outside
    1..8, a batch outside 1..256 and a negative offset are DRA_EINVAL without a device."""
    from deeprl_amd import dqn_mlp, dqn_replay_mlp
    from deeprl_amd._lib import lib
    net, uo = dqn_mlp.Net(), dqn_replay_mlp.UpdateIO()
    call = lambda: lib.dra_dqn_replay_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None)
    assert call() == -22 and lib.dra_dqn_replay_mlp_update.raw(ctypes.byref(net), None, None) == -22
    assert lib.dra_dqn_replay_mlp_update.raw(None, ctypes.byref(uo), None) == -22
    net.param = net.target = 4096
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, 64, 1
    pointers = [f for f, t in dqn_replay_mlp.UpdateIO._fields_ if t is ctypes.c_void_p]
    assert len(pointers) == 14

    def fill(per):
        for f in pointers:
            setattr(uo, f, 4096)
        if not per:
            uo.prob = uo.beta = uo.out_prio = uo.out_weights = None
        uo.discount, uo.step_discount, uo.replay_eps, uo.replay_alpha = 0.99 ** 3, 0.99, 0.01, 0.5
        uo.batch, uo.capacity, uo.n_step, uo.double_q = 10, 100, 3, 0
    for per in (True, False):
        for b, cap, n in ((0, 100, 3), (257, 100, 3), (10, 100, 0), (10, 100, 9), (10, 3, 3), (10, 8, 8), (10, 1, 1), (10, 1 << 31, 3)):
            fill(per)
            uo.batch, uo.capacity, uo.n_step = b, cap, n
            assert call() == -22, (per, b, cap, n)
        needed = [f for f in pointers if per or f not in ("prob", "beta", "out_prio", "out_weights")]
        for f in needed:
            if f == "prob":      # (prob NULL is the uniform mode; its companions may then be anything)
                continue
            fill(per)
            setattr(uo, f, None)
            assert call() == -22, (per, f)
        for f in ("w1", "b1", "w2", "b2", "wq", "bq"):
            fill(per)
            setattr(net, f, -1)
            assert call() == -22, (per, f)
            setattr(net, f, 0)
        fill(per)
        net.target = None
        assert call() == -22
        net.target = 4096


# ------------------------------------------------------------------------------------------ eligibility
def _replay(cls, **kw):
    from deeprl_amd.replay import ReplayWrapper
    return ReplayWrapper(cls, dict(dict(memory_size=100, batch_size=10, n_step=3, discount=0.99, history_length=1), **kw), False)


@pytest.mark.parametrize("kind", K.KINDS)
def test_why_not_names_the_first_reason(monkeypatch, kind):
    import deeprl_amd as d
    from deeprl_amd import device_env, dqn_mlp, dqn_replay_mlp
    from deeprl_amd.replay import PrioritizedReplay, UniformReplay
    d.select_device(-1)
    cls = PrioritizedReplay if kind == "per" else UniformReplay
    want_kind = dqn_replay_mlp.PerKind if kind == "per" else dqn_replay_mlp.WindowKind
    why = dqn_replay_mlp.why_not
    stub = lambda n_step=3, **kw: _stub(d, **dict(dict(replay=_replay(cls, n_step=n_step), n_step=n_step, discount=0.99,
                                                          fused_dqn_feature=False, fused_dqn_replay_feature=True), **kw))
    assert dqn_replay_mlp.kind_of(stub()) is want_kind
    assert why(stub()) == "the task is not one envs.CartPole environment, or there is no device"     # everything but a device
    monkeypatch.setattr(device_env._RolloutVec, "_host_envs", staticmethod(lambda task, config: task.env.envs))
    for n in (1, 2, 3, 8):
        assert why(stub(n)) is None and why(stub(n, double_q=True)) is None
    assert why(stub(fused_dqn_replay_feature=False)) == "config.fused_dqn_replay_feature is not on"
    assert why(stub(fused_dqn_replay_feature=1)) == "config.fused_dqn_replay_feature is not on"
    assert "not a plain DQNAgent" in why(stub(cls=d.CategoricalDQNAgent))
    assert "n_step is not between 1 and 8" in why(stub(9))
    assert "n_step is not between 1 and 8" in why(stub(replay=_replay(cls, n_step=2)))       # the replay's is not the configuration's
    assert why(stub(replay=_replay(cls, memory_size=7))) == "the replay holds fewer slots than an agent step and an n-step window need"
    assert why(stub(replay=_replay(cls, memory_size=8))) is None
    assert why(stub(replay=_replay(cls, discount=0.9))) == "the replay's discount is not the configuration's"
    assert why(stub(batch_size=257, replay=_replay(cls, batch_size=257))) == (
        "dra_dqn_replay_mlp_update is not built for minibatches of 257 over an n-step window of 3")
    assert why(stub(batch_size=257, replay=_replay(cls, batch_size=257), fused_dqn_replay_update=False)) is None
    assert why(stub(noisy_linear=True)) == "noisy_linear is on"
    assert why(stub(history_length=2)) == "history_length is not 1"
    if kind == "per":
        rp = _replay(cls)
        rp.replay.ordered_updates = True
        assert why(stub(replay=rp)) == "the replay has ordered_updates forced"
        sub = type("SubReplay", (PrioritizedReplay,), {})
        assert why(stub(replay=_replay(sub))) == "the replay is not a PrioritizedReplay"
    else:
        sub = type("SubReplay", (UniformReplay,), {})
        assert why(stub(replay=_replay(sub))) == "the replay is not a UniformReplay"
    # config.fused_dqn_feature alone keeps its two answers
    old = dqn_mlp.why_not
    assert old(stub(fused_dqn_feature=True, fused_dqn_replay_feature=False)) == (
        "the replay is a PrioritizedReplay" if kind == "per" else "n_step is not 1")
    assert old(stub(1, fused_dqn_feature=True, fused_dqn_replay_feature=False)) == (
        "the replay is a PrioritizedReplay" if kind == "per" else None)


def test_adoption_logs_the_reason_once_and_keeps_the_host_path():
    import deeprl_amd as d
    from deeprl_amd import dqn_replay_mlp
    from deeprl_amd.replay import PrioritizedReplay
    d.select_device(-1)
    a = _stub(d, replay=_replay(PrioritizedReplay), n_step=3, discount=0.99, fused_dqn_feature=False, fused_dqn_replay_feature=True)
    task = a.actor._task
    assert dqn_replay_mlp.adopt(a) is None and a.actor._task is task and type(task) is d.Task
    assert len(a.logger.warnings) == 1 and "no device" in a.logger.warnings[0]
    b = _stub(d, replay=_replay(PrioritizedReplay), n_step=3, discount=0.99, fused_dqn_feature=False)
    assert dqn_replay_mlp.adopt(b) is None and b.logger.warnings == []


def test_agent_asks_the_new_switch_behind_the_old_one():
    """DQNAgent.__init__ asks dqn_replay_mlp.adopt only under config.fused_dqn_replay_feature and only when config.fused_dqn_feature
    left no Step."""
    import inspect

    import deeprl_amd as d
    src = inspect.getsource(d.DQNAgent.__init__)
    old, new, dist = src.index("dqn_mlp.adopt(self)"), src.index("dqn_replay_mlp.adopt(self)"), src.index("dist_mlp.adopt(self)")
    assert old < new < dist
    assert "getattr(config, 'fused_dqn_replay_feature', False) is True and self._feature is None" in src


def test_the_step_overrides_only_what_differs():
    from deeprl_amd import dqn_mlp, dqn_replay_mlp as m
    own = lambda cls: {k for k, v in vars(cls).items() if inspect.isfunction(v) and not k.startswith("__")}
    assert own(m.Step) == {"replay_io", "update"}
    assert own(m.PerStep) == {"staged_tail", "make_outputs", "replay_io", "module_update", "prepare", "after_learn"}
    assert m.Step.KIND is m.WindowKind and m.PerStep.KIND is m.PerKind and issubclass(m.PerStep, m.Step) and issubclass(m.Step, dqn_mlp.Step)
    for kind, per in ((m.WindowKind, False), (m.PerKind, True)):
        assert (kind.PRIORITIZED, kind.MAX_N_STEP, kind.NOISY) == (per, 8, False)
        assert (kind.SWITCH, kind.UPDATE_SWITCH) == ("fused_dqn_replay_feature", "fused_dqn_replay_update") == (m.SWITCH, m.UPDATE_SWITCH)
        assert (kind.ACT, kind.EVAL, kind.UPDATE, kind.ENTRY) == ("dra_dqn_mlp_act", "dra_dqn_mlp_eval", "dra_dqn_replay_mlp_update", "dqn_feature")
        assert kind.Net is dqn_mlp.Net and kind.AGENTS == ("DQNAgent",)


def test_staged_beta_sits_directly_behind_the_last_probability():
    """ops.td_loss reads a device beta at sampling_prob[B] (beta < 0): PerStep.staged_tail puts it there, for even and odd B."""
    from deeprl_amd import dqn_replay_mlp as m
    for b in (1, 8, 10, 255, 256):
        s = m.PerStep.__new__(m.PerStep)
        s.batch, s._o_tail = b, 128
        tail = s.staged_tail()
        assert s._o_prob == 128 and s._o_beta == 128 + 4 * b and tail % 8 == 0 and tail >= 4 * b + 4


# ------------------------------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("n_step", K.FOLD_N_STEPS)
def test_restated_fold_is_the_reference_replays(n_step):
    """tests/golden/dqn_replay_feature/replay_fold.npz: at every index the reference's UniformReplay calls valid, the restatement's
    minibatch has the reference's next frame, folded reward (narrowed as tensor() does) and mask; every other index is invalid."""
    z = np.load(os.path.join(GOLDEN, "replay_fold.npz"))
    rg = K.make_ring(K.FOLD_RING)
    assert int(z["pos"]) == rg["pos"] and int(z["size"]) == rg["size"]
    rows = z["n%d" % n_step]
    valid = [i for i in range(rg["size"]) if R.valid_index(i, rg["pos"], rg["size"], n_step)]
    assert [int(r[0]) for r in rows] == valid and len(valid) >= 40
    mb = R.minibatch(rg["ring"], np.asarray(valid), n_step, K.DISCOUNT)
    assert [int(r[1]) for r in rows] == [i + n_step for i in valid]
    assert np.array_equal(mb["reward"], rows[:, 2].astype(np.float32)) and np.array_equal(mb["mask"], rows[:, 3].astype(np.float32))
    assert [R.fold(rg["ring"]["rewards"], rg["ring"]["masks"], i, n_step, K.DISCOUNT)[0] for i in valid] == list(rows[:, 2])
    if n_step > 1:
        assert (rows[:, 3] == 0).any() and (rows[:, 3] == 1).any() == (n_step < 8) and len(set(rows[:, 2])) >= min(n_step, 3)


@pytest.mark.parametrize("tag", [t[0] for t in K.FIXTURE_TAGS])
def test_restatement_reproduces_the_reference_steps(tag):
    """tests/golden/dqn_replay_feature/steps.npz: from the recorded initial parameters and seeds the restatement's agent run has the
    reference's actions, explore flags, ring, data indices, (per) drawn leaves, leaves, pending set and generator tails to the word;
    probabilities, totals, the tree and max_priority within 1e-5 of scale against the reference's fp32 priorities; td, priorities and
    the parameters behind every step within rtol 2e-5 / atol 2e-6."""
    z = np.load(os.path.join(GOLDEN, "steps.npz"))
    f = K.FIXTURE
    per = next(t for t in K.FIXTURE_TAGS if t[0] == tag)[1]
    got = K.restated(z, tag)
    k = tag + "_"
    ups = [u for u in got["updates"] if u is not None]
    assert np.array_equal(got["actions"], z[k + "actions"]) and np.array_equal(got["flags"], z[k + "flags"])
    assert np.array_equal(got["random_actions"], z[k + "random_actions"])
    assert [s for s, u in enumerate(got["updates"]) if u is not None] == list(z[k + "update_steps"]) and got["copies"] == list(z[k + "copies"])
    assert np.array_equal(got["ring"]["frames"], z[k + "ring_frames"]) and np.array_equal(got["ring"]["rewards"], z[k + "ring_rewards"])
    assert np.array_equal(got["ring"]["actions"], z[k + "ring_actions"]) and np.array_equal(got["ring"]["masks"], z[k + "ring_masks"])
    assert got["pos"] == int(z[k + "pos"]) and got["total"] == int(z[k + "total_steps"]) == f["steps"] * f["k"]
    assert np.array_equal(got["rng_tail"], z[k + "np_tail"]) and np.array_equal(got["random_tail"], z[k + "random_tail"])
    for u, data, td in zip(ups, z[k + "data"], z[k + "td"]):
        assert np.array_equal(u["data"], data)
        np.testing.assert_allclose(u["td"], td, rtol=2e-5, atol=2e-6)
    if per:
        for i, u in enumerate(ups):
            assert np.array_equal(u["drawn"], z[k + "drawn"][i]) and np.array_equal(u["leaves"], z[k + "leaves"][i])
            assert u["beta"] == z[k + "beta"][i]
            np.testing.assert_allclose(u["prob"], z[k + "prob"][i], rtol=1e-5)
            np.testing.assert_allclose(u["total"], z[k + "total_before"][i], rtol=1e-5)
            np.testing.assert_allclose(u["prio"], z[k + "prio"][i], rtol=2e-5, atol=2e-6)
        assert got["pending"] == list(z[k + "pending"])
        np.testing.assert_allclose(got["tree"], z[k + "tree"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got["max_priority"], float(z[k + "max_priority"]), rtol=1e-5)
    for name in R.KEYS:
        np.testing.assert_allclose(np.stack([p[name] for p in got["params"]]), z[k + "params_" + name], rtol=2e-5, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(got["target"][name], z[k + "target_" + name], rtol=2e-5, atol=2e-6, err_msg=name)
    padded, twice, terminal, margin = K.run_conditions(got, per)
    assert terminal >= 1 and margin >= K.MARGIN and (not per or (padded >= 1 and twice >= 1))


def test_fixture_holds_data_only_and_is_small():
    names = sorted(os.listdir(GOLDEN))
    assert names == ["learning_reference.json", "replay_fold.npz", "steps.npz"]
    assert sum(os.path.getsize(os.path.join(GOLDEN, n)) for n in names) < 256 * 1024
    for n in names:
        if n.endswith(".npz"):
            z = np.load(os.path.join(GOLDEN, n), allow_pickle=False)
            assert all(z[k].dtype.kind in "fiub" for k in z.files), n
    ref = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))
    rand = json.load(open(os.path.join(os.path.dirname(GOLDEN), "dqn_feature", "random_policy.json")))["mean"]
    assert ref["bar"] == 2.0 * rand and abs(ref["bar"] - 44.157) < 1e-3 and set(ref["n_learn"]) == set(K.KINDS)
    for kind in K.KINDS:
        one = ref["kinds"][kind]
        assert one["seeds"] == [1, 2, 3, 4, 5] and sorted(one["medians"], key=int) == ["10000", "15000", "25000"]
        reached = [n for n in (10000, 15000, 25000) if one["medians"][str(n)] >= 2.0 * ref["bar"]]
        assert ref["n_learn"][kind] == (reached[0] if reached else None)


# ------------------------------------------------------------------------------------------ what the case tables cover
def test_update_cases_are_the_stated_ones():
    c = K.UPDATE_CASES
    assert {x[0] for x in c} == {16, 32, 64} and {x[1] for x in c} == {"relu", "tanh"}
    assert {x[2] for x in c} == {1, 10, 63, 64, 65, 256} and {x[4] for x in c} == {1, 2, 3, 8}
    assert {x[3] for x in c} == {False, True} and {x[7] for x in c if x[6]} == {0.5, 0.7} and {x[8] for x in c if x[6]} == {0.4, 1.0}
    assert any(not x[6] for x in c) and any(x[6] and x[2] == 65 for x in c) and any(x[6] and x[2] == 256 for x in c)
    for name in ("window_full", "window_long"):
        rg = K.make_ring(name)
        assert rg["size"] == K.RINGS[name]["capacity"] and 0 < rg["pos"] < rg["size"] - 1 - K.MAX_N_STEP
        assert np.isfinite(rg["ring"]["frames"]).all() and (rg["ring"]["masks"] == 0).sum() >= 5


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_cases_have_margin_and_cover_their_edges(case):
    hidden, gate, batch, double_q, n_step, kind, per, alpha, beta = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    idx, masks, cap = u["idx"], rg["ring"]["masks"], K.RINGS[kind]["capacity"]
    assert idx.shape == (batch,) and all(R.valid_index(int(i), rg["pos"], rg["size"], n_step) for i in idx)
    assert idx.min() >= 0 and idx.max() <= cap - 1 - n_step
    if batch >= 10:
        for row, where in enumerate((0, n_step // 2, n_step - 1)):
            assert masks[idx[row] + where] == 0, (row, where)
        assert idx[3] == cap - 1 - n_step and idx[4] == idx[5]
        assert (u["batch"]["mask"] == 0).any()
        assert (u["batch"]["action"] == 0).any() and (u["batch"]["action"] == 1).any()
    if batch >= 63 and n_step < 8:
        assert (u["batch"]["mask"] == 1).any() and len(set(u["batch"]["reward"].tolist())) >= 2
    if per:
        w = u["weights"]
        assert u["prob"].dtype == np.float32 and w.max() == 1.0 and (batch == 1 or w.min() < 0.9)
        if batch >= 65:
            assert int(np.argmax(w)) == batch - 1 >= 64 * ((batch - 1) // 64) and (w[:64] < 0.5).all()
        assert (u["prio"] > 0).all()
    else:
        assert u["prob"] is None and u["weights"] is None and u["prio"] is None
    if gate == "relu":
        assert u["min_preact"] >= K.PREACT_MARGIN
    if double_q:
        assert u["argmax_margin"] >= K.MARGIN and u["fp32_same_argmax"]


@pytest.mark.parametrize("kind", K.KINDS)
def test_agent_case_has_margin_and_covers_its_edges(kind):
    a, want = K.agent_cfg(kind), K.restated_agent_run(kind)
    want32 = K.restated_agent_run(kind, dtype=torch.float32)
    per = kind == "per"
    assert K.agent_run_ok(kind, want, want32)
    padded, twice, terminal, margin = K.run_conditions(want, per)
    assert margin >= K.MARGIN and want["leaf_margin"] >= K.MARGIN and terminal >= 1 and (not per or (padded >= 1 and twice >= 1))
    assert want["copies"] == [2, 5, 8] and want["total"] == a["steps"] * a["k"] > a["capacity"]      # copies inside, the ring wraps
    assert a["k"] < a["exploration_steps"] < 2 * a["k"]                                           # crossed inside the second step
    assert [u is None for u in want["updates"]] == [True] + [False] * (a["steps"] - 1)
    assert want["flags"].any() and (~want["flags"]).any() and len(want["events"]) >= 4
