"""n_step_dqn_feature, host side (no GPU): the zoo entry against the Config the reference's examples.py::n_step_dqn_feature
builds, the committed fixtures against a live run of the reference (tests/golden/make_golden_nstep_feature.py), the restatement
the GPU tests lean on (tests/nstep_feature_restatement.py) against the reference's recorded NStepDQNAgent.step, the conditions on
the test inputs the GPU comparisons rest on (Q margins, exploring and greedy pairs, relu pre-activation margins, episode ends),
the ctypes mirrors of the kernels' structs, the shapes the kernels take, and which configurations NStepDQNAgent moves to the
device."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import nstep_feature_cases as K
import nstep_feature_restatement as R
import ref_shim
from golden import crosscheck_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nstep_feature")
RECORD = os.path.join(GOLDEN, "nstep_feature_config.json")
FIXTURE = os.path.join(GOLDEN, "nstep_feature_step.npz")
RANDOM = os.path.join(GOLDEN, "random_policy.json")
LEARNING = os.path.join(GOLDEN, "learning_reference.json")
TAGS = ("t5n5", "t3n2", "t3n2_sync")
LENGTHS = (50000, 100000, 150000, 200000)

needs_ref = pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    """These tests seed np.random and switch the package's device; the tests after them see what they saw before."""
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


# ------------------------------------------------------------------------------------------ records
def test_random_policy_mean_is_the_committed_one():
    rec = json.load(open(RANDOM))
    assert rec["episodes"] == 2000 and rec["mean"] == K.random_policy_mean(rec["episodes"], rec["seed"], rec["env_seed"])
    assert 15.0 < rec["mean"] < 30.0


def test_learning_reference_record():
    """The hand-regenerated record of the reference's own learning runs: at the chosen length its median is >= 2 x the bar, the
    bar is 2 x the committed random-policy mean, 5 seeds, and no shorter length reached it."""
    rec, rnd = json.load(open(LEARNING)), json.load(open(RANDOM))
    assert rec["random_policy_mean"] == rnd["mean"] and rec["bar"] == 2.0 * rnd["mean"] and len(rec["seeds"]) == 5
    n = rec["n_learn"]
    assert n in LENGTHS
    assert rec["medians"][str(n)] >= 2.0 * rec["bar"] == rec["reference_must_reach"]
    assert all(rec["medians"][str(m)] < 2.0 * rec["bar"] for m in LENGTHS if m < n)
    assert rec["medians"][str(n)] == float(np.median([r["ends"][str(n)]["last_mean"] for r in rec["runs"]]))


def test_zoo_n_step_dqn_feature_equals_reference_example():
    import deeprl_amd as d
    from deeprl_amd import zoo
    rec = json.load(open(RECORD))
    want = rec["config"]
    assert rec["agent"] == zoo.ZOO["n_step_dqn_feature"]["agent"] == "NStepDQNAgent"
    d.select_device(-1)
    np.random.seed(0)
    cfg = zoo.config("n_step_dqn_feature", game=rec["game"])
    have = C.describe_config(cfg)
    assert rec["game"] == "classic-CartPole-v0"
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert want[k] == have[k], "%s: reference %s, zoo %s" % (k, want[k], have[k])
    assert callable(zoo.n_step_dqn_feature)
    assert getattr(cfg, "fused_nstep_feature", False) is not True          # the device path is opt-in
    assert zoo.config("n_step_dqn_feature", game=rec["game"], fused_nstep_feature=True).fused_nstep_feature is True


@needs_ref
def test_nstep_feature_fixtures_are_the_reference_output(tmp_path):
    """tests/golden/make_golden_nstep_feature.py run live in a fresh interpreter (importing the reference installs stand-in
    modules that must not leak into the other tests): the same records, the same arrays, bit for bit."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable] + flags + [os.path.join(ROOT, "tests", "golden", "make_golden_nstep_feature.py")],
                          env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = os.path.join(str(tmp_path), "nstep_feature")
    assert json.load(open(os.path.join(out, "nstep_feature_config.json"))) == json.load(open(RECORD))
    assert json.load(open(os.path.join(out, "random_policy.json"))) == json.load(open(RANDOM))
    fresh, committed = dict(np.load(os.path.join(out, "nstep_feature_step.npz"))), dict(np.load(FIXTURE))
    assert sorted(fresh) == sorted(committed)
    for k in committed:
        assert fresh[k].dtype == committed[k].dtype and np.array_equal(fresh[k], committed[k]), k


def _params(g, tag, which):
    pre = "%s_%s_" % (tag, which)
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def test_fixture_holds_data_only_and_is_small():
    assert os.path.getsize(FIXTURE) < 256 * 1024 and os.path.getsize(RECORD) < 16 * 1024
    g = np.load(FIXTURE, allow_pickle=False)
    for tag in TAGS:
        t_len, n = int(g[tag + "_cfg"][3]), int(g[tag + "_cfg"][4])
        assert g[tag + "_states"].shape == (t_len + 1, n, 4) and g[tag + "_states"].dtype == np.float32
        assert g[tag + "_q"].shape == (t_len, n, 2) and g[tag + "_action"].shape == (t_len, n, 1)
        assert g[tag + "_explore"].shape == g[tag + "_random_action"].shape == (t_len, n)
        assert g[tag + "_explore"].any() and not g[tag + "_explore"].all()
        assert (g[tag + "_reward"] == 1.0).all()
        init, target = _params(g, tag, "init"), _params(g, tag, "target")
        assert set(init) == set(target) == set(R.KEYS)
        assert all(not np.array_equal(init[k], target[k]) for k in R.KEYS if not k.endswith("bias"))      # another seed
    assert (int(g["t5n5_cfg"][3]), int(g["t5n5_cfg"][4]), int(g["t5n5_cfg"][5])) == (5, 5, 200)
    for tag in ("t3n2", "t3n2_sync"):
        assert int(g[tag + "_cfg"][5]) == 2 and (g[tag + "_mask"] == 0).any() and (g[tag + "_mask"] == 1).any()
    assert int(g["t3n2_sync_cfg"][6]) == 2 and int(g["t3n2_cfg"][6]) == int(g["t5n5_cfg"][6]) == 200


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_step(tag):
    """The restatement from the fixture's start (the task's seed, the initial online and target parameters, the draws the
    reference made): actions, masks, the float32 observations equal; the fp32 return scan equal to the bit from the reference's
    bootstrap (the reference's loop and operation order); q, bootstrap, ret and the loss of the fp64 restatement within 1e-5 of
    each tensor's largest magnitude (floor 1: the reference ran in fp32); the parameters after the update within rtol 2e-5 /
    atol 2e-6 (the bars of the GPU update test, which compares the kernels with the same fixture).  In the sync tag the target
    copy fell inside the rollout: the bootstrap is the ONLINE network's, and bootstrapping from the stored target parameters
    misses the reference."""
    g = np.load(FIXTURE)
    discount, clip, lr = [float(x) for x in g[tag + "_cfg"][:3]]
    t_len, n, horizon, freq, env_seed = [int(x) for x in g[tag + "_cfg"][3:8]]
    init, target = _params(g, tag, "init"), _params(g, tag, "target")
    boot_params = init if freq <= t_len else target
    envs, raw = K.make_envs(n, env_seed, horizon)
    roll = R.rollout(init, boot_params, envs, raw, t_len, g[tag + "_explore"], g[tag + "_random_action"], gate="relu")
    assert roll["margin"] >= K.MARGIN
    assert np.array_equal(roll["action"], g[tag + "_action"].reshape(t_len, n))
    assert np.array_equal(roll["mask"], g[tag + "_mask"].reshape(t_len, n))
    assert np.array_equal(roll["state"], g[tag + "_states"][:t_len]) and np.array_equal(roll["bootstrap_state"], g[tag + "_states"][t_len])
    within = lambda got, want: np.abs(np.asarray(got, dtype=np.float64) - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert within(roll["q"], g[tag + "_q"].astype(np.float64))
    assert within(roll["bootstrap"], g[tag + "_bootstrap"].astype(np.float64))
    ret32 = R.returns(g[tag + "_reward"].reshape(t_len, n), g[tag + "_mask"].reshape(t_len, n), g[tag + "_bootstrap"], discount,
                      dtype=np.float32)
    assert ret32.dtype == np.float32 and np.array_equal(ret32, g[tag + "_ret"].reshape(t_len, n))
    new, keep = R.nstep_update(init, boot_params, g[tag + "_states"], roll["action"], roll["reward"], roll["mask"], discount, clip, lr)
    assert within(keep["ret"], g[tag + "_ret"].reshape(t_len, n).astype(np.float64))
    assert within(keep["loss"], np.asarray(float(g[tag + "_loss"])))
    final = _params(g, tag, "final")
    assert set(final) == set(new)
    moved = 0
    for k in final:
        np.testing.assert_allclose(new[k], final[k], rtol=2e-5, atol=2e-6, err_msg=k)
        moved += int((final[k] != init[k]).sum())
    assert moved > 100          # the update moved the parameters: the comparison above is not of two copies of the start
    # bootstrapping from the WRONG network misses the reference's returns
    wrong, _ = R.nstep_update(init, target if boot_params is init else init, g[tag + "_states"], roll["action"], roll["reward"],
                              roll["mask"], discount, clip, lr)
    if (g[tag + "_mask"][t_len - 1] != 0).any():
        assert any(not np.allclose(wrong[k], final[k], rtol=2e-5, atol=2e-6) for k in final)


def test_restatement_returns_follow_the_reference_order():
    """r + (discount * m) * ret, one rounding per operation: against torch's fp32 tensors running NStepDQN_agent.py:58-60."""
    rs = np.random.RandomState(5)
    reward, mask = rs.randn(7, 9).astype(np.float32), (rs.rand(7, 9) > 0.3).astype(np.float32)
    boot = rs.randn(9).astype(np.float32)
    ret = torch.from_numpy(boot)
    want = []
    for i in reversed(range(7)):
        ret = torch.from_numpy(reward[i]) + 0.99 * torch.from_numpy(mask[i]) * ret
        want.append(ret.numpy())
    assert np.array_equal(R.returns(reward, mask, boot, 0.99, dtype=np.float32), np.stack(want[::-1]))


# ------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("case", K.ROLLOUT_CASES, ids=K.case_id)
def test_rollout_cases_have_margin_and_cover_their_edges(case):
    """The smallest gap between the two Q values at a NON-exploring (step, environment) of the fp64 restatement is >= 1e-4 (fp32
    forwards differ from it by ~1e-6: no correct implementation picks another action), an fp32 run of the restatement picks the
    same actions, cases with 8 or more pairs explore and act greedily, the online and target parameters differ, and the
    short-horizon cases end episodes inside the rollout (ring rows)."""
    hidden, gate, n, t_len, horizon, padded, pseed, tseed, _ = case
    want, envs, start = K.restated_rollout(case)
    print("%s: margin %.3e, %d episodes ended" % (K.case_id(case), want["margin"], len(want["events"])))
    assert want["margin"] >= K.MARGIN and want["fp32_same_actions"]
    assert [e.c for e in envs] == [t_len] * n
    assert pseed != tseed and not np.array_equal(start["params"]["fc_head.weight"], start["target"]["fc_head.weight"])
    if n * t_len >= 8:
        assert start["explore"].any() and not start["explore"].all()
        assert set(np.unique(want["action"])) == {0, 1}
    if horizon <= t_len:
        assert len(want["events"]) >= n * (t_len // horizon) and (want["mask"] == 0).sum() == len(want["events"])
        assert want["events"] == sorted(want["events"])                            # (step, environment) order
        assert all(r <= horizon for _, _, r in want["events"])
    if horizon == 3:
        assert len(want["events"]) > K.RING_CAP - K.RING_COUNT0                     # the GPU test's short ring wraps
    # the bootstrap is the TARGET network's: the online parameters give another one
    online = R.forward(R.to_t(start["params"]), want["bootstrap_state"], gate).numpy().max(axis=1)
    assert np.abs(online - want["bootstrap"]).max() > 1e-3


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_cases_cover_their_edges(case):
    """Relu cases keep every pre-activation of both hidden layers at least 1e-5 from zero (the fp32 kernel takes the derivative
    the fp64 restatement takes); the row counts are the ones the table states; the short-horizon cases hold zero masks; the
    one-action case holds action 0 alone."""
    hidden, gate, n, t_len, horizon, force_zero = case[:6]
    u = K.restated_update(case)
    print("%s: smallest |pre-activation| %.3e, loss %.4f" % (K.update_id(case), u["min_preact"], u["loss"]))
    if gate == "relu":
        assert u["min_preact"] >= K.PREACT_MARGIN
    assert u["inputs"]["state"].shape == (t_len, n, 4) and n * t_len <= K.UPDATE_CAP
    if horizon <= t_len:
        assert (u["inputs"]["mask"] == 0).any() and (u["inputs"]["mask"] == 1).any() and len(u["events"]) > 0
    acts = set(np.unique(u["inputs"]["action"]))
    assert acts == ({0} if force_zero else ({0, 1} if n * t_len >= 8 else acts))
    if force_zero:
        assert not u["grads"]["fc_head.weight"][1].any() and u["grads"]["fc_head.bias"][1] == 0.0
        assert np.abs(u["grads"]["fc_head.weight"][0]).max() > 1e-3
    assert all(np.isfinite(v).all() for v in u["grads"].values()) and np.isfinite(u["loss"])


def test_update_cases_hold_the_stated_row_counts():
    rows = [c[2] * c[3] for c in K.UPDATE_CASES]
    assert rows == [1, 25, 51, 320, K.UPDATE_CAP, 32]


def test_agent_case_has_margin():
    run = K.restated_agent_run()
    print("agent case: margin %.3e, %d episodes, %d exploring / %d greedy" % (run["margin"], len(run["events"]), run["explored"], run["greedy"]))
    assert run["margin"] >= K.MARGIN and run["fp32_same_actions"]
    assert run["explored"] >= 8 and run["greedy"] >= 8
    assert len(run["events"]) >= 8 and (run["masks"] == 0).sum() == len(run["events"])
    moved = sum(int((np.asarray(run["params"][k], dtype=np.float32) != run["init"][k]).sum()) for k in run["init"])
    assert moved > 100


def test_plan_epsilon_greedy_is_the_restated_draw_order():
    """The agent case's restated draws (randint, then rand, per step, the schedule called with the worker count) are the ones
    support.plan_epsilon_greedy makes."""
    from deeprl_amd.support import LinearSchedule, plan_epsilon_greedy
    a = K.AGENT
    np.random.seed(a["np_seed"])
    sched = LinearSchedule(*a["eps"])
    rs = np.random.RandomState(a["np_seed"])
    eps = K.epsilon_schedule(*a["eps"])
    for _ in range(a["steps"]):
        explore, rand = plan_epsilon_greedy(sched, a["t_len"], a["n_env"], 2, a["n_env"])
        for t in range(a["t_len"]):
            e = eps(a["n_env"])
            assert np.array_equal(rand[t], rs.randint(2, size=a["n_env"])) and np.array_equal(explore[t], rs.rand(a["n_env"]) < e)
    assert sched.current == eps.state["current"] == K.restated_agent_run()["epsilon"]


# ------------------------------------------------------------------------------------------ C ABI mirrors, shapes
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_q_mlp_net", "dra_q_mlp_rollout_io", "dra_q_mlp_update_io"])
def test_ctypes_mirror_matches_the_header(tmp_path, which):
    from deeprl_amd import q_mlp
    from test_struct_layouts import _c_layout
    mirror = {"dra_q_mlp_net": q_mlp.Net, "dra_q_mlp_rollout_io": q_mlp.RolloutIO, "dra_q_mlp_update_io": q_mlp.UpdateIO}[which]
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, which, names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_supported_shapes():
    from deeprl_amd import cat_mlp, q_mlp
    ok = q_mlp.supported
    assert ok(4, 2, 64, 5, 1) and ok(4, 2, 16, 1, 1) and ok(4, 2, 32, 64, 2) and ok(4, 2, 64, 64, 1)
    assert not ok(5, 2, 64, 5, 2) and not ok(3, 2, 64, 5, 2) and not ok(4, 3, 64, 5, 2) and not ok(4, 1, 64, 5, 2)
    assert not ok(4, 2, 48, 5, 2) and not ok(4, 2, 128, 5, 2) and not ok(4, 2, 8, 5, 2)
    assert not ok(4, 2, 64, 65, 2) and not ok(4, 2, 64, 0, 2) and not ok(4, 2, 64, 5, 0) and not ok(4, 2, 64, 5, 3)
    for h in (8, 16, 32, 48, 64, 128):          # the shapes dra_cat_mlp_supported takes
        for n in (0, 1, 5, 64, 65):
            for gate in (0, 1, 2, 3):
                assert ok(4, 2, h, n, gate) == cat_mlp.supported(4, 2, h, n, gate)
    up = q_mlp.update_supported
    assert K.UPDATE_CAP >= 320
    assert up(4, 2, 64, 1, 1) and up(4, 2, 16, 320, 2) and up(4, 2, 32, K.UPDATE_CAP, 1)
    assert all(up(4, 2, 64, 5 * n, 1) for n in range(1, 65))        # every n_env the rollout takes at the example's T = 5
    assert not up(4, 2, 32, K.UPDATE_CAP + 1, 1) and not up(4, 2, 32, 0, 1) and not up(4, 2, 48, 25, 1) and not up(4, 2, 64, 25, 3)
    assert not up(5, 2, 64, 25, 1) and not up(4, 3, 64, 25, 1)


def test_kernels_refuse_unsupported_shapes_before_any_launch():
    """dra_q_mlp_rollout / dra_q_mlp_update validate on the host: null pointers and shapes outside the table are DRA_EINVAL
    without a device."""
    from deeprl_amd import q_mlp
    from deeprl_amd._lib import lib
    net, io, uo = q_mlp.Net(), q_mlp.RolloutIO(), q_mlp.UpdateIO()
    assert lib.dra_q_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    assert lib.dra_q_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22
    net.param = net.target = 4096
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, 48, 1
    io.n_env, io.t_len, io.horizon, io.ring_cap = 5, 5, 200, 64
    assert lib.dra_q_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    net.hidden = 64
    uo.t_len, uo.n_env = 17, 64            # 1088 rows: above the cap, refused before the pointers are looked at
    for f in ("state", "action", "reward", "mask", "bootstrap", "grad", "out_ret", "out_loss"):
        setattr(uo, f, 4096)
    assert lib.dra_q_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22
    uo.t_len, uo.n_env = 1 << 20, 1 << 20  # (a row count that overflows 32 bits)
    assert lib.dra_q_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22


# ------------------------------------------------------------------------------------------ eligibility
class _Fused:
    def __init__(self, flat):
        self.flat = flat


class _Agent:
    """What q_mlp.why_not reads of an NStepDQNAgent."""

    def __init__(self, d, network, target, target_order=None, **cfg):
        from deeprl_amd.optim import FlatParams
        self.config = d.Config()
        self.config.num_workers, self.config.rollout_length = 5, 5
        for k, v in cfg.items():
            setattr(self.config, k, v)
        self.network, self.target_network, self.grad_hook = network, target, None
        self._fused = _Fused(FlatParams(list(network.parameters())))
        tp = list(target.parameters())
        self._target_flat = FlatParams(tp if target_order is None else [tp[i] for i in target_order])


def test_why_not_names_the_first_reason():
    import deeprl_amd as d
    from deeprl_amd import q_mlp
    d.select_device(-1)
    net = lambda *a, **k: d.VanillaNet(2, d.FCBody(4, *a, **k))
    yes = lambda *a: True
    on = dict(fused_nstep_feature=True)
    assert q_mlp.why_not(_Agent(d, net(), net(), **on), yes) is None
    assert q_mlp.why_not(_Agent(d, net(gate=torch.tanh), net(gate=torch.tanh), **on), yes) is None
    assert q_mlp.why_not(_Agent(d, net(), net()), yes) == "config.fused_nstep_feature is not on"                 # opt-in
    assert "not on" in q_mlp.why_not(_Agent(d, net(), net(), fused_nstep_feature=1), yes)
    a = _Agent(d, net(), net(), **on)
    a.grad_hook = lambda g: None
    assert q_mlp.why_not(a, yes) == "a grad_hook is installed"
    assert "the network is not VanillaNet" in q_mlp.why_not(_Agent(d, net((64, 64, 64)), net((64, 64, 64)), **on), yes)
    assert "the network is not VanillaNet" in q_mlp.why_not(_Agent(d, net((64, 32)), net((64, 32)), **on), yes)
    assert "the network is not VanillaNet" in q_mlp.why_not(_Agent(d, net(), net((32, 32)), **on), yes)
    assert "laid out differently" in q_mlp.why_not(_Agent(d, net(), net(), target_order=[5, 4, 3, 2, 1, 0], **on), yes)
    a = _Agent(d, net(), net(), **on)
    a._fused.flat.params = a._fused.flat.params[:-1]
    assert "one optimiser does not own" in q_mlp.why_not(a, yes)
    assert "not built for" in q_mlp.why_not(_Agent(d, net(), net(), **on), lambda *s: False)
    assert "not built for" in q_mlp.why_not(_Agent(d, net(), net(), num_workers=65, **on))
    assert "dra_q_mlp_update is not built for 1280 rows" in q_mlp.why_not(_Agent(d, net(), net(), num_workers=64, rollout_length=20, **on))
    assert q_mlp.why_not(_Agent(d, net(), net(), num_workers=64, rollout_length=20, fused_nstep_update=False, **on)) is None
    assert q_mlp.shape(net()) == (4, 2, 64, 1) and q_mlp.shape(net((16, 16), gate=torch.tanh)) == (4, 2, 16, 2)
    assert q_mlp.shape(d.CategoricalActorCriticNet(4, 2, d.FCBody(4))) is None


def test_adoption_without_a_device_keeps_the_host_path():
    """Without a device the switch cannot move anything: NStepDQNAgent._adopt_feature leaves envs.Task in place and logs the
    reason at warning level; with the default Config it logs nothing.  (The agent itself needs a device to be built: its target
    copy is a kernel.)"""
    import deeprl_amd as d
    from deeprl_amd import zoo
    d.select_device(-1)
    warned = []

    class Rec:
        def info(self, *a, **k):
            pass

        def warning(self, msg, *a, **k):
            warned.append(str(msg))

    for switch in (False, True):
        cfg = zoo.config("n_step_dqn_feature", game="classic-CartPole-v0", tag="nstep_feat_host%d" % switch,
                         **(dict(fused_nstep_feature=True) if switch else {}))
        agent = d.NStepDQNAgent.__new__(d.NStepDQNAgent)
        agent.config, agent.logger, agent.task = cfg, Rec(), cfg.task_fn()
        assert agent._adopt_feature() is None and type(agent.task) is d.Task
        assert len(warned) == int(switch)
    assert "stay on the host" in warned[0] and "no device" in warned[0]
