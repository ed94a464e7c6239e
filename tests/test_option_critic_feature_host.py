"""option_critic_feature, host side (no GPU): the zoo entry against the Config the reference's examples.py::option_critic_feature
builds, the committed fixtures against a live run of the reference (tests/golden/make_golden_option_critic_feature.py), the
restatement the GPU tests lean on (tests/option_critic_feature_restatement.py) against the reference's recorded
OptionCriticAgent.step, the conditions on the test inputs the GPU comparisons rest on (decision margins, both option branches,
relu pre-activation margins, episode ends), the ctypes mirrors of the kernels' structs, the shapes the kernels take, and which
configurations OptionCriticAgent moves to the device."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import option_critic_feature_cases as K
import option_critic_feature_restatement as R
import ref_shim
from golden import crosscheck_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "option_critic_feature")
RECORD = os.path.join(GOLDEN, "option_critic_feature_config.json")
FIXTURE = os.path.join(GOLDEN, "option_critic_feature_step.npz")
RANDOM = os.path.join(GOLDEN, "random_policy.json")
LEARNING = os.path.join(GOLDEN, "learning_reference.json")
TAGS = ("t5n5", "t3n2", "t3n2_o3")
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
    """The hand-regenerated record of the reference's own learning runs, 5 seeds.  Where a length reached 2 x (2 x the random
    policy's mean) in the median, n_learn is the smallest such length and the bar 2 x the random policy's mean; else n_learn is
    200 000 and the bar half the reference's median there, and `learns` says whether that is at least 1.25 x the random policy's
    mean (the GPU suite has a closed-loop test only then)."""
    rec, rnd = json.load(open(LEARNING)), json.load(open(RANDOM))
    assert rec["random_policy_mean"] == rnd["mean"] and len(rec["seeds"]) == 5
    n = rec["n_learn"]
    assert n in LENGTHS
    assert rec["medians"][str(n)] == float(np.median([r["ends"][str(n)]["last_mean"] for r in rec["runs"]]))
    reached = [m for m in LENGTHS if rec["medians"][str(m)] >= 4.0 * rnd["mean"]]
    if reached:
        assert n == reached[0] and rec["bar"] == 2.0 * rnd["mean"] and rec["learns"] is True
        assert rec["medians"][str(n)] >= 2.0 * rec["bar"] == rec["reference_must_reach"]
    else:
        assert n == LENGTHS[-1] and rec["bar"] == 0.5 * rec["medians"][str(n)]
        assert rec["learns"] == (rec["bar"] >= 1.25 * rnd["mean"])


def test_zoo_option_critic_feature_equals_reference_example():
    import deeprl_amd as d
    from deeprl_amd import zoo
    rec = json.load(open(RECORD))
    want = rec["config"]
    assert rec["agent"] == zoo.ZOO["option_critic_feature"]["agent"] == "OptionCriticAgent"
    d.select_device(-1)
    np.random.seed(0)
    cfg = zoo.config("option_critic_feature", game=rec["game"])
    have = C.describe_config(cfg)
    assert rec["game"] == "classic-CartPole-v0"
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert want[k] == have[k], "%s: reference %s, zoo %s" % (k, want[k], have[k])
    assert callable(zoo.option_critic_feature)
    assert getattr(cfg, "fused_oc_feature", False) is not True          # the device path is opt-in
    assert zoo.config("option_critic_feature", game=rec["game"], fused_oc_feature=True).fused_oc_feature is True
    net = cfg.network_fn()
    assert int(net.num_options) == 2 and cfg.random_option_prob(0) == 1.0 and cfg.num_workers == 5


@needs_ref
def test_option_critic_feature_fixtures_are_the_reference_output(tmp_path):
    """tests/golden/make_golden_option_critic_feature.py run live in a fresh interpreter (importing the reference installs
    stand-in modules that must not leak into the other tests): the same records, the same arrays, bit for bit."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable] + flags + [os.path.join(ROOT, "tests", "golden", "make_golden_option_critic_feature.py")],
                          env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = os.path.join(str(tmp_path), "option_critic_feature")
    assert json.load(open(os.path.join(out, "option_critic_feature_config.json"))) == json.load(open(RECORD))
    assert json.load(open(os.path.join(out, "random_policy.json"))) == json.load(open(RANDOM))
    fresh, committed = dict(np.load(os.path.join(out, "option_critic_feature_step.npz"))), dict(np.load(FIXTURE))
    assert sorted(fresh) == sorted(committed)
    for k in committed:
        assert fresh[k].dtype == committed[k].dtype and np.array_equal(fresh[k], committed[k]), k


def _params(g, tag, which):
    pre = "%s_%s_" % (tag, which)
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def _cfg(g, tag):
    c = g[tag + "_cfg"]
    return dict(discount=float(c[0]), clip=float(c[1]), lr=float(c[2]), t_len=int(c[3]), n=int(c[4]), horizon=int(c[5]),
                freq=int(c[6]), env_seed=int(c[7]), n_opt=int(c[8]), term_reg=float(c[9]), ent_w=float(c[10]))


def test_fixture_holds_data_only_and_is_small():
    assert os.path.getsize(FIXTURE) < 256 * 1024 and os.path.getsize(RECORD) < 16 * 1024
    g = np.load(FIXTURE, allow_pickle=False)
    for tag in TAGS:
        c = _cfg(g, tag)
        t_len, n, n_opt = c["t_len"], c["n"], c["n_opt"]
        assert g[tag + "_states"].shape == (t_len + 1, n, 4) and g[tag + "_states"].dtype == np.float32
        assert g[tag + "_q"].shape == g[tag + "_beta"].shape == (t_len, n, n_opt) and g[tag + "_log_pi"].shape == (t_len, n, 2)
        assert g[tag + "_fresh_p"].shape == g[tag + "_continued_p"].shape == (t_len, n, n_opt)
        assert g[tag + "_action_draw_p"].shape == (t_len, n, 2)
        for name in ("option", "prev_option", "action", "init", "entropy", "reward", "mask", "ret", "advantage", "beta_advantage"):
            assert g[tag + "_" + name].shape == (t_len, n), name
        assert (g[tag + "_reward"] == 1.0).all() and (g[tag + "_init"][0] == 1).all() and (g[tag + "_prev_option"][0] == 1).all()
        assert np.all(np.diff(g[tag + "_eps"]) < 0) and g[tag + "_loss"].shape == (4,)
        init, target = _params(g, tag, "init"), _params(g, tag, "target")
        assert set(init) == set(target) == set(R.KEYS)
        assert all(not np.array_equal(init[k], target[k]) for k in R.KEYS if not k.endswith("bias"))      # the generator's next draws
    assert [_cfg(g, t)["n_opt"] for t in TAGS] == [2, 2, 3] and [_cfg(g, t)["freq"] for t in TAGS] == [200, 200, 2]
    c = _cfg(g, "t5n5")
    assert (c["t_len"], c["n"], c["horizon"]) == (5, 5, 200)
    for tag in ("t3n2", "t3n2_o3"):
        assert _cfg(g, tag)["horizon"] == 2 and (g[tag + "_mask"] == 0).any() and (g[tag + "_init"][1:] == 1).any()
        assert (g[tag + "_init"] == 0).any()


# ------------------------------------------------------------------------------------------ the restatement
def fixture_uniforms(g, tag):
    """The midpoint of every recorded draw's probability interval: [T, N, 3] float32 (fresh option, continued option, action)."""
    c = _cfg(g, tag)
    u = np.zeros((c["t_len"], c["n"], 3), dtype=np.float32)
    for j, name in enumerate(("fresh", "continued", "action_draw")):
        for t in range(c["t_len"]):
            for i in range(c["n"]):
                u[t, i, j] = R.midpoint(g["%s_%s_p" % (tag, name)][t, i], int(g["%s_%s" % (tag, name)][t, i]))
    return u


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_step(tag):
    """The restatement from the fixture's start (the task's seed, the initial online and target parameters, the recorded option
    epsilons, the midpoint uniforms of the draws the reference made): options, previous options, init flags, actions, masks and
    the float32 observations equal; the fp32 return scan equal to the bit from the reference's bootstrap; q, beta, log pi,
    entropy, the bootstrap, ret, advantage, beta_advantage and the four losses of the fp64 restatement within 1e-5 of each
    tensor's largest magnitude (floor 1: the reference ran in fp32); the parameters after the update within rtol 2e-5 / atol
    2e-6.  In the o3 tag the target copy fell inside the rollout: the bootstrap is the ONLINE network's."""
    g = np.load(FIXTURE)
    c = _cfg(g, tag)
    t_len, n = c["t_len"], c["n"]
    init, target = _params(g, tag, "init"), _params(g, tag, "target")
    boot_params = init if c["freq"] <= t_len else target
    envs, raw = K.make_envs(n, c["env_seed"], c["horizon"])
    roll = R.rollout(init, boot_params, envs, raw, t_len, g[tag + "_eps"], fixture_uniforms(g, tag), np.ones(n, dtype=np.int64),
                     np.ones(n, dtype=bool))
    for name in ("option", "prev_option", "action"):
        assert np.array_equal(roll[name], g[tag + "_" + name]), name
    assert np.array_equal(roll["init"], g[tag + "_init"]) and np.array_equal(roll["mask"], g[tag + "_mask"])
    assert np.array_equal(roll["state"], g[tag + "_states"][:t_len]) and np.array_equal(roll["bootstrap_state"], g[tag + "_states"][t_len])
    within = lambda got, want: np.abs(np.asarray(got, dtype=np.float64) - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    lg = roll["logits"]
    log_pi = lg - lg.max(-1, keepdims=True) - np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1, keepdims=True))
    assert within(roll["q"], g[tag + "_q"].astype(np.float64)) and within(roll["beta"], g[tag + "_beta"].astype(np.float64))
    assert within(log_pi, g[tag + "_log_pi"].astype(np.float64)) and within(roll["entropy"], g[tag + "_entropy"].astype(np.float64))
    assert within(np.take_along_axis(log_pi, roll["action"][..., None], axis=-1)[..., 0], roll["log_pi_a"])
    assert within(roll["bootstrap"], g[tag + "_bootstrap"].astype(np.float64))
    ret32 = R.returns(g[tag + "_reward"], g[tag + "_mask"], g[tag + "_bootstrap"], c["discount"], dtype=np.float32)
    assert ret32.dtype == np.float32 and np.array_equal(ret32, g[tag + "_ret"])
    new, keep = R.oc_update(init, roll, c["discount"], c["term_reg"], c["ent_w"], c["clip"], c["lr"])
    assert within(keep["ret"], g[tag + "_ret"].astype(np.float64)) and within(keep["adv"], g[tag + "_advantage"].astype(np.float64))
    assert within(keep["beta_adv"], g[tag + "_beta_advantage"].astype(np.float64))
    assert within(keep["loss"], g[tag + "_loss"].astype(np.float64))
    final = _params(g, tag, "final")
    assert set(final) == set(new)
    moved = 0
    for k in final:
        np.testing.assert_allclose(new[k], final[k], rtol=2e-5, atol=2e-6, err_msg=k)
        moved += int((final[k] != init[k]).sum())
    assert moved > 100          # the update moved the parameters: the comparison above is not of two copies of the start
    # bootstrapping from the WRONG network misses the reference's bootstrap
    wrong = R.rollout(init, target if boot_params is init else init, *K.make_envs(n, c["env_seed"], c["horizon"]), t_len,
                      g[tag + "_eps"], fixture_uniforms(g, tag), np.ones(n, dtype=np.int64), np.ones(n, dtype=bool))
    assert not within(wrong["bootstrap"], g[tag + "_bootstrap"].astype(np.float64))


def test_inverse_cdf_takes_the_recorded_draws_at_their_midpoints():
    g = np.load(FIXTURE)
    for tag in TAGS:
        for name in ("fresh", "continued", "action_draw"):
            p, k = g["%s_%s_p" % (tag, name)], g["%s_%s" % (tag, name)]
            for idx in np.ndindex(*k.shape):
                assert R.inv_cdf(p[idx].astype(np.float64), R.midpoint(p[idx], int(k[idx])))[0] == int(k[idx])


# ------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("case", K.ROLLOUT_CASES, ids=K.case_id)
def test_rollout_cases_have_margin_and_cover_their_edges(case):
    """No row needs excluding: the smallest gap between a uniform that decided an option or an action and a boundary of its CDF,
    and the smallest gap between a row's two largest option values (the greedy option), are >= 1e-4 in the fp64 restatement (fp32
    forwards differ from it by ~1e-6), and an fp32 run of the restatement makes the same option and action at every (step,
    environment).  Cases with 8 or more pairs take both option branches, keep and switch options and take both actions; the online
    and target parameters differ; the short-horizon cases end episodes inside the rollout (ring rows, init rows mid-rollout)."""
    hidden, gate, n, t_len, horizon, n_opt, padded, pseed, tseed, _ = case
    want, envs, start = K.restated_rollout(case)
    print("%s: margin %.3e, q gap %.3e, %d episodes ended" % (K.case_id(case), want["margin"], want["q_gap"], len(want["events"])))
    assert want["margin"] >= K.MARGIN and want["q_gap"] >= K.MARGIN and want["fp32_same_decisions"]
    assert [e.c for e in envs] == [t_len] * n
    assert pseed != tseed and not np.array_equal(start["params"]["fc_q.weight"], start["target"]["fc_q.weight"])
    assert want["option"].min() >= 0 and want["option"].max() < n_opt
    assert np.array_equal(want["prev_option"][0], start["prev_option"]) and np.array_equal(want["init"][0], start["is_initial"])
    assert np.array_equal(want["prev_option"][1:], want["option"][:-1]) and np.array_equal(want["init"][1:], 1.0 - want["mask"][:-1])
    if n * t_len >= 8:
        init, opt, prev = want["init"] > 0, want["option"], want["prev_option"]
        assert init.any() and (~init).any() and (~init & (opt != prev)).any() and (~init & (opt == prev)).any()
        assert set(np.unique(want["action"])) == {0, 1} and len(np.unique(opt)) == n_opt
    if horizon <= t_len:
        assert len(want["events"]) >= n * (t_len // horizon) and (want["mask"] == 0).sum() == len(want["events"])
        assert want["events"] == sorted(want["events"])                            # (step, environment) order
        assert (want["init"][1:] == 1).any()
    if horizon == 3:
        assert len(want["events"]) > K.RING_CAP - K.RING_COUNT0                     # the GPU test's short ring wraps
    # the bootstrap is the TARGET network's: the online parameters give another one
    qo, bo, _ = [v.numpy() for v in R.forward(R.to_t(start["params"]), want["bootstrap_state"], gate)]
    w, p = np.arange(n), want["prev_option_out"]
    online = (1 - bo[w, p]) * qo[w, p] + bo[w, p] * qo.max(axis=1)
    assert np.abs(online - want["bootstrap"]).max() > 1e-3


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_cases_cover_their_edges(case):
    """Relu cases keep every pre-activation of both hidden layers at least 1e-5 from zero (the fp32 kernel takes the derivative
    the fp64 restatement takes); the row counts are the ones the table states; the short-horizon case holds zero masks and init
    rows; the one-option case holds option 1 alone and the other options' head gradients are exactly zero."""
    hidden, gate, n, t_len, horizon, n_opt, one_option = case[:7]
    u = K.restated_update(case)
    print("%s: smallest |pre-activation| %.3e, losses %s" % (K.update_id(case), u["min_preact"], u["loss"]))
    if gate == "relu":
        assert u["min_preact"] >= K.PREACT_MARGIN
    inp = u["inputs"]
    assert inp["state"].shape == (t_len, n, 4) and inp["q"].shape == (t_len, n, n_opt) and n * t_len <= K.UPDATE_CAP
    assert all(inp[k].dtype == np.float32 for k in ("state", "q", "beta", "logits", "log_pi_a", "entropy", "init", "bootstrap"))
    if horizon <= t_len:
        assert (inp["mask"] == 0).any() and (inp["mask"] == 1).any() and len(u["events"]) > 0
        assert (inp["init"][1:] == 1).any() and (inp["init"] == 0).any()
    g = u["grads"]
    if one_option:
        o = K.FORCED_OPTION
        assert (inp["option"] == o).all() and (inp["prev_option"] == o).all()
        others = [j for j in range(n_opt) if j != o]
        assert not g["fc_q.weight"][others].any() and not g["fc_beta.weight"][others].any()
        assert not g["fc_pi.weight"].reshape(n_opt, 2, hidden)[others].any() and not g["fc_q.bias"][others].any()
        assert np.abs(g["fc_q.weight"][o]).max() > 1e-3 and np.abs(g["fc_pi.weight"].reshape(n_opt, 2, hidden)[o]).max() > 1e-4
        assert np.abs(g["fc_beta.weight"][o]).max() > 1e-5
    elif n * t_len >= 25:
        assert len(np.unique(inp["option"])) == n_opt and set(np.unique(inp["action"])) == {0, 1}
    assert set(g) == set(R.KEYS)
    assert all(np.isfinite(v).all() for v in g.values()) and np.isfinite(u["loss"]).all()
    assert abs(u["loss"][0] - (u["loss"][1] + u["loss"][2] + u["loss"][3])) < 1e-12


def test_update_cases_hold_the_stated_row_counts():
    rows = [c[2] * c[3] for c in K.UPDATE_CASES]
    assert rows == [1, 25, 51, 320, K.UPDATE_CAP, 32]


def test_restated_gradient_is_the_gradient_of_the_three_losses():
    """The restatement's autograd gradient against central differences of its own total loss (the detached terms held fixed), on
    the smallest tanh case: a few elements of every tensor."""
    case = K.UPDATE_CASES[2]
    u = K.restated_update(case)
    params = {k: np.asarray(v, dtype=np.float64) for k, v in u["params"].items()}
    rs = np.random.RandomState(0)
    for k in R.KEYS:
        for _ in range(2):
            idx = tuple(rs.randint(s) for s in params[k].shape)
            h = 1e-6
            side = []
            for sgn in (1, -1):
                p2 = {n: v.copy() for n, v in params.items()}
                p2[k][idx] += sgn * h
                side.append(R.loss_and_grads(p2, u["inputs"], u["eps"], K.DISCOUNT, K.TERM_REG, K.ENT_W, case[1])["loss"][0])
            num = (side[0] - side[1]) / (2 * h)
            assert abs(num - u["grads"][k][idx]) <= 1e-6 * max(1.0, abs(num)), (k, idx, num, u["grads"][k][idx])


# ------------------------------------------------------------------------------------------ C ABI mirrors, shapes
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_oc_mlp_net", "dra_oc_mlp_rollout_io", "dra_oc_mlp_update_io"])
def test_ctypes_mirror_matches_the_header(tmp_path, which):
    from deeprl_amd import oc_mlp
    from test_struct_layouts import _c_layout
    mirror = {"dra_oc_mlp_net": oc_mlp.Net, "dra_oc_mlp_rollout_io": oc_mlp.RolloutIO, "dra_oc_mlp_update_io": oc_mlp.UpdateIO}[which]
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, which, names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_supported_shapes():
    from deeprl_amd import oc_mlp, q_mlp
    ok = oc_mlp.supported
    assert ok(4, 2, 64, 5, 1, 2) and ok(4, 2, 16, 1, 1, 8) and ok(4, 2, 32, 64, 2, 3) and ok(4, 2, 64, 64, 1, 8)
    assert not ok(4, 2, 64, 5, 1, 1) and not ok(4, 2, 64, 5, 1, 9) and not ok(4, 2, 64, 5, 1, 0) and not ok(4, 2, 64, 5, 1, -1)
    for h in (8, 16, 32, 48, 64, 128):          # otherwise the shapes dra_q_mlp_supported takes
        for n in (0, 1, 5, 64, 65):
            for gate in (0, 1, 2, 3):
                assert ok(4, 2, h, n, gate, 2) == q_mlp.supported(4, 2, h, n, gate)
    assert not ok(5, 2, 64, 5, 1, 2) and not ok(4, 3, 64, 5, 1, 2)
    up = oc_mlp.update_supported
    assert up(4, 2, 64, 1, 1, 2) and up(4, 2, 16, 320, 2, 8) and up(4, 2, 32, K.UPDATE_CAP, 1, 4)
    assert all(up(4, 2, 64, 5 * n, 1, 2) for n in range(1, 65))        # every n_env the rollout takes at the example's T = 5
    assert not up(4, 2, 32, K.UPDATE_CAP + 1, 1, 2) and not up(4, 2, 32, 0, 1, 2) and not up(4, 2, 48, 25, 1, 2)
    assert not up(4, 2, 64, 25, 3, 2) and not up(4, 2, 64, 25, 1, 1) and not up(4, 2, 64, 25, 1, 9)
    assert not up(5, 2, 64, 25, 1, 2) and not up(4, 3, 64, 25, 1, 2)


def test_kernels_refuse_unsupported_shapes_before_any_launch():
    """dra_oc_mlp_rollout / dra_oc_mlp_update validate on the host: null pointers, negative offsets and shapes outside the table
    are DRA_EINVAL without a device."""
    from deeprl_amd import oc_mlp
    from deeprl_amd._lib import lib
    net, io, uo = oc_mlp.Net(), oc_mlp.RolloutIO(), oc_mlp.UpdateIO()
    assert lib.dra_oc_mlp_rollout.raw(None, ctypes.byref(io), None) == -22
    assert lib.dra_oc_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    assert lib.dra_oc_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22
    net.param = net.target = 4096
    net.state_dim, net.n_actions, net.hidden, net.gate, net.n_options = 4, 2, 48, 1, 2
    io.n_env, io.t_len, io.horizon, io.ring_cap = 5, 5, 200, 64
    assert lib.dra_oc_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    net.hidden = 64
    for f, _ in oc_mlp.RolloutIO._fields_[:25]:
        setattr(io, f, 4096)
    for bad in (1, 9):
        net.n_options = bad
        assert lib.dra_oc_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    net.n_options, net.wp = 2, -1
    assert lib.dra_oc_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    net.wp = 0
    uo.t_len, uo.n_env = 17, 64            # 1088 rows: above the cap, refused before the pointers are looked at
    for f, _ in oc_mlp.UpdateIO._fields_[:19]:
        setattr(uo, f, 4096)
    assert lib.dra_oc_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22
    uo.t_len, uo.n_env = 1 << 20, 1 << 20  # (a row count that overflows 32 bits)
    assert lib.dra_oc_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22
    uo.t_len, uo.n_env, net.bb = 5, 5, -3
    assert lib.dra_oc_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22
    net.bb, uo.eps = 0, None
    assert lib.dra_oc_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22


# ------------------------------------------------------------------------------------------ eligibility
class _Fused:
    def __init__(self, flat):
        self.flat = flat


class _Agent:
    """What oc_mlp.why_not reads of an OptionCriticAgent."""

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
    from deeprl_amd import oc_mlp
    d.select_device(-1)
    net = lambda *a, options=2, **k: d.OptionCriticNet(d.FCBody(4, *a, **k), 2, options)
    yes = lambda *a: True
    on = dict(fused_oc_feature=True)
    assert oc_mlp.why_not(_Agent(d, net(), net(), **on), yes) is None
    assert oc_mlp.why_not(_Agent(d, net(gate=torch.tanh, options=8), net(gate=torch.tanh, options=8), **on), yes) is None
    assert oc_mlp.why_not(_Agent(d, net(), net()), yes) == "config.fused_oc_feature is not on"                 # opt-in
    assert "not on" in oc_mlp.why_not(_Agent(d, net(), net(), fused_oc_feature=1), yes)
    assert oc_mlp.why_not(_Agent(d, net(options=1), net(options=1)), yes) == "config.fused_oc_feature is not on"
    a = _Agent(d, net(), net(), **on)
    a.grad_hook = lambda g: None
    assert oc_mlp.why_not(a, yes) == "a grad_hook is installed"
    assert "the network is not OptionCriticNet" in oc_mlp.why_not(_Agent(d, net((64, 64, 64)), net((64, 64, 64)), **on), yes)
    assert "the network is not OptionCriticNet" in oc_mlp.why_not(_Agent(d, net((64, 32)), net((64, 32)), **on), yes)
    assert "the network is not OptionCriticNet" in oc_mlp.why_not(_Agent(d, net(), net((32, 32)), **on), yes)
    assert "the network is not OptionCriticNet" in oc_mlp.why_not(_Agent(d, net(), net(options=3), **on), yes)
    vanilla = d.VanillaNet(2, d.FCBody(4))
    assert "the network is not OptionCriticNet" in oc_mlp.why_not(_Agent(d, vanilla, vanilla, **on), yes)
    assert "not built for 1 option " in oc_mlp.why_not(_Agent(d, net(options=1), net(options=1), **on), yes)
    assert "not built for 9 options" in oc_mlp.why_not(_Agent(d, net(options=9), net(options=9), **on), yes)
    assert "laid out differently" in oc_mlp.why_not(_Agent(d, net(), net(), target_order=[9, 8, 7, 6, 5, 4, 3, 2, 1, 0], **on), yes)
    a = _Agent(d, net(), net(), **on)
    a._fused.flat.params = a._fused.flat.params[:-1]
    assert "one optimiser does not own" in oc_mlp.why_not(a, yes)
    assert "not built for" in oc_mlp.why_not(_Agent(d, net(), net(), **on), lambda *s: False)
    assert "not built for" in oc_mlp.why_not(_Agent(d, net(), net(), num_workers=65, **on))
    assert "dra_oc_mlp_update is not built for 1280 rows" in oc_mlp.why_not(_Agent(d, net(), net(), num_workers=64, rollout_length=20, **on))
    assert oc_mlp.why_not(_Agent(d, net(), net(), num_workers=64, rollout_length=20, fused_oc_update=False, **on)) is None
    assert oc_mlp.shape(net()) == (4, 2, 64, 1, 2) and oc_mlp.shape(net((16, 16), gate=torch.tanh, options=3)) == (4, 2, 16, 2, 3)
    assert oc_mlp.shape(d.CategoricalActorCriticNet(4, 2, d.FCBody(4))) is None
    assert [f for f, _ in oc_mlp._fields(net())] == list(oc_mlp._OFFSETS)


def test_adoption_without_a_device_keeps_the_host_path():
    """Without a device the switch cannot move anything: OptionCriticAgent._adopt_feature leaves envs.Task in place and logs the
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
        cfg = zoo.config("option_critic_feature", game="classic-CartPole-v0", tag="oc_feat_host%d" % switch,
                         **(dict(fused_oc_feature=True) if switch else {}))
        agent = d.OptionCriticAgent.__new__(d.OptionCriticAgent)
        agent.config, agent.logger, agent.task = cfg, Rec(), cfg.task_fn()
        assert agent._adopt_feature() is None and type(agent.task) is d.Task and agent._feature is None
        assert len(warned) == int(switch)
    assert "stay on the host" in warned[0] and "no device" in warned[0]


def test_the_feature_methods_are_shared_not_copied():
    """NStepDQNAgent and OptionCriticAgent take the ring / drain / save / load / step methods from _TargetRolloutAgent."""
    import deeprl_amd as d
    from deeprl_amd.agents import _TargetRolloutAgent
    for name in ("close", "eval_episodes", "save", "load", "drain_episodes", "episodes", "_step_feature"):
        assert getattr(d.NStepDQNAgent, name) is getattr(d.OptionCriticAgent, name) is getattr(_TargetRolloutAgent, name), name
    assert d.NStepDQNAgent._feature_learn is not d.OptionCriticAgent._feature_learn
