"""CPU proof of the tables in tests/policy_head_edge_cases.py: every case reaches what it is named for under the restated dispatch,
the tables together cover COVERAGE, the integer set stays exact, the float32 CPU run of every reference is within the bar, every
sampling row is strict or clear of the CDF boundaries, the fold transcription agrees with float64, the reference on clamped
actions is torch.distributions.Categorical's, and the restated limits are the ones in the sources."""
import os
import re

import numpy as np
import pytest
import torch

import policy_head_edge_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deeprl_amd", "csrc")


def _ids(cases):
    return [c["name"] for c in cases]


def _src(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _fig(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


_WORST = {}


def _within_bar(name, key, got32, want64):
    f = _fig(got32, want64)
    _WORST[(name, key)] = f
    print("policy head cases %s %s: float32 CPU err/scale %.3g" % (name, key, f))
    assert f <= E.bar(name, key), "%s %s: the float32 CPU run misses the bar (%.3g): the inputs cannot carry it" % (name, key, f)


# ------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("c", [c for c in E.ALL_CASES if "reaches" in c], ids=_ids([c for c in E.ALL_CASES if "reaches" in c]))
def test_every_case_reaches_what_it_names(c):
    d = E.dispatch_of(c)
    if isinstance(d, tuple):
        assert d == c["reaches"], (c["name"], d)
        return
    assert c["reaches"], c["name"] + " names nothing"
    for k, v in c["reaches"].items():
        assert d[k] == v, "%s: %s is %r under the restated dispatch, the case says %r" % (c["name"], k, d[k], v)


@pytest.mark.parametrize("item", sorted(E.COVERAGE))
def test_the_tables_cover(item):
    assert E.COVERAGE[item](), item


def test_restatements_at_the_values_the_issue_names():
    """The restated dispatch itself, at hand-checked values (so that an edit of a restatement and of a case together shows)."""
    assert E.fwd_dispatch(5, 65, 15, 1) == dict(wgs=2, last_rows=1, kregs=2, ktail=1, groups=2, last_group=8, straddle=True)
    assert E.fwd_dispatch(33, 512, 64, 1)["groups"] == 9 and E.fwd_dispatch(33, 512, 64, 1)["last_group"] == 1
    assert [E.bwd_dispatch(b, 8, 2, 1)["rounds"] for b in (8, 40, 47, 257)] == [(0, 1, 0), (1, 1, 0), (1, 1, 7), (8, 0, 1)]
    assert [E.bwd_dispatch(1, k, 2, 1)["halves"] for k in (1, 255, 256, 257, 512)] == [(1, 0), (255, 0), (256, 0), (256, 1), (256, 256)]
    assert E.bwd_dispatch(257, 8, 2, 1)["trips"] == 2 and E.bwd_dispatch(256, 8, 2, 1)["trips"] == 1
    assert [E.riding_dispatch(b, "plain")["waves"] for b in (16, 17)] == [8, 4]
    assert E.head_path(512, 64, 8192, True, True) == ("policy_head_fn", "policy_head_fn")
    assert E.head_path(512, 64, 8193, True, True) == ("linear_pair_fn", "categorical_policy")
    assert E.head_path(513, 64, 5, False, False) == ("separate", "categorical_policy")
    assert E.head_path(512, 65, 5, False, False) == ("linear_fwd_pair", "torch")
    assert E.head_path(512, 64, 5, True, False) == ("linear_pair_fn", "categorical_policy")
    assert E.head_path(512, 64, 5, False, False) == ("sample", "sample")


def test_integer_operands_stay_exact():
    for c in E.FWD_CASES + [c for c in E.BWD_CASES if c["kind"] == "bwd_pair"]:
        assert E.int_bound(c) < 2 ** 24, c["name"]
    op = E.fwd_operands("fwd_pair-5x65x70+2", "integer")
    for k in ("x", "w0", "w1", "b0", "b1"):
        assert np.array_equal(op[k], np.round(op[k])) and np.abs(op[k]).max() <= 4
    assert np.array_equal(op["y0"], np.round(op["y0"])) and np.abs(op["y0"]).max() <= E.int_bound(E.by_name("fwd_pair-5x65x70+2"))


# ------------------------------------------------------------------------------------------------ float32 CPU yardstick
@pytest.mark.parametrize("c", E.FWD_CASES, ids=_ids(E.FWD_CASES))
def test_forward_inputs_carry_the_bar(c):
    op = E.fwd_operands(c["name"], "random")
    y0, y1 = E.heads_ref(op["x"], op["w0"], op["b0"], op["w1"], op["b1"], op["act"], dtype=E.F)
    assert y0.dtype == E.F
    _within_bar(c["name"], "y0", y0, op["y0"])
    _within_bar(c["name"], "y1", y1, op["y1"])
    for k in ("y0", "y1"):      # no tensor's scale is a cancelled sum (E._anchor)
        assert np.abs(op[k]).max() >= E.MIN_SCALE, "%s: max |%s| is %.3g" % (c["name"], k, np.abs(op[k]).max())
    if c["kind"] != "fwd_pair":
        r = E.head_ref(y0, None, op["action"], dtype=E.F)
        _within_bar(c["name"], "log_pi_a", r["log_pi_a"], op["lp_given"])
        _within_bar(c["name"], "entropy", r["entropy"], op["ent"])
        _rows_clear(c["name"], op, op["y0"])


def _rows_clear(name, op, logits64):
    """Every row strict or clear of every CDF boundary by the threshold: no exempt row."""
    thr = E.cdf_threshold(logits64)
    strict = op["u"] >= 1.0
    ok = strict | (op["margin"] >= thr)
    assert ok.all(), "%s: rows %s fall under the margin %.3g (smallest %.3g)" % (name, np.nonzero(~ok)[0][:8], thr, op["margin"][~ok].min())
    assert strict.any() or "riding" in name and len(strict) == 0
    A = op["p"].shape[1]
    assert np.all(op["sampled"][strict] == A - 1)


@pytest.mark.parametrize("c", E.FOLD_CASES, ids=_ids(E.FOLD_CASES))
def test_fold_transcription_and_inputs(c):
    op = E.fold_operands(c["name"])
    phi64 = E.fold_ref(op["slabs"], op["bias"])
    _within_bar(c["name"], "phi", op["phi"], phi64)
    pre = op["pre"]
    bits = pre.view(np.uint32)
    assert np.all(bits[:, 0:4] == 0) and np.all(bits[:, 4:8] == 0x80000000), "the exact +0 and -0.0 sums are not there"
    assert np.all(op["phi"].view(np.uint32)[:, 0:8] == 0), "relu of a zero of either sign is +0"
    neg = float((pre[:, 8:] < 0).mean())
    assert 0.35 < neg < 0.65, neg
    logits, v = E.heads_ref(op["phi"], op["w0"], op["b0"], op["w1"], op["b1"], dtype=E.F)
    _within_bar(c["name"], "logits", logits, op["logits"])
    _within_bar(c["name"], "v", v[:, 0], op["v"])
    assert np.abs(op["logits"]).max() >= E.MIN_SCALE and np.abs(op["v"]).max() >= E.MIN_SCALE
    r = E.head_ref(logits, None, op["action"], dtype=E.F)
    _within_bar(c["name"], "log_pi_a", r["log_pi_a"], op["lp_given"])
    _within_bar(c["name"], "entropy", r["entropy"], op["ent"])
    _rows_clear(c["name"], op, op["logits"])


@pytest.mark.parametrize("c", E.BWD_CASES, ids=_ids(E.BWD_CASES))
def test_backward_inputs_carry_the_bar(c):
    op = E.bwd_operands(c["name"], "random")
    if c["kind"] == "bwd_pair":
        got = E.pair_bwd_ref(op["g0"], op["g1"], op["x"], op["w0"], op["w1"], dtype=E.F)
    else:
        got = E.heads_bwd_ref(op["logits"], op["action"], op["g_lp"], op["g_ent"], op["g_v"], op["x"], op["w0"], op["w1"], c["relu"], dtype=E.F)
    w = op["want"]
    for k in ("dx", "dw0", "db0", "dw1", "db1"):
        assert got[k].dtype == E.F
        _within_bar(c["name"], k, got[k], w[k])
    if "g_v" not in c["null"] and c["B"] >= 256:      # the one-number tensor of a long sum is no cancelled sum (E.G_MEAN)
        assert abs(float(w["db1"].sum())) >= 0.25 * c["B"] * c["O1"] * E.G_MEAN, (c["name"], w["db1"])
    if c["kind"] == "heads_bwd":
        if c["A"] == 1 or {"g_lp", "g_ent"} <= set(c["null"]):
            assert not w["dlogits"].any() and not w["dw0"].any() and not w["db0"].any(), "float64 says exactly zero here"
        if "g_v" in c["null"]:
            assert not w["dw1"].any() and not w["db1"].any()
        if c["relu"]:
            x = op["x"]
            assert (x == 0).mean() > 0.3 and (np.signbit(x) & (x == 0)).any(), "the features carry +0 and -0.0"
            assert not w["dx"][x <= 0].any()


@pytest.mark.parametrize("c", E.OOR_CASES, ids=_ids(E.OOR_CASES))
def test_out_of_range_cases_hold_all_three_values(c):
    op = E.oor_operands(c["name"])
    a, A = op["action"], c["A"]
    assert (a == -1).any() and (a == A).any() and (a == 2 ** 40).any()
    assert ((a < 0) | (a >= A)).sum() == (c["B"] + 10) // 11
    # the reference on clamped actions is torch.distributions.Categorical's in float64
    logits = torch.tensor(op["logits"], dtype=torch.float64, requires_grad=True)
    dist = torch.distributions.Categorical(logits=logits)
    lp, ent = dist.log_prob(torch.from_numpy(E.clamp_action(a, A))), dist.entropy()
    (lp * torch.tensor(op["g_lp"], dtype=torch.float64) + ent * torch.tensor(op["g_ent"], dtype=torch.float64)).sum().backward()
    np.testing.assert_allclose(op["lp"], lp.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(op["ent"], ent.detach().numpy(), rtol=0, atol=1e-12)
    dl = op["dlogits"] if c["kind"] == "categorical" else op["bwd"](op["logits"])["dlogits"]
    np.testing.assert_allclose(dl, logits.grad.numpy(), rtol=0, atol=1e-12)
    r32 = E.head_ref(op["logits"], None, a, (op["g_lp"], op["g_ent"]), dtype=E.F)
    _within_bar(c["name"], "log_pi_a", r32["log_pi_a"], op["lp"])
    _within_bar(c["name"], "dlogits", r32["dlogits"], dl)


@pytest.mark.parametrize("c", E.SAMPLING_CASES, ids=_ids(E.SAMPLING_CASES))
def test_sampling_rows(c):
    op = E.sampling_operands(c["name"])
    lg, u = E.sampling_rows()
    assert {0.0, float(E.U_BELOW_ONE), 1.0} <= set(float(v) for v in u)
    assert np.all(np.sort(lg[:4], axis=1)[:, -1] - np.sort(lg[:4], axis=1)[:, -2] > 45), "rows 0-3: one logit 50 above the rest"
    assert np.all(lg[4:8] == lg[4:8, :1]), "rows 4-7: all logits equal"
    assert lg.min() >= 0
    _rows_clear(c["name"], op, op["logits"])
    # what the edge uniforms must give: u = 0 the first action with mass, 1 - 2^-24 the last action where it holds the mass
    assert list(op["sampled"][[0, 1, 2, 3]]) == [0, 63, 63, 42] and list(op["sampled"][[4, 5, 6, 7]]) == [0, 63, 63, 32]
    assert list(op["sampled"][[8, 9, 10]]) == [0, 63, 63]


@pytest.mark.parametrize("c", E.RIDING_CASES, ids=_ids(E.RIDING_CASES))
def test_riding_inputs(c):
    op = E.riding_operands(c["name"])
    assert op["frames"].dtype == np.uint8 and op["frames"].shape == (c["B"], 4, 84, 84)
    if c["mode"] == "none":
        return
    logits, v = E.heads_ref(op["phi"], op["w0"], op["b0"], op["w1"], op["b1"], dtype=E.F)
    _within_bar(c["name"], "logits", logits, op["logits"])
    _within_bar(c["name"], "v", v[:, 0], op["v"])
    assert np.abs(op["logits"]).max() >= E.MIN_SCALE and np.abs(op["v"]).max() >= E.MIN_SCALE
    _rows_clear(c["name"], op, op["logits"])
    if c["mode"] != "plain":
        _within_bar(c["name"], "phi", op["phi_fold"], E.fold_ref(op["slabs"], op["bias"]))


@pytest.mark.parametrize("c", E.FC4_CASES, ids=_ids(E.FC4_CASES))
def test_fc4_head_inputs_carry_the_bar(c):
    op = E.fc4_operands(c["name"])
    r32 = E.fc4_ref(op, dtype=E.F)
    for k, want in op["want"].items():
        _within_bar(c["name"], k, r32[k], want)
    assert np.abs(op["want"]["v"]).max() >= E.MIN_SCALE and 0.3 < (op["want"]["phi"] == 0).mean() < 0.7


@pytest.mark.parametrize("c", E.NET_CASES, ids=_ids(E.NET_CASES))
def test_net_inputs(c):
    op = E.net_operands(c["name"])
    assert op["relu_margin"] >= E.RELU_MARGIN, "%s: a ReLU pre-activation %.3g from zero" % (c["name"], op["relu_margin"])
    _rows_clear(c["name"], op, op["logits"])
    r32, r64 = E.net_ref(op, c, op["action"], dtype=torch.float32), E.net_ref(op, c, op["action"])
    for k in ("log_pi_a", "entropy", "v", "dx", "dwb", "dbb", "dwa", "dba", "dwc", "dbc"):
        _within_bar(c["name"], k, r32[k], r64[k])


def test_zz_the_largest_float32_figure_is_the_one_in_the_docstring():
    """(runs last in this module: the figure the case file's docstring quotes is the largest one measured above)"""
    assert not E.BAR_OVERRIDES
    if not _WORST:      # (the per-case tests did not run in this process)
        return
    (name, key), worst = max(_WORST.items(), key=lambda kv: kv[1])
    print("largest float32 CPU figure: %.3g (%s %s)" % (worst, name, key))
    assert worst <= E.BAR and not E.BAR_OVERRIDES


# ------------------------------------------------------------------------------------------------------------ limits
def test_restated_limits_are_the_sources():
    from deeprl_amd import ops
    assert E.HEADS_BWD_MAX_BATCH == ops.HEADS_BWD_MAX_BATCH
    ig = _src(CSRC, "igemm.hip")
    assert re.search(r"constexpr int kHeadsBwdMaxBatch = %d;" % E.HEADS_BWD_MAX_BATCH, ig)
    lim = r"batch < 1 \|\|\s*batch > %d \|\|\s*in_features < 1 \|\| in_features > %d \|\| n_actions < 1 \|\| n_actions > %d" % (
        E.MAX_FWD_BATCH, E.MAX_K, E.MAX_A)
    assert len(re.findall(lim, ig)) == 2, "dra_policy_heads_sample / _given (igemm.hip:296-297, 311-312)"
    assert len(re.findall(r"batch < 1 \|\|\s*batch > %d \|\| n_actions < 1 \|\| n_actions > %d" % (E.MAX_FWD_BATCH, E.MAX_A), ig)) == 2, \
        "dra_policy_heads_given_fold / _sample_fold28 (igemm.hip:328-329, 349-350)"
    assert re.search(r"batch < 1 \|\| batch > %d \|\| in_features < 1 \|\| in_features > %d \|\| out0 < 1 \|\| out1 < 1" % (
        E.MAX_FWD_BATCH, E.MAX_K), ig), "dra_linear_fwd_pair (igemm.hip:463)"
    assert re.search(r"batch < 1 \|\| batch > kHeadsBwdMaxBatch \|\|\s*in_features < 1 \|\| in_features > %d \|\| n_actions < 1 \|\| n_actions > %d" % (
        E.MAX_K, E.MAX_A), ig), "dra_policy_heads_bwd (igemm.hip:451-452)"
    assert re.search(r"n_slabs != %d && n_slabs != %d" % E.GIVEN_FOLD_SLICES, ig), "dra_policy_heads_given_fold (igemm.hip:328)"
    assert "policy_heads_foldwg_kernel<%d>" % E.ROLLOUT_SLICES in ig, "dra_policy_heads_sample_fold28 (igemm.hip:355)"
    cv = _src(CSRC, "conv_v2.hip")
    assert re.search(r"constexpr int kConvNw8MaxBatch = %d;" % E.NW8_MAX_BATCH, cv), "conv_v2.hip:1638"
    assert re.search(r"!y1 \|\| batch < 1 \|\| batch > %d\) return DRA_EINVAL" % E.RIDING_MAX_BATCH, cv), "conv_v2.hip:1855"
    assert "policy_head_row_fold_wg<%d>(h, (int)blockIdx.x, s_phi, s_out[0])" % E.ROLLOUT_SLICES in cv, "conv_v2.hip:1826"
    rr = _src(CSRC, "rollout_roles.h")
    assert "const int o = min(oc + u, OT - 1);" in rr and "for (int oc = 0; oc < OT; oc += 8)" in rr, "rollout_roles.h:26-30"
    assert "const int k0 = t, k1 = t + 256;" in ig, "igemm.hip:388, 486"
    nets = _src(ROOT, "deeprl_amd", "nets.py")
    assert "phi_a.shape[1] <= %d and phi_a.shape[0] <= %d" % (E.MAX_K, E.MAX_FWD_BATCH) in nets, "nets.py:1242"
    assert "phi_a.shape[0] <= ops.HEADS_BWD_MAX_BATCH" in nets, "nets.py:1256"
    assert nets.count("self.fc_action.weight.shape[0] <= %d" % E.MAX_A) >= 3 and "logits.shape[-1] <= %d" % E.MAX_A in nets
