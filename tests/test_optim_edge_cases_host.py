"""CPU proof that the inputs of tests/optim_edge_cases.py can carry the bar tests/test_gpu_optim_edges.py holds the optimizer
kernels to, and that every case reaches the path it is named for (runs everywhere, no GPU): a GPU failure there is then a
finding about a kernel, not about the test.

  noise floor  the float32 transcription of every step against the float64 reference stays within HALF the GPU bar (max-abs
               error over max |want64|) for the applied step and both states; printed next to the bar (pytest -s shows it)
  headroom     max |p| <= 80 max |step|: float32 rounding of the parameter (2^-24 |p|) stays under half the bar of the step
  centered     s - a^2 >= 1e-3 s on every element: no cancellation regime
  paths        the work decomposition recomputed from the launcher arithmetic of csrc/optim.hip (and, for the segmented
               launches, asked from the library's host-only planners) is the one each case names"""
import ctypes

import numpy as np
import pytest

import optim_edge_cases as E

HALF_BAR = 0.5 * E.BAR


def _ids(cases):
    return [c["name"] for c in cases]


def _floor(what, got32, want64):
    got32, want64 = np.asarray(got32, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    scale = np.abs(want64).max()
    assert scale > 0.0, what
    err = np.abs(got32 - want64).max() / scale
    assert err <= HALF_BAR, "%s: float32 transcription is %.3g of the scale away from float64 (half bar %.1g): change the inputs" % (
        what, err, HALF_BAR)
    return err


def _check_step(what, kind, p, g, s1, s2, sqsum, max_norm, t):
    """One step from float32 state: the three conditions above.  Returns the float32 transcription (the next step's state)."""
    w = E.ref_step(kind, p, g, s1, s2, sqsum, max_norm, t)
    f = E.f32_step(kind, p, g, s1, s2, sqsum, max_norm, t)
    errs = [_floor(what + " step", f["step"], w["step"]), _floor(what + " s1", f["s1"], w["s1"])]
    if w["s2"] is not None:
        errs.append(_floor(what + " s2", f["s2"], w["s2"]))
    ratio = np.abs(p).max() / np.abs(w["step"]).max()
    print("%-58s coef %.3g  fp32-vs-fp64 err/scale step %.3g s1 %.3g%s (half bar %.1g)  max|p|/max|step| %.3g" % (
        what, w["coef"], errs[0], errs[1], " s2 %.3g" % errs[2] if len(errs) > 2 else "", HALF_BAR, ratio))
    assert ratio <= 80.0, "%s: max |p| is %.3g x max |step|: float32 rounding of p would eat the bar" % (what, ratio)
    if E.KINDS[kind]["centered"]:
        assert np.all(w["s1"] - w["s2"] ** 2 >= 1e-3 * w["s1"]), what + ": centered RMSprop in its cancellation regime"
    assert abs(float(f["norm"]) - w["norm"]) <= 1e-6 * w["norm"] and abs(float(f["coef"]) - w["coef"]) <= 1e-6 * w["coef"]
    return f


def _zeros(n):
    return np.zeros(n, dtype=np.float32)


def _trajectory(c, grads, sqsums):
    p, s1, s2 = c["p0"], _zeros(c["n"]), _zeros(c["n"])
    coefs = []
    for k in range(E.STEPS):
        f = _check_step("%s step %d (scale %g)" % (c["name"], k, c["scales"][k]), c["kind"], p, grads[k], s1, s2, sqsums[k],
                        c["max_norm"], k + 1)
        p, s1, s2 = f["p"], f["s1"], s2 if f["s2"] is None else f["s2"]
        coefs.append(float(f["coef"]))
    assert min(coefs) < 1.0 and max(coefs) == 1.0, "%s: steps that clip AND steps that do not (%s)" % (c["name"], coefs)


# ------------------------------------------------------------------------------------------------------ noise floor
@pytest.mark.parametrize("c", E.step_cases() + E.adam_cases(), ids=_ids(E.step_cases() + E.adam_cases()))
def test_step_cases_carry_the_bar(c):
    assert sorted(c["scales"]) == sorted(E.SCALES) and len(c["grads"]) == E.STEPS
    _trajectory(c, c["grads"], [E.sqsum64(g) for g in c["grads"]])


@pytest.mark.parametrize("c", [c for c in E.step_cases() if c["kind"] == "adam"], ids=lambda c: c["name"])
def test_unclipped_adam_step_carries_the_bar(c):
    """test_adam_step_counter_without_partials: the first gradient, unclipped, as step t = 2 from zero state."""
    _check_step(c["name"] + " no partials", "adam", c["p0"], c["grads"][0], _zeros(c["n"]), _zeros(c["n"]), 1.0, 0.0, 2)


@pytest.mark.parametrize("c", E.coef_cases(), ids=_ids(E.coef_cases()))
def test_coef_cases_carry_the_bar(c):
    assert c["partials"].shape == (c["n_partials"],) and c["partials"].min() >= 1e-6 and c["partials"].max() <= 1e6
    assert c["n_partials"] == 1 or c["partials"].max() > 1e10 * c["partials"].min()      # drawn log-uniformly over twelve decades
    f = _check_step(c["name"], c["kind"], c["p0"], c["grad"], _zeros(c["n"]), _zeros(c["n"]), c["sqsum"], c["max_norm"], 1)
    assert float(f["coef"]) < 0.3                                     # the clipped run clips
    big = float(E.F(4.0 * np.sqrt(c["sqsum"])))                       # a norm below max_norm: the coefficient clamps to 1
    assert float(E.f32_step(c["kind"], c["p0"], c["grad"], _zeros(c["n"]), _zeros(c["n"]), c["sqsum"], big, 1)["coef"]) == 1.0
    _check_step(c["name"] + " unclipped", c["kind"], c["p0"], c["grad"], _zeros(c["n"]), _zeros(c["n"]), c["sqsum"], 0.0, 1)


@pytest.mark.parametrize("layout", E.SEGS_LAYOUTS, ids=_ids(E.SEGS_LAYOUTS))
def test_segs_cases_carry_the_bar(layout):
    c = E.segs_case(layout)
    f = _check_step(c["name"], c["kind"], c["p0"], c["want"], _zeros(c["n"]), _zeros(c["n"]), E.sqsum64(c["want"]), c["max_norm"], 1)
    assert float(f["coef"]) < 1.0
    assert np.all(np.isfinite(c["want"]))                             # no NaN of the padding reaches the fold
    for sl, cnt in zip(c["seg_slabs"], c["counts"]):
        assert sl.shape[1] == cnt + c["pad"] and np.all(np.isnan(sl[:, cnt:])) and np.all(np.isfinite(sl[:, :cnt]))


@pytest.mark.parametrize("c", E.late_cases(), ids=_ids(E.late_cases()))
def test_late_cases_carry_the_bar(c):
    steps = [E.late_step_inputs(c, k) for k in range(E.STEPS)]
    for st in steps:
        assert np.all(np.isfinite(st["grad"])) and st["grad"].shape == (c["n"],) and np.all(st["prior"] >= 0.0)
        assert np.all(np.isnan(st["slabs"][:, c["count"]:]))
    _trajectory(c, [st["grad"] for st in steps], [st["sqsum"] for st in steps])


# ------------------------------------------------------------------------------------------------------------ paths
@pytest.mark.parametrize("c", E.step_cases(), ids=_ids(E.step_cases()))
def test_step_cases_reach_their_paths(c):
    got = E.step_path(c["n"])
    print("%-28s %s" % (c["name"], got))
    assert got == c["expect"]


def test_step_shapes_cover_every_path_of_the_two_slot_kernels():
    paths = [E.step_path(n) for n, _ in E.STEP_SHAPES]
    assert any(p["last_slot1"] == 1 for p in paths) and any(p["last_slot1"] == 256 for p in paths)      # slot v = 1: first, full
    assert any(p["blocks"] == 2 and p["last_slot0"] == 1 for p in paths)                                # a second workgroup of one float4
    assert any(p["blocks"] > 2 and p["tail"] for p in paths)                                            # a tail with several workgroups
    assert any(p["blocks"] == 1 and p["last_slot0"] == 256 and not p["last_slot1"] and p["tail"] for p in paths)
    assert min(n for n, _ in E.STEP_SHAPES) == 4


@pytest.mark.parametrize("c", E.adam_cases(), ids=_ids(E.adam_cases()))
def test_adam_cases_reach_their_paths(c):
    got = E.adam_path(c["n"])
    print("%-28s %s" % (c["name"], got))
    assert got == c["expect"]
    assert c["n"] <= 2048 * 256 or got["trips"] == 2


@pytest.mark.parametrize("c", E.sqnorm_cases(), ids=_ids(E.sqnorm_cases()))
def test_sqnorm_cases_reach_their_paths(c):
    got = E.sqnorm_path(c["n"])
    print("%-28s %s" % (c["name"], got))
    assert got == c["expect"]
    assert c["stride"] > c["n"] and c["stride"] % 4 == 0
    if c["n_slabs"]:
        assert c["slabs"].shape == (c["n_slabs"], c["stride"]) and np.all(np.isnan(c["slabs"][:, c["n"]:]))


def test_coef_cases_cover_the_reduction_shapes():
    """16 straight-line loads per thread at 256 threads: one entry, the last thread of the first load, the first of the
    second, two full loads (dra_grad_sqnorm's count), and the maximum with and without its last entry."""
    assert E.COEF_PARTIALS == (1, 255, 256, 257, 512, 4095, 4096) and E.step_path(E.COEF_N)["blocks"] == 2


class _T:                                    # a fake 16-byte aligned "tensor": the planners only validate pointers
    def __init__(self, addr=0x10000):
        self._a = addr

    def data_ptr(self):
        return self._a


@pytest.mark.parametrize("layout", E.SEGS_LAYOUTS, ids=_ids(E.SEGS_LAYOUTS))
def test_segs_layouts_reach_their_paths(layout):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib
    got = E.segs_path(layout["counts"], layout["slabs"], layout["tail"])
    print("%-24s %s" % (layout["name"], got))
    assert got == layout["expect"]
    segs, off = [], 0
    for cnt, ns in zip(layout["counts"], layout["slabs"]):
        segs.append((off, cnt, _T(), cnt + layout["pad"], ns))
        off += cnt
    b = ctypes.c_int(0)
    rc = lib.dra_grad_sqnorm_segs_blocks.raw(off + layout["tail"], ops._fold_seg_array(segs), len(segs), ctypes.byref(b))
    assert rc == 0 and b.value == layout["expect"]["partials"]


def test_plain_two_strides_layout_is_the_one_the_issue_names():
    e = [l for l in E.SEGS_LAYOUTS if l["name"] == "plain-two-strides"][0]["expect"]
    assert (e["fold_blocks"], e["plain_blocks"], e["plain_iters"], e["partials"]) == (4000, 49, 2, 4049)


@pytest.mark.parametrize("c", E.late_cases(), ids=_ids(E.late_cases()))
def test_late_cases_reach_their_paths(c):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib
    got = E.late_path(c["count"], c["n_slabs"], c["n"])
    print("%-52s %s" % (c["name"], got))
    assert got == c["expect"]
    b = ctypes.c_int(0)
    rc = lib.dra_clip_step_late_blocks.raw(ops._fold_seg_array([(0, c["count"], _T(), c["stride"], c["n_slabs"])]), ctypes.byref(b))
    assert rc == 0 and b.value == c["expect"]["fold_blocks"]
    assert c["n_prior"] + b.value <= 4096 and c["stride"] % 4 == 0 and c["stride"] >= c["count"]


def test_late_cases_cover_what_they_promise():
    cs = E.late_cases()
    inst = {(E.KINDS[c["kind"]]["opt"], c["expect"]["ng"], 16 if c["n_prior"] > 1024 else 4) for c in cs}
    assert inst == {(o, ng, npt) for o in ("rmsprop", "adam") for ng in (4, 16) for npt in (4, 16)}, inst
    for kind in ("rmsprop_centered", "rmsprop_plain"):       # both RMSprop forms at both group counts
        assert {c["expect"]["ng"] for c in cs if c["kind"] == kind} == {4, 16}
    assert {(c["count"], c["n_slabs"]) for c in cs} == set(E.LATE_SEGS)
    assert {c["extra"] for c in cs} == set(E.LATE_EXTRA) == {0, 3, 3079}
    priors = {c["n_prior"] for c in cs}
    assert {0, 1, 1024, 1025} <= priors and any(c["n_prior"] + c["expect"]["fold_blocks"] == 4096 for c in cs)
    assert any(c["expect"]["fold_blocks"] == 256 for c in cs)                                   # thread 255 polls
    assert any(c["extra"] == 3 and c["expect"]["plain_blocks"] == 0 for c in cs)                # a fold workgroup steps the tail
    for ng in (4, 16):                                                                          # ... and a plain one, per fold form
        assert any(c["expect"]["ng"] == ng and c["expect"]["plain_blocks"] == 2 and c["expect"]["tail"] for c in cs)
    assert any(c["stride"] > c["count"] for c in cs) and any(c["stride"] == c["count"] for c in cs)


# -------------------------------------------------------------------------------------------------------- references
def test_fold_orders_differ_and_agree_with_float64():
    """The two fold orders are different float32 sums of the same slabs (so a bit-exact comparison tells them apart) and
    both are float32-close to the float64 sum."""
    rs = np.random.RandomState(11)
    sl = rs.standard_normal((64, 4096)).astype(np.float32)
    a, b, c = E.fold_grouped(sl, 16), E.fold_grouped(sl, 4), E.fold_in_order(sl)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    rev = E.fold_grouped(sl[[s for g in range(3, -1, -1) for s in range(g, 64, 4)]], 16)
    assert a.dtype == np.float32 and rev.dtype == np.float32
    want = sl.astype(np.float64).sum(0)
    for x in (a, b, c):
        np.testing.assert_allclose(x, want, rtol=0, atol=2e-5)
    one = E.fold_grouped(sl[:1], 16)
    assert np.array_equal(one, sl[0])


def test_references_agree_with_torch_optimizers():
    """ref_step against torch.optim.RMSprop / Adam in float64 over three clipped steps (clip_grad_norm_'s coefficient)."""
    import torch
    rs = np.random.RandomState(3)
    n = 257
    for kind, hp in E.KINDS.items():
        h = E.hyper(kind)
        p = torch.tensor((rs.standard_normal(n) * 0.1).astype(np.float32), dtype=torch.float64, requires_grad=True)
        if hp["opt"] == "rmsprop":
            opt = torch.optim.RMSprop([p], lr=float(h["lr"]), alpha=float(h["alpha"]), eps=float(h["eps"]), centered=hp["centered"])
        else:
            opt = torch.optim.Adam([p], lr=float(h["lr"]), betas=(float(h["beta1"]), float(h["beta2"])), eps=float(h["eps"]))
        s1, s2 = np.zeros(n), np.zeros(n)
        mine = p.detach().numpy().copy()
        for t in range(1, 4):
            g = rs.standard_normal(n).astype(np.float32)
            p.grad = torch.tensor(g, dtype=torch.float64)
            torch.nn.utils.clip_grad_norm_([p], 2.0)
            opt.step()
            w = E.ref_formulas(kind, g.astype(np.float64), s1, s2, E.sqsum64(g), 2.0, t)     # float64 states stay float64
            mine, s1, s2 = mine - w["step"], w["s1"], s2 if w["s2"] is None else w["s2"]
            np.testing.assert_allclose(mine, p.detach().numpy(), rtol=0, atol=1e-12)
