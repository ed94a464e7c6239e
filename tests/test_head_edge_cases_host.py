"""CPU proof that the inputs of tests/head_edge_cases.py can carry the bar tests/test_gpu_head_edges.py holds the n-step,
option-critic, noisy-layer, dueling and PER kernels to, and that every case reaches the path it is named for (runs everywhere,
no GPU): a GPU failure there is then a finding about a kernel, not about the test.

  noise floor  the float32 transcription of the kernel's summation order stays within HALF the GPU bar (max-abs error over
               max |want64| per output tensor) of the float64 reference, and is exactly zero where float64 is.  (The noisy
               layer's y and dx use one accumulator per output, an order no better than the kernels' split sums; the Gaussian
               head computes in float64 and rounds once, so it has no float32 order to transcribe.)
  paths        list lengths, trip counts, ragged last workgroups, the split plans of csrc/noisy.hip restated in Python (and asked
               from the library where it loads), which of the vector / scalar kernels a shape and an alignment select
  decisions    the discrete outputs of the rollout heads: no row of a case sits within the margin a GPU test may leave out"""
import ctypes

import numpy as np
import pytest

import head_edge_cases as H

HALF_BAR = 0.5 * H.BAR


def _ids(cases):
    return [c["name"] for c in cases]


def _floor(what, got32, want64):
    """err / scale of one output tensor, held to half the bar; zero where float64 says zero."""
    got32, want64 = np.asarray(got32, dtype=np.float64).reshape(np.shape(want64)), np.asarray(want64, dtype=np.float64)
    scale = np.abs(want64).max() if want64.size else 0.0
    if scale == 0.0:
        assert np.all(got32 == 0.0), "%s: float64 says exactly zero, the float32 transcription does not" % what
        return 0.0
    err = np.abs(got32 - want64).max() / scale
    assert err <= HALF_BAR, "%s: float32 transcription is %.3g of the scale away from float64 (half bar %.1g)" % (what, err, HALF_BAR)
    return err


def _floors(name, f32, ref, keys=None):
    errs = {k: _floor("%s %s" % (name, k), f32[k], ref[k]) for k in (keys or ref)}
    print("%-34s fp32-vs-fp64 err/scale (half bar %.1g): %s" % (name, HALF_BAR, "  ".join("%s %.2g" % kv for kv in errs.items())))
    return errs


# ------------------------------------------------------------------------------------------------ dra_nstep_q_loss_bwd
@pytest.mark.parametrize("c", H.nstep_cases(), ids=_ids(H.nstep_cases()))
def test_nstep_cases_carry_the_bar(c):
    ref = H.nstep_ref(c)
    _floors(c["name"], H.nstep_f32(c), ref)
    assert np.all(ref["dphi"][c["phi"] == 0] == 0) and np.any(np.signbit(c["phi"]) & (c["phi"] == 0)) and np.any(c["phi"] > 0)
    if c["unused"] is not None:
        assert not ref["dw"][c["unused"]].any() and ref["db"][c["unused"]] == 0 and ref["dw"].any()


@pytest.mark.parametrize("shape", [s for s, v in H.NSTEP_VARIANTS if v == "one-action"], ids=lambda s: "T%d-N%d-A%d" % s)
def test_nstep_tree_sum_stays_inside_its_error_bound(shape):
    """All rows on one action: db is a mean of differences of both signs, far smaller than the sum of their magnitudes, so the
    summation order decides its error.  At most 7 + 15 + 15 additions lie between a term and the result of the kernel's tree,
    which bounds the error by 37 u sum |g| (u = 2^-24; the standard bound of a summation tree by its depth), whatever the
    terms; one running sum over 2048 rows has 2047 u."""
    c = H.nstep_case(shape, "one-action")
    rows = c["R"]
    ret = H._returns(c["reward"], c["mask"], c["boot"], c["gamma"], np.float32).reshape(-1)
    g = (c["q"].reshape(rows, c["A"])[:, -1] - ret) / np.float32(rows)
    exact, mag = g.astype(np.float64).sum(), np.abs(g.astype(np.float64)).sum()
    err = abs(float(H._tree(g)) - exact)
    print("%s: sum |g| / |db| = %.0f, tree error %.2g u sum |g|" % (c["name"], mag / abs(exact), err / (2.0 ** -24 * mag)))
    assert err <= 37 * 2.0 ** -24 * mag and mag > 20 * abs(exact)
    assert rows == 2048 and H.NSTEP_SUM_SPANS == (8, 128) and (8 - 1) + (128 // 8 - 1) + (2048 // 128 - 1) == 37


def test_nstep_cases_reach_their_paths():
    cases = {c["name"]: c for c in H.nstep_cases()}
    assert [(c["T"], c["N"], c["A"]) for c in H.nstep_cases()[:len(H.NSTEP_SHAPES)]] == H.NSTEP_SHAPES
    paths = {k: H.nstep_path(c) for k, c in cases.items()}
    assert max(c["R"] for c in cases.values()) == 2048 and {c["A"] for c in cases.values()} >= {1, 64}
    assert paths["T1-N257-A4-plain"]["env_trips"] == 2 and paths["T1-N2048-A64-plain"]["env_trips"] == 8
    assert paths["T3-N1-A2-plain"]["last_rows"] == 3 and paths["T1-N257-A4-plain"]["last_rows"] == 1      # the r >= R break
    assert paths["T1-N1-A1-plain"]["last_rows"] == 1 and paths["T8-N256-A4-plain"]["last_rows"] == 4
    for k, c in cases.items():
        lists = paths[k]["lists"]
        assert lists.sum() == c["R"]
        if c["variant"] == "unused-action":
            assert lists[c["unused"]] == 0 and np.count_nonzero(lists) == c["A"] - 1
        if c["variant"] == "one-action":
            assert lists[-1] == c["R"] and np.count_nonzero(lists) == 1
        if c["variant"] == "clamped":
            raw = c["action"].reshape(-1)
            assert {-1, c["A"], 2 ** 40} <= set(raw.tolist()) or c["R"] < 23
            assert (raw < 0).any() and ((raw < 0) | (raw >= c["A"])).sum() == -(-c["R"] // 11)
        if c["R"] >= 64:
            assert (c["mask"] == 0).all() == (c["variant"] == "mask0") and (c["mask"] == 1).all() == (c["variant"] == "mask1")
    assert cases["T8-N256-A4-gamma0"]["gamma"] == 0.0 and cases["T8-N256-A4-gamma1"]["gamma"] == 1.0
    assert 600 % H.NSTEP_SUM_SPANS[0] == 0 and 600 % H.NSTEP_SUM_SPANS[1] != 0 and 257 % H.NSTEP_SUM_SPANS[0] != 0      # ragged spans


# ----------------------------------------------------------------------------------------------------- dra_oc_loss_bwd
@pytest.mark.parametrize("c", H.oc_cases(), ids=_ids(H.oc_cases()))
def test_oc_cases_carry_the_bar(c):
    ref = H.oc_ref(c)
    _floors(c["name"], H.oc_f32(c), ref)
    assert np.all(ref["dphi"][c["phi"] == 0] == 0)
    if c["variant"] == "init1":
        assert not ref["dw_beta"].any() and not ref["db_beta"].any() and ref["loss"][3] == 0 and ref["dw_q"].any()
    if c["A"] == 1:
        assert not ref["dw_pi"].any() and not ref["db_pi"].any()          # one action: its probability is 1, no gradient


def test_oc_cases_reach_their_paths():
    cases = {c["name"]: c for c in H.oc_cases()}
    assert [(c["T"], c["N"], c["O"], c["A"]) for c in H.oc_cases()[:len(H.OC_SHAPES)]] == H.OC_SHAPES
    paths = {k: H.oc_path(c) for k, c in cases.items()}
    lists = paths["T8-N256-O8-A4-lists"]
    for key in ("by_option", "by_prev"):                    # fc_q / fc_pi by option, fc_beta by prev_option
        assert tuple(lists[key][:6]) == H.OC_LIST_LENGTHS and lists[key].sum() == 2048 and lists[key][6:].min() > 258
    assert lists["compaction_trips"] == 8
    opt = cases["T8-N256-O8-A4-lists"]["option"].reshape(-1)
    # the compaction of the 255 .. 258-row lists spans trips: their rows are spread over all eight blocks of 256 rows
    for o in (2, 3, 4, 5):
        assert len(set(np.nonzero(opt == o)[0] // 256)) == 8
    one = paths["T2048-N1-O1-A2-plain"]
    assert tuple(one["by_option"]) == (2048,) and tuple(one["by_prev"]) == (2048,) and one["env_trips"] == 1
    assert paths["T1-N257-O4-A6-plain"]["env_trips"] == 2 and paths["T1-N257-O4-A6-plain"]["last_rows"] == 1
    assert paths["T3-N1-O2-A3-plain"]["last_rows"] == 3 and paths["T1-N257-O4-A6-plain"]["compaction_trips"] == 2
    assert min(paths["T2-N300-O2-A18-plain"]["by_option"]) > 256          # a list longer than 256: second trip of i += 256
    for k, c in cases.items():
        if c["variant"] == "clamped":
            for key, n in (("option", c["O"]), ("prev", c["O"]), ("action", c["A"])):
                raw = c[key].reshape(-1)
                assert (raw < 0).any() and ((raw < 0) | (raw >= n)).sum() == -(-c["R"] // 11), (k, key)
        if c["variant"] == "ties":
            q = c["q"][:, ::2]
            assert ((q == q.max(-1, keepdims=True)).sum(-1) >= 2).all() and (q[..., -1] == q.max(-1)).all()
        assert (c["variant"] != "init1" or (c["init"] == 1).all()) and (c["R"] < 64 or c["variant"] == "init1" or (c["init"] == 0).any())
        assert (c["eps"] == 0).all() == (c["variant"] == "eps0") and (c["eps"] == 1).all() == (c["variant"] == "eps1")
        assert (c["ent_w"] == 0) == (c["variant"] == "ent0")


# ---------------------------------------------------------------------------------------- dueling over atoms, PER weights
@pytest.mark.parametrize("c", H.dueling_cases(), ids=_ids(H.dueling_cases()))
def test_dueling_cases_carry_the_bar(c):
    ref = H.dueling_ref(c)
    _floors(c["name"], H.dueling_f32(c), ref)
    if c["A"] == 1:
        assert np.array_equal(ref["logits"][:, 0], c["value"].astype(np.float64)) and not ref["d_adv"].any()


def test_dueling_cases_reach_their_paths():
    got = {c["name"]: (c["wgs"], c["last_wg"]) for c in H.dueling_cases()}
    assert got == {"B1-A1-Z1": (1, 1), "B1-A1-Z51": (1, 51), "B5-A3-Z51": (1, 255), "B5-A18-Z52": (2, 4), "B257-A2-Z1": (2, 1)}


@pytest.mark.parametrize("c", H.per_cases(), ids=_ids(H.per_cases()))
def test_per_cases_carry_the_bar(c):
    ref = H.per_ref(c)
    _floors(c["name"], H.per_f32(c), ref)
    assert int(np.argmin(c["sp"])) == c["argmax"] and ref["w"].max() == 1.0
    assert c["argmax"] // 64 == (c["B"] - 1) // 64 and c["argmax"] in (c["B"] - 1, 64 * ((c["B"] - 1) // 64))     # the last wave
    if c["beta"] == 0.0:
        assert np.all(ref["w"] == 1.0)


def test_per_cases_cover_the_table():
    cs = H.per_cases()
    assert {(c["B"], c["alpha"], c["beta"]) for c in cs} == {(b, a, k) for b in H.PER_BATCHES for a in H.PER_ALPHAS for k in H.PER_BETAS}
    for b in (65, 1024):
        assert {c["argmax"] for c in cs if c["B"] == b} == {b - 1, 64 * ((b - 1) // 64)}


# ------------------------------------------------------------------------------------------------------- noisy layers
@pytest.mark.parametrize("c", H.noisy_cases() + [H.noisy_case(s) for s in H.NOISY_OFFSET_SHAPES],
                         ids=_ids(H.noisy_cases() + [H.noisy_case(s) for s in H.NOISY_OFFSET_SHAPES]))
def test_noisy_cases_carry_the_bar(c):
    for act in H.NOISY_ACTS:
        ref = H.noisy_ref(c, act)
        _floors("%s %s" % (c["name"], act), H.noisy_f32(c, act), ref, keys=("y", "dw_mu", "dw_sigma", "db_mu", "db_sigma", "dx"))
        if act == "relu":
            assert (ref["y"] == 0).any() and (ref["y"] > 0).any()


def test_noisy_zero_noise_is_the_plain_layer():
    for shape in H.NOISY_OFFSET_SHAPES:
        c = H.noisy_case(shape, zero_noise=True)
        assert all(np.all(c[k] == 0) and np.signbit(c[k]).any() and not np.signbit(c[k]).all() for k in ("e_in", "e_out", "e_b"))
        ref = H.noisy_ref(c, "none")
        assert np.array_equal(ref["y"], ref["plain"]) and not ref["dw_sigma"].any() and not ref["db_sigma"].any()


NOISY_EXPECT = {
    # shape: forward kernel, row passes or (row groups, kb, cpw), what the case is named for
    (2, 8, 3): "col4-vec", (3, 20, 33): "col4-vec", (4, 36, 1): "col4-vec", (7, 516, 31): "col4-vec", (8, 20, 32): "mfma1",
    (31, 36, 33): "mfma1", (33, 516, 65): "mfma2", (65, 8, 31): "mfma2", (1024, 36, 33): "mfma2", (9, 7, 5): "col4-scalar",
    (33, 513, 2): "col4-scalar",
}


def test_noisy_cases_reach_their_paths():
    assert set(NOISY_EXPECT) == set(H.NOISY_SHAPES)
    for (rows, k, n), fwd in NOISY_EXPECT.items():
        path = H.noisy_path(rows, k, n)
        assert path["fwd"] == fwd, (rows, k, n, path)
        assert (path["bwd_w"], path["bwd_x"]) == (("vec", "mfma") if k % 4 == 0 else ("scalar", "any"))
        off = H.noisy_path(rows, k, n, aligned=False)         # a view one float into a buffer: always the scalar kernels
        assert off["fwd"].endswith("scalar") and (off["bwd_w"], off["bwd_x"]) == ("scalar", "any")
    # column kernel: a single ragged pass (2, 3), exactly one pass (4), a full pass and a ragged one (7)
    assert [(r, -(-r // 4), r % 4) for r, _, _ in H.NOISY_SHAPES[:4]] == [(2, 1, 2), (3, 1, 3), (4, 1, 0), (7, 2, 3)]
    p = H.noisy_fwd_plan(8, 20, 32)                           # one half-filled chunk: ok[u] false from k = 20 on
    assert (p["rt"], p["chunks"], p["cpw"], p["kb"]) == (1, 1, 2, 1) and 20 % 32 == 20
    p = H.noisy_fwd_plan(31, 36, 33)                          # two column tiles; chunk 1 holds 4 of 32 k; wave 0's range ends at K
    assert (p["rt"], p["col_tiles"], p["chunks"], p["cpw"], p["kb"]) == (1, 2, 2, 2, 1)
    p = H.noisy_fwd_plan(33, 516, 65)                         # RT = 2 with ONE valid row in the second tile; 17 chunks
    assert (p["rt"], p["row_groups"], p["chunks"], p["col_tiles"]) == (2, 1, 17, 3) and 33 - 32 == 1
    assert p["cpw"] * 4 * p["kb"] >= 17 > p["cpw"] * 4 * (p["kb"] - 1) and (17 % p["cpw"] != 0 or p["cpw"] * 4 * p["kb"] > 17)
    p = H.noisy_fwd_plan(65, 8, 31)                           # two row groups, the second with one valid row of 64
    assert (p["rt"], p["row_groups"], p["chunks"]) == (2, 2, 1)
    p = H.noisy_fwd_plan(1024, 36, 33)
    assert (p["rt"], p["row_groups"], p["col_tiles"]) == (2, 16, 2)
    for shape in H.NOISY_OFFSET_SHAPES:
        assert shape[1] % 4 == 0
    assert {H.noisy_path(*s)["fwd"] for s in H.NOISY_OFFSET_SHAPES} == {"col4-vec", "mfma2"}
    b = H.noisy_bwd_plan(33, 516, 65)
    assert (b["col_blocks"], b["row_groups"]) == (5, 2) and b["npw"] % 2 == 0 and b["nb"] * 4 * b["npw"] >= 65


def test_noisy_plans_equal_the_library():
    """dra_noisy_workspace_floats is host-only arithmetic: the Python restatement of fwd_plan / bwd_plan gives its numbers at
    every shape of the sweep and at the launcher's limits."""
    from deeprl_amd._lib import lib
    fn = lib.dra_noisy_workspace_floats.raw
    shapes = list(H.NOISY_SHAPES) + list(H.NOISY_OFFSET_SHAPES) + [(1, 1, 1), (1024, 3136, 512), (32, 512, 51 * 18), (8, 4, 1)]
    for rows, k, n in shapes:
        f, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert fn(rows, k, n, ctypes.byref(f), ctypes.byref(b)) == 0
        assert (f.value, b.value) == H.noisy_workspace(rows, k, n), (rows, k, n)
    f = ctypes.c_int64(-1)
    for rows in (0, 1025):
        assert fn(rows, 8, 8, ctypes.byref(f), ctypes.byref(f)) == -22 and f.value == -1


# ---------------------------------------------------------------------------------------------------- rollout heads
@pytest.mark.parametrize("c", H.q_head_cases(), ids=_ids(H.q_head_cases()))
def test_q_head_cases_carry_the_bar(c):
    ref = H.q_head_ref(c)
    q32 = H.head_f32(ref["phi"], c["w"], c["b"])
    _floors(c["name"], dict(q=q32), dict(q=ref["q"]))
    assert (ref["phi"] == 0).any() and (ref["phi"] > 0).any()
    if c["winner"] is not None:                               # the tie is exact in both precisions and beats every other action
        tied, others = ref["q"][:, c["tied"]], np.delete(ref["q"], c["tied"], axis=1)
        assert np.allclose(tied, tied[:, :1], rtol=1e-13, atol=0) and all(np.array_equal(q32[:, t], q32[:, c["winner"]]) for t in c["tied"])
        assert others.size == 0 or np.all(tied[:, 0] - others.max(-1) > 1e-5 * np.abs(ref["q"]).max())
        assert np.all(np.argmax(q32, -1) == c["winner"]) and c["winner"] == min(c["tied"])
    else:                                                     # no row's decision sits within the score margin
        top2 = np.sort(ref["q"], -1)[:, -2:]
        assert c["A"] == 1 or np.all(top2[:, 1] - top2[:, 0] >= 1e-5), "a row within 1e-5 in score: it would have to be left out"


def test_q_head_cases_cover_the_table():
    cs = H.q_head_cases()
    assert [(c["A"], c["B"]) for c in cs] == [(a, b) for a in H.Q_HEAD_A for b in H.Q_HEAD_B]
    assert {c["ties"] for c in cs} == set(H.Q_TIES) and {c["explore_kind"] for c in cs} == set(H.Q_EXPLORE)
    assert {c["b"] is None for c in cs} == {True, False}
    assert any(c["ties"] == "last" and c["A"] - 1 in c["tied"] and c["winner"] > 0 for c in cs)
    assert any(c["ties"] == "first" and c["winner"] == 0 and c["A"] - 1 in c["tied"] and c["A"] > 1 for c in cs)
    for c in cs:
        assert (c["explore"] != 0).all() == (c["explore_kind"] == "all") or c["B"] == 1
        assert (c["explore"] == 0).all() == (c["explore_kind"] == "none") or c["B"] == 1


@pytest.mark.parametrize("c", H.oc_head_cases(), ids=_ids(H.oc_head_cases()))
def test_oc_head_cases_carry_the_bar_and_decide_clear_of_the_margin(c):
    ref, f32 = H.oc_head_ref(c), H.oc_head_f32(c)
    _floors(c["name"], f32, ref, keys=("q", "beta", "logits"))
    assert np.array_equal(f32["phi"], ref["phi"])
    dec = H.oc_head_decide(c, f32["q"], f32["beta"], lambda r, o: f32["logits"][r, o])
    near = dec["margin"] < 1e-6
    assert near.sum() <= 0.01 * c["B"] and not (c["exact"] and near.any()), "%d rows within 1e-6 of an action boundary" % near.sum()
    # the option's boundaries as well: float64 probabilities give the option the float32 order gives
    for r in range(c["B"]):
        g = int(np.argmax(ref["q"][r]))
        assert g == int(np.argmax(f32["q"][r]))
        pi_opt = np.full(c["O"], c["eps"] / c["O"])
        pi_opt[g] += 1.0 - c["eps"]
        prev = int(np.clip(c["prev_option"][r], 0, c["O"] - 1))
        pi_hat = (1.0 - ref["beta"][r]) * (np.arange(c["O"]) == prev) + ref["beta"][r] * pi_opt
        p, u = (pi_opt, c["uniform"][r, 0]) if c["init"][r] else (pi_hat, c["uniform"][r, 1])
        cdf = np.cumsum(p / p.sum())
        hit = np.nonzero(cdf[:-1] > float(u))[0]
        assert (hit[0] if hit.size else c["O"] - 1) == dec["option"][r], (c["name"], r)


def test_oc_head_cases_cover_the_table():
    cs = H.oc_head_cases()
    assert [(c["O"], c["A"], c["B"], c["eps"]) for c in cs] == [(o, a, b, e) for o, a in H.OC_HEAD_OA for b in H.OC_HEAD_B for e in H.OC_HEAD_EPS]
    assert sorted({2 * o + o * a for o, a in H.OC_HEAD_OA}) == [3, 8, 9, 32, 33, 160]        # a chunk of 8, a round of 4 waves, +1
    assert {c["uniforms"] for c in cs} == set(H.OC_UNIFORMS) and {c["init_kind"] for c in cs} == set(H.OC_INIT)
    assert {c["prev_kind"] for c in cs} == set(H.OC_PREV) and {c["bias"] for c in cs} == {True, False}
    assert H.ALMOST_ONE < 1.0 and np.float32(H.ALMOST_ONE) == np.nextafter(np.float32(1), np.float32(0))
    for col, branch in ((0, 1), (1, 0)):                      # the fresh-option uniform where a row is initial, and the reverse
        for v in ("zero", "almost-one"):
            assert any(c["uniforms"] == "col%d-%s" % (col, v) and (c["init"] == branch).any() and c["O"] > 1 for c in cs), (col, v)
    assert any(c["prev_kind"] == "minus-one" and (c["prev_option"] == -1).any() and (c["init"] == 0).any() for c in cs)
    assert any(c["prev_kind"] == "count" and (c["prev_option"] == c["O"]).any() and (c["init"] == 0).any() for c in cs)


@pytest.mark.parametrize("c", H.gauss_cases(), ids=_ids(H.gauss_cases()))
def test_gauss_cases_reach_their_paths(c):
    assert (-(-c["n"] // 256), c["n"] % 256) in ((1, 255), (2, 1), (5, 1)) and c["A"] in (1, 64)
    assert np.abs(np.tanh(c["z"].astype(np.float64))).max() > 0.999 and np.all(np.isfinite(c["action"]))
