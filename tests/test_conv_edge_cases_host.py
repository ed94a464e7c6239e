"""CPU proof of tests/conv_edge_cases.py at 256 compute units: every case reaches the path and share shape it is named for (by the
module's restatement of the launchers' conditions; tests/test_gpu_conv_edges.py ties that restatement to the library through the slab
count and the slabs that are written), the tables together cover the coverage list with no unused name, the slab counts agree with
the closed forms in the headers, the integer operand sets keep every partial sum below 2^24, the float32 CPU run of every forward
reference stays within the bar, and the kept-subset rule never drops a sample of a ragged last group or share."""
import numpy as np
import pytest

import conv_edge_cases as E

N_CU = 256
FWD_CASES = E.fwd_cases(N_CU)
COVERAGE = E.coverage(FWD_CASES, N_CU)


def _ids(cases):
    return [c["name"] for c in cases]


def _figure(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (np.abs(want).max() + 1e-300))


def test_tables_are_what_the_issue_lists():
    names = _ids(FWD_CASES) + _ids(E.BWD_CASES)
    assert len(names) == len(set(names)), "case names must be unique"
    assert max(c["batch"] for c in FWD_CASES + list(E.BWD_CASES)) == E.MAX_BATCH == 1025
    assert E.conv1_tp_batches(256) == [(384, 2), (511, 1), (512, 1), (512, 2), (1023, 1), (1024, 1)]
    tp = {(c["batch"], c["nz"]): c["reaches"] for c in FWD_CASES if c["reaches"][0] == "conv1-u8-tp"}
    assert tp == {(384, 1): ("conv1-u8-tp", 1, 2), (511, 1): ("conv1-u8-tp", 1, 2), (512, 1): ("conv1-u8-tp", 1, 1),
                  (1023, 1): ("conv1-u8-tp", 1, 1), (1024, 1): ("conv1-u8-tp", 2, 1), (1025, 1): ("conv1-u8-tp", 2, 1),
                  (384, 2): ("conv1-u8-tp", 1, 1), (512, 2): ("conv1-u8-tp", 2, 1)}
    assert E.conv1_tp_shape(1025, 1, 256)["last_group_samples"] == 1 and E.conv1_tp_shape(1024, 1, 256)["last_group_samples"] == 2
    assert E.conv1_tp_shape(389, 1, 256)["tp"] == 2          # what tests/test_gpu_kernels.py already runs
    assert {c["nz"] for c in FWD_CASES} == {1, 2, 3} and all(1 <= c["nz"] <= E.MAX_Z for c in FWD_CASES)
    assert E.BAR == 1e-5 and E.BAR_OVERRIDES == {}
    assert all(len(v) == 2 for v in E.BAR_OVERRIDES.values()) and all(k[0] in names for k in E.BAR_OVERRIDES)
    assert E.TILES_PER_SAMPLE == {1: 13, 2: 3, 3: 2} and E.GROUPS_PER_SAMPLE == {1: 7, 2: 1, 3: 1}
    assert [E.slab_stride(l) for l in (1, 2, 3)] == [32 * 256 + 32, 64 * 512 + 64, 64 * 576 + 64]      # no alignment gap in a slab


def test_tp4_is_unreachable_on_256_compute_units():
    """tp = 4 needs 2 * batch < per = 2 * n_cu / nz with batch >= 384: n_cu > 384 nz (DESIGN.md notes it; the code is left alone)."""
    assert not E.tp4_reachable(256) and not E.tp4_reachable(304) and not E.tp4_reachable(384)
    assert E.tp4_reachable(385)


@pytest.mark.parametrize("c", FWD_CASES, ids=_ids(FWD_CASES))
def test_forward_case_reaches_its_path(c):
    path = E.fwd_path(c["layer"], c["u8"], c["batch"], c["nz"], N_CU)
    assert path == c["reaches"] and path != ("refused",)
    b = c["batch"]
    want = ("latency eight-wave",) if b <= 16 else ("latency four-wave",) if b < 128 else None
    if want is not None:
        assert path == want
    elif c["layer"] == 1 and not c["u8"]:
        assert path == ("two-tile conv1-f32",)
    elif c["layer"] == 1 and b >= 384:
        assert path[0] == "conv1-u8-tp" and path[2] in (1, 2) and (path[1] == 2) == (b >= 2 * (512 // c["nz"]))
    else:
        assert path == ("persistent conv%d" % c["layer"],)


@pytest.mark.parametrize("c", E.BWD_CASES, ids=_ids(E.BWD_CASES))
def test_backward_case_reaches_its_roles_and_share_shape(c):
    r = E.bwd_path(c["layer"], c["u8"], c["batch"], c["variant"])
    assert r == c["reaches"]
    # the restatement of dra_conv_wgrad_slabs against the closed form of the role dra_conv_bwd_fused launches
    assert E.wgrad_slabs(c["layer"], c["batch"], E.KSPLIT, c["variant"]) == r["n_slabs"]
    if c["name"] in E.BWD_SHARES:
        assert (r["wgrad"], r["n_slabs"], r["spw"], r["last_share"]) == E.BWD_SHARES[c["name"]]
    if r["spw"] is not None and E.WG_ROLES[r["wgrad"]][0]:
        assert (r["n_slabs"] - 1) * r["spw"] + r["last_share"] == c["batch"] and 1 <= r["last_share"] <= r["spw"]
    roles = [x for l in r["launches"] for x in l if x != "tp"]
    assert roles.count(r["wgrad"]) == 1 and (c["layer"] == 1) == (E.dgrad_role(r) is None)
    # the scatter bit changes nothing about the weight gradient
    plain = E.bwd_path(c["layer"], c["u8"], c["batch"], c["variant"] & ~E.SCATTER & ~E.FUSED)
    if c["variant"] & E.OWGRAD:
        assert (plain["wgrad"], plain["n_slabs"]) == (r["wgrad"], r["n_slabs"])


def test_every_named_share_shape_has_its_case():
    assert set(E.BWD_SHARES) <= set(_ids(E.BWD_CASES))


def test_slab_counts_equal_the_closed_forms_at_every_batch():
    for layer in (1, 2, 3):
        for variant in E.VARIANTS.values():
            for batch in range(1, E.MAX_BATCH + 1):
                assert E.wgrad_slabs(layer, batch, E.KSPLIT, variant) == E.bwd_path(layer, False, batch, variant)["n_slabs"], (layer, variant, batch)


@pytest.mark.parametrize("item", list(COVERAGE), ids=list(COVERAGE))
def test_coverage_item_is_reached(item):
    assert COVERAGE[item](), "no case reaches: " + item


def test_coverage_list_has_no_unused_case():
    """Every case is what at least one coverage item asks for: dropping it makes an item fail."""
    for i, c in enumerate(FWD_CASES):
        rest = FWD_CASES[:i] + FWD_CASES[i + 1:]
        cov = E.coverage(rest, N_CU)
        assert not all(p() for p in cov.values()), "forward case %s is needed by no coverage item" % c["name"]
    saved = E.BWD_CASES
    try:
        for i, c in enumerate(saved):
            E.BWD_CASES = saved[:i] + saved[i + 1:]
            assert not all(p() for p in E.coverage(FWD_CASES, N_CU).values()), "backward case %s is needed by no coverage item" % c["name"]
    finally:
        E.BWD_CASES = saved


def test_batch_independence_tables_reach_every_form():
    paths = {E.fwd_path(l, u8, b, nz, N_CU) for l, u8, b, nz in E.fwd_independence(N_CU)}
    assert paths == {c["reaches"] for c in FWD_CASES}
    for l, u8, b, nz in E.fwd_independence(N_CU):
        p = E.fwd_path(l, u8, b, nz, N_CU)
        assert b == 2 or E.fwd_path(l, u8, b - 1, nz, N_CU) != p, "not the smallest batch of its path"
    forms = {E.dgrad_role(c["reaches"]) for c in E.BWD_CASES if c["layer"] > 1}
    assert forms <= {f for _, _, _, f in E.BWD_INDEPENDENCE}
    for layer, batch, variant, form in E.BWD_INDEPENDENCE:
        assert E.dgrad_role(E.bwd_path(layer, False, batch, variant)) == form
        if batch > 3:
            assert E.dgrad_role(E.bwd_path(layer, False, batch - 1, variant)) != form


def test_ring_stack_rule():
    assert E.ring_stack_slots(0, None) == [4, 5, 6, 0] and E.ring_stack_slots(2, 3) == [6, 0, 1, 2] and E.ring_stack_slots(6, None) == [3, 4, 5, 6]
    assert E.ring_stack_slots(2, 1) == [1, 1, 1, 2] and E.ring_stack_slots(0, 1) == [6, 6, 6, 0] and E.ring_stack_slots(0, 0) == [0] * 4
    assert {n for n, _ in E.RING_CASES} == {0, 2, 6} and {a for _, a in E.RING_CASES} == {None, 3, 1, 0}


@pytest.mark.parametrize("c", FWD_CASES + list(E.BWD_CASES), ids=_ids(FWD_CASES + list(E.BWD_CASES)))
def test_integer_operands_are_exact_in_float32(c):
    b = E.int_bounds(c["layer"], c["batch"])
    assert set(b) == {"fwd", "dw", "db", "dx", "fold"} and max(b.values()) < 2 ** 24, (c["name"], b)


def test_integer_operands_are_distinct_per_sample_and_channel():
    for layer in (1, 2, 3):
        rs = E._rs("distinct", layer)
        x8, x, coef = E.draw_input(rs, layer, 8, "integer")
        w, b = E.draw_weights(rs, layer, "integer")
        assert coef == 1.0 and x.min() == 0 and x.max() == 3 and w.min() == -2 and w.max() == 2
        if x8 is not None:
            assert np.array_equal(x8.astype(np.float32), x)
        planes = x.reshape(-1, x.shape[2] * x.shape[3])
        assert len({p.tobytes() for p in planes}) == len(planes), "two (sample, channel) planes are equal"
        taps = w.reshape(w.shape[0] * w.shape[1], -1)
        assert len({t.tobytes() for t in taps}) == len(taps) or layer == 3      # 3 x 3 taps of 5 values: a repeat among 4096 is chance
        assert len({t.tobytes() for t in w.reshape(w.shape[0], -1)}) == w.shape[0]


@pytest.mark.parametrize("c", FWD_CASES, ids=_ids(FWD_CASES))
def test_kept_subset_keeps_the_ragged_ends(c):
    keep = E.kept_samples(c["layer"], c["u8"], c["batch"], c["nz"], N_CU)
    B = c["batch"]
    assert len(keep) >= min(B, 40) and len(set(keep)) == len(keep) and keep.min() == 0 and keep.max() == B - 1
    assert set(range(min(B, 40))) <= set(keep) and set(range(max(0, B - 40), B)) <= set(keep)
    first = E.first_sample_of_last_iteration(c["layer"], c["u8"], B, c["nz"], N_CU)
    assert set(range(first, B)) <= set(keep)
    if c["reaches"][0] == "conv1-u8-tp":
        t = E.conv1_tp_shape(B, c["nz"], N_CU)
        # walk the grid as the kernel does (conv_v2.hip:1376-1377): the samples of every workgroup's last group are kept
        for wg in range(t["nwg"]):
            g = wg + ((t["n_groups"] - 1 - wg) // t["nwg"]) * t["nwg"]
            if g >= ((t["n_groups"] - 1) // t["nwg"]) * t["nwg"]:
                b0 = (g // t["tp"]) * t["spg"]
                assert set(range(b0, min(B, b0 + t["spg"]))) <= set(keep)
        assert set(range(B - t["last_group_samples"], B)) <= set(keep)
    if c["layer"] > 1 or B <= 160:
        assert len(keep) == B


@pytest.mark.parametrize("c", E.BWD_CASES, ids=_ids(E.BWD_CASES))
def test_kept_subset_keeps_the_last_share(c):
    r = c["reaches"]
    share = r["last_share"] or 0
    keep = E.kept_samples(c["layer"], c["u8"], c["batch"], 1, N_CU, last_share=share)
    assert len(keep) >= min(c["batch"], 40) and set(range(c["batch"] - share, c["batch"])) <= set(keep)


@pytest.mark.parametrize("c", FWD_CASES, ids=_ids(FWD_CASES))
def test_forward_inputs_carry_the_bar(c):
    op = E.fwd_operands(c["layer"], c["batch"], c["nz"], "random", N_CU)
    keep = op["keep"]
    for z in range(c["nz"]):
        got = E.act64(E.conv_ref(op["x"][z][keep], op["w"][z], op["b"][z], c["layer"], dtype=np.float32), c["act"])
        fig = _figure(got, E.act64(op["pre"][z], c["act"]))
        print("%s y[%d]: float32 CPU run err/scale %.3g (bar %.1g)" % (c["name"], z, fig, E.bar(c["name"], "y")))
        assert fig <= E.bar(c["name"], "y"), "%s: the float32 CPU run misses the bar: %.3g -- the inputs do not carry it" % (c["name"], fig)
        assert (op["pre"][z] < 0).mean() > 0.1, "hardly a negative pre-activation: act none would show nothing relu hides"
    ints = E.fwd_operands(c["layer"], c["batch"], c["nz"], "integer", N_CU)
    for z in range(c["nz"]):
        pre = ints["pre"][z]
        assert np.array_equal(pre, np.rint(pre)) and np.abs(pre).max() <= E.int_bounds(c["layer"], c["batch"])["fwd"]
        assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
        assert ints["coef"] == 1.0 and ints["x"][z].max() == 3
