"""CPU proof of tests/linear_edge_cases.py: every case reaches the path it is named for (by the module's restatement of the
launchers' conditions; tests/test_gpu_linear_edges.py ties that restatement to the library through the workspace it writes),
the tables together cover COVERAGE, the float32 CPU run of every reference stays within the bar its GPU test applies, and the
integer operand sets keep every partial sum below 2^24."""
import numpy as np
import pytest

import linear_edge_cases as E

F = np.float32


def _ids(cases):
    return [c["name"] for c in cases]


def _figure(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (np.abs(want).max() + 1e-300))


def _judge(name, key, got32, want64):
    fig = _figure(got32, want64)
    print("%s %s: float32 CPU run err/scale %.3g (bar %.1g)" % (name, key, fig, E.bar(name, key)))
    assert fig <= E.bar(name, key), "%s %s: the float32 CPU run misses the bar: %.3g -- the inputs do not carry it" % (name, key, fig)
    if (name, key) in E.BAR_OVERRIDES:
        b, measured = E.BAR_OVERRIDES[(name, key)]
        assert b == max(E.BAR, 4 * measured) and 0.5 * measured <= fig <= 2 * measured, (name, key, b, measured, fig)


def test_tables_are_what_the_issue_lists():
    shapes = {(c["B"], c["K"], c["O"]) for c in E.FWD_CASES}
    assert shapes >= {(1, 1, 1), (1, 64, 5), (9, 65, 3), (33, 128, 7), (40, 129, 6), (128, 256, 2), (31, 257, 4), (128, 512, 512),
                      (3, 260, 5), (5, 100, 6), (129, 256, 2), (128, 512, 513), (5, 958, 6), (32, 516, 3), (9, 1000, 4), (7, 2048, 5),
                      (7, 2052, 5), (32, 4096, 3), (1, 3136, 2), (5, 1024, 6), (5, 1022, 6), (5, 1030, 9), (3, 4100, 4), (33, 1092, 6),
                      (33, 2000, 6), (33, 3136, 512), (33, 3136, 40), (65, 3136, 1), (32, 3136, 512), (33, 3136, 8)}
    assert [(c["B"], c["K"], c["O"], c["ksplit"]) for c in E.SLABS_CASES] == [(5, 200, 7, 2), (5, 200, 7, 4), (5, 200, 7, 9), (33, 130, 33, 3)]
    assert [c["ksplit"] for c in E.SLABS_ONE_CASES] == [8, 14, 28] and all((c["B"], c["K"], c["O"], c["nz"]) == (33, 3136, 40, 2) for c in E.SLABS_ONE_CASES)
    assert [(c["B"], c["I"], c["O"], c["db"]) for c in E.BWD_W_CASES] == [
        (1, 1, 1, True), (5, 4, 63, True), (5, 4, 64, True), (33, 63, 64, True), (33, 64, 64, True), (65, 31, 3, True), (65, 32, 3, True),
        (32, 17, 70, True), (64, 5, 9, True), (65, 5, 9, True), (33, 63, 64, False)]
    assert [(c["B"], c["I"], c["O"], c["mask"]) for c in E.BWD_X_CASES] == [
        (1, 1, 1, None), (33, 33, 65, None), (33, 33, 65, "relu"), (33, 33, 65, "tanh"), (5, 1023, 512, None), (5, 3136, 511, "tanh"),
        (1, 1024, 512, None), (33, 1030, 512, "relu"), (32, 3136, 512, "tanh")]
    assert {(c["B"], c["I"]) for c in E.XW_CASES} == {(1, 1024), (33, 1030)}
    assert sorted({c["n"] for c in E.ACT_BWD_CASES}) == [1, 2048 * 256, 2048 * 256 + 1]
    assert [(c["B"], c["K"], c["O"], c["act"], c["x_relu"]) for c in E.AUTOGRAD_CASES] == [
        (9, 65, 3, "tanh", False), (32, 516, 3, "relu", False), (33, 3136, 512, "relu", True), (40, 129, 6, None, False)]
    assert E.BAR == 1e-5
    # an override carries max(1e-5, 4 x the float32 CPU figure) with the figure beside it (checked where it is used)
    assert all(len(v) == 2 for v in E.BAR_OVERRIDES.values())
    assert all(k[0] in {c["name"] for c in E.ALL_CASES} for k in E.BAR_OVERRIDES)
    assert not E.xw_one512_accepts(1023) and E.xw_one512_accepts(1024)
    assert [E.slabs_one_accepts(K, ks, off is None) for _, K, ks, off in E.SLABS_ONE_REFUSALS] == [False] * 4
    assert all(E.slabs_one_accepts(c["K"], c["ksplit"], True) for c in E.SLABS_ONE_CASES)


@pytest.mark.parametrize("c", E.FWD_CASES, ids=_ids(E.FWD_CASES))
def test_forward_case_reaches_its_path(c):
    assert E.fwd_case_path(c) == c["reaches"], (c["name"], E.fwd_case_path(c))
    assert 1 <= c["nz"] <= E.MAX_Z and c["act"] in E.ACTS


def test_forward_split_counts_the_issue_works_out():
    lim = {c["name"]: E._limits(c) for c in E.FWD_CASES if c["reaches"][0] == "igemm"}
    assert lim["fwd-5x1030x9"] == (8, 8, 6) and lim["fwd-3x4100x4"] == (32, 32, 22) and lim["fwd-33x1092x6"] == (9, 9, 9)
    assert lim["fwd-33x2000x6-ws5"] == (16, 5, 5) and lim["fwd-33x2000x6-ws-null"] == (16, 1, 1)
    assert lim["fwd-5x1024x6-x-off"] == (8, 8, 8) and lim["fwd-5x1022x6"] == (8, 8, 8) and lim["fwd-5x958x6"] == (1, 1, 1)
    assert lim["fwd-33x3136x512-w-off"] == (8, 8, 7) and lim["fwd-33x3136x8-ws-1"] == (24, 7, 7)


@pytest.mark.parametrize("c", E.BWD_W_CASES, ids=_ids(E.BWD_W_CASES))
def test_weight_gradient_case_reaches_its_tiles(c):
    assert E.bwd_w_path(c["B"], c["I"], c["O"]) == c["reaches"] == E.BWD_W_REACHES[c["name"]]


@pytest.mark.parametrize("c", E.BWD_X_CASES, ids=_ids(E.BWD_X_CASES))
def test_input_gradient_case_reaches_its_path(c):
    assert E.bwd_x_path(c["B"], c["I"], c["O"]) == c["reaches"]


def test_pair_cases_run_the_one_pass_role_beside_the_64_wide_weight_gradient():
    for c in E.XW_CASES:
        assert c["reaches"][0][0] == "one512" and c["reaches"][1][1] == 64 and E.xw_one512_accepts(c["I"])
    assert {c["reaches"][0][1] for c in E.XW_CASES} == {False, True}


@pytest.mark.parametrize("item", list(E.COVERAGE), ids=list(E.COVERAGE))
def test_coverage_item_is_reached(item):
    assert E.COVERAGE[item](), "no case reaches: " + item


@pytest.mark.parametrize("c", E.ALL_CASES, ids=_ids(E.ALL_CASES))
def test_integer_operands_are_exact_in_float32(c):
    if "n" in c or c["name"].startswith("autograd"):
        return                                         # act_bwd and autograd run on the random set only
    assert E.int_bound(c) < 2 ** 24, (c["name"], E.int_bound(c))


@pytest.mark.parametrize("c", E.FWD_CASES, ids=_ids(E.FWD_CASES))
def test_forward_inputs_carry_the_bar(c):
    op = E.fwd_operands(c["name"], "random")
    for z in range(c["nz"]):
        _judge(c["name"], "y", E.fwd_ref(op["x"][z], op["w"][z], op["bias"][z], c["act"], dtype=F), op["want"][z])
    ints = E.fwd_operands(c["name"], "integer")
    for z in range(c["nz"]):
        got = E.fwd_ref(ints["x"][z], ints["w"][z], ints["bias"][z], None, dtype=np.int64)
        assert np.array_equal(got, ints["want"][z]) and np.abs(ints["want"][z]).max() <= E.int_bound(c)
        assert np.array_equal(ints["want"][z].astype(F).astype(np.float64), ints["want"][z])


@pytest.mark.parametrize("c", E.SLABS_CASES + E.SLABS_ONE_CASES, ids=_ids(E.SLABS_CASES + E.SLABS_ONE_CASES))
def test_slab_inputs_carry_the_bar(c):
    op = E.slabs_operands(c["name"], "random")
    for z in range(c["nz"]):
        _judge(c["name"], "sum", E.fwd_ref(op["x"][z], op["w"][z], None, None, dtype=F), op["want"][z])


@pytest.mark.parametrize("c", E.BWD_W_CASES, ids=_ids(E.BWD_W_CASES))
def test_weight_gradient_inputs_carry_the_bar(c):
    op = E.bwd_w_operands(c["name"], "random")
    dw, db = E.bwd_w_ref(op["dy"], op["x"], dtype=F)
    _judge(c["name"], "dw", dw, op["dw"])
    _judge(c["name"], "db", db, op["db"])


@pytest.mark.parametrize("c", E.BWD_X_CASES, ids=_ids(E.BWD_X_CASES))
def test_input_gradient_inputs_carry_the_bar(c):
    op = E.bwd_x_operands(c["name"], "random")
    _judge(c["name"], "dx", E.bwd_x_ref(op["dy"], op["w"], op["xact"], op["mask"], dtype=F), op["dx"])
    if c["mask"] == "relu":
        assert 0.3 < (op["xact"] > 0).mean() < 0.7 or op["xact"].size < 64       # the mask is not all-pass
    if c["mask"] == "tanh":
        assert np.abs(op["xact"]).max() < 1.0


@pytest.mark.parametrize("c", E.XW_CASES, ids=_ids(E.XW_CASES))
def test_pair_inputs_carry_the_bar(c):
    op = E.xw_operands(c["name"], "random")
    dw, db = E.bwd_w_ref(op["dy"], op["x"], dtype=F)
    _judge(c["name"], "dx", E.bwd_x_ref(op["dy"], op["w"], op["x"], "relu" if c["relu"] else None, dtype=F), op["dx"])
    _judge(c["name"], "dw", dw, op["dw"])
    _judge(c["name"], "db", db, op["db"])


@pytest.mark.parametrize("c", E.AUTOGRAD_CASES, ids=_ids(E.AUTOGRAD_CASES))
def test_autograd_inputs_carry_the_bar_and_no_relu_gate_is_ambiguous(c):
    import torch
    op = E.autograd_operands(c["name"])
    assert op["margin"] > E.RELU_MARGIN, "%s: a float64 pre-activation within %g of zero: %g" % (c["name"], E.RELU_MARGIN, op["margin"])
    xt, wt, bt = [torch.tensor(op[k], requires_grad=True) for k in ("x", "w", "b")]
    pre = torch.nn.functional.linear(xt, wt, bt)
    y = torch.relu(pre) if c["act"] == "relu" else torch.tanh(pre) if c["act"] == "tanh" else pre
    y.backward(torch.tensor(op["dy"]))
    dx = xt.grad.numpy() * ((op["x"] > 0) if c["x_relu"] else 1.0)
    for key, got in (("y", y.detach().numpy()), ("dx", dx), ("dw", wt.grad.numpy()), ("db", bt.grad.numpy())):
        assert got.dtype == F or key == "dx"
        _judge(c["name"], key, got, op[key])


@pytest.mark.parametrize("c", E.ACT_BWD_CASES, ids=_ids(E.ACT_BWD_CASES))
def test_act_bwd_reference_is_one_float32_statement(c):
    dy, y, want = E.act_bwd_operands(c["name"])
    assert want.dtype == F and want.shape == (c["n"],) and np.all(np.isfinite(want))
    d64 = dy.astype(np.float64) * (1.0 if c["act"] is None else (y > 0) if c["act"] == "relu" else 1.0 - y.astype(np.float64) ** 2)
    assert _figure(want, d64) <= 1e-6
    if c["act"] is None:
        assert np.array_equal(want, dy)


def test_rows_to_compare_names_both_ends_of_every_block():
    assert E.rows_to_compare(1) == [0] and E.rows_to_compare(32) == [0, 31] and E.rows_to_compare(33) == [0, 31, 32]
    assert E.rows_to_compare(67) == [0, 31, 32, 63, 64, 66]
