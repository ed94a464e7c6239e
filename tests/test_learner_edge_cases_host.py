"""CPU proofs about tests/learner_edge_cases.py, before anything runs on a GPU: the case matrix is the one that stands on both
sides of every switch of csrc/learner.hip; every case's first update has a float64 ReLU margin of at least 5e-7; the float32 CPU
run of the reference meets every bar against the float64 one on every case's inputs (the inputs carry the bar); the expected path
flags follow from the library's conditions; the double-Q cases have rows whose online and target argmax differ; the action cases
store actions 0 and A - 1; no case's minibatches are free of terminal (or of non-terminal) transitions."""
import numpy as np
import pytest
import torch

import fake_envs
import learner_edge_cases as E
from oracle import net_oracle as N, numerics_oracle as NUM


def _ids(cases):
    return [c["name"] for c in cases]


def test_case_matrix_is_the_issues():
    shape = lambda c: (c["B"], c["A"]) + ((c["atoms"],) if c["head"] != "vanilla" else ())
    sel = lambda f: sorted(shape(c) for c in E.IN_ORDER_CASES if f(c))
    assert sel(lambda c: c["head"] == "vanilla" and not c["double_q"] and c["A"] == 4) == [(b, 4) for b in (1, 5, 16, 17, 24, 31, 33, 40, 128)]
    assert sel(lambda c: c["head"] == "vanilla" and not c["double_q"] and c["A"] != 4) == [(17, a) for a in (1, 3, 8, 9, 18, 64)]
    assert sel(lambda c: c["head"] == "vanilla" and c["double_q"]) == sorted([(17, 5), (17, 6), (32, 64), (5, 18)])
    assert sel(lambda c: c["head"] == "c51") == sorted([(5, 3, 51), (17, 18, 51), (32, 64, 64), (7, 4, 2), (17, 6, 51)])
    assert [c["name"] for c in E.IN_ORDER_CASES if c["head"] == "c51" and c["double_q"]] == ["c51-double-q-batch17-actions6"]
    assert sel(lambda c: c["head"] == "qr") == sorted([(7, 6, 200), (40, 2, 8), (3, 20, 200)])
    assert sorted((c["B"], c["A"]) for c in E.PIPELINED_CASES) == sorted([(17, 4), (24, 4), (31, 4), (32, 1), (32, 9), (32, 18), (17, 64), (33, 4)])
    assert sorted(c["A"] for c in E.IN_ORDER_CASES if c["actor"] and c["head"] == "vanilla") == [1, 9, 18, 64]
    for head in ("c51", "qr"):      # the actor on the largest head of each kind
        big = max((c for c in E.IN_ORDER_CASES if c["head"] == head), key=lambda c: c["n_out"])
        assert big["actor"] and [c["name"] for c in E.IN_ORDER_CASES if c["head"] == head and c["actor"]] == [big["name"]]
    assert max(c["n_out"] for c in E.IN_ORDER_CASES) == 4096
    # every update but batch 128's fourth: capture, two replays, one eager
    assert all(c["updates"] == 4 for c in E.IN_ORDER_CASES if c["B"] != 128) and E.by_name("batch128-throughput-shape")["updates"] == 3
    assert len({c["name"] for c in E.IN_ORDER_CASES + E.PIPELINED_CASES}) == len(E.IN_ORDER_CASES) + len(E.PIPELINED_CASES)
    assert E.CAP <= 512 and not E.BAR_OVERRIDES        # (an override needs its float32 figure beside it: see the module's docstring)


@pytest.mark.parametrize("c", E.IN_ORDER_CASES, ids=_ids(E.IN_ORDER_CASES))
def test_first_update_is_unambiguous_and_float32_meets_the_bar(c):
    wide, narrow = E.first_update(c["name"], True), E.first_update(c["name"], False)
    assert wide["margin"] >= E.MARGIN, "float64 ReLU margin %g of the first update" % wide["margin"]
    fig = E.measure(c, narrow, wide, with_state=True)
    assert {k.split(":")[0] for k in fig} == {"out", "vec", "loss", "norm", "params", "state1", "state2", "grad"}
    E.judge(c, fig, False, "float32 on the CPU against float64")
    # the first update means something: a gradient everywhere, and both forms of the clip among the cases (below)
    assert all(float(np.abs(g).max()) > 0 for g in wide["grads"].values()) and wide["norm"] > 0 and np.isfinite(wide["loss"])
    n_vec = c["atoms"] if c["head"] == "qr" else c["B"]
    assert wide["vec"].shape == (n_vec,) and wide["out"].size == c["B"] * c["n_out"]


def test_clip_is_active_in_some_cases_and_idle_in_others():
    clipped = [E.first_update(c["name"], True)["clipped"] for c in E.IN_ORDER_CASES]
    assert any(clipped) and not all(clipped)


def _pipe_first(c):
    """The pipelined case's schedule up to its first update, in float64: (the state before it, its minibatch, the oracle)."""
    p0 = fake_envs.numpy_params(fake_envs.nature_vanilla_shapes(c["A"]), E.PARAM_SEEDS[0])
    orc = E.schedule_oracle(c, p0)
    keep = np.random.get_state()
    try:
        np.random.seed(c["draw_seed"])
        orc.actor_step(orc._snapshot())
        idx, batch = orc.sample()
    finally:
        np.random.set_state(keep)
    state = dict(params=p0, target=p0, state1={k: np.zeros_like(v) for k, v in p0.items()}, state2={k: np.zeros_like(v) for k, v in p0.items()})
    return state, batch, orc


@pytest.mark.parametrize("c", E.PIPELINED_CASES, ids=_ids(E.PIPELINED_CASES))
def test_pipelined_first_update_is_unambiguous_and_float32_meets_the_bar(c):
    state, batch, orc = _pipe_first(c)
    wide = E.reference_update(c, state, batch, 1)
    narrow = E.reference_update(c, state, batch, 1, torch.float32)
    assert wide["margin"] >= E.MARGIN, "float64 ReLU margin %g of the first update" % wide["margin"]
    E.judge(c, E.measure(c, narrow, wide, with_state=True), False, "float32 on the CPU against float64")
    assert batch[4].min() == 0 and batch[4].max() == 1, "terminal and non-terminal transitions in the first minibatch"
    # the schedule oracle's own float64 update is the same update by another route (its hyperparameters are not rounded to
    # float32 first: 1e-8 relative)
    loss, delta, q, norm = orc.update(batch)
    assert delta.dtype == np.float64 and orc.relu_margin == wide["margin"]
    np.testing.assert_allclose(q, wide["out"], rtol=0, atol=1e-7 * np.abs(wide["out"]).max())
    np.testing.assert_allclose(delta, wide["vec"], rtol=0, atol=1e-7 * np.abs(wide["vec"]).max())
    np.testing.assert_allclose([loss, norm], [wide["loss"], wide["norm"]], rtol=1e-7)
    for k, v in wide["params"].items():
        np.testing.assert_allclose(orc.p[k].detach().numpy(), v, rtol=1e-7, atol=1e-9, err_msg=k)


def test_expected_flags_follow_from_the_librarys_conditions():
    from deeprl_amd import ops
    default = ops.get_tuning()
    # the bits the conditions of csrc/learner.hip ask for are the library default's; the opt-in chains are not
    need = (E.V_FUSED_BWD | E.V_ONESHOT_DGRAD | E.V_ONESHOT_FWD | E.V_ONESHOT_WGRAD | E.V_PINNED_IDX | E.V_ACTOR_PARAMS | E.V_PIPE_GATHER |
            E.V_ACTOR_RING | E.V_ACTOR_FUSED_CONV1 | E.V_GATHER_ON_UPDATE | E.V_RING_DIRECT | E.V_LATE_FOLD | E.V_ACTOR_MEGA | E.V_DEFER_FC4 |
            E.V_ACTOR_PERSIST | E.V_FWD_CHAIN | E.V_BWD_CHAIN | E.V_FLAG_SYNC | E.V_LANE_EAGER)
    assert default & need == need and not default & (E.V_HEAD_CHAIN | E.V_TARGET_AHEAD | E.V_BWD_CHAIN_FC | E.V_ACTOR_V3 | E.V_GATHER_IN_GRAPH)
    for name in ("FUSED_BWD", "ONESHOT_DGRAD", "ONESHOT_FWD", "ONESHOT_WGRAD", "PINNED_IDX", "ACTOR_PARAMS", "PIPE_GATHER", "ACTOR_V3",
                 "GATHER_IN_GRAPH", "ACTOR_RING", "ACTOR_FUSED_CONV1", "GATHER_ON_UPDATE", "RING_DIRECT", "HEAD_CHAIN", "LATE_FOLD",
                 "ACTOR_MEGA", "DEFER_FC4", "ACTOR_PERSIST", "FWD_CHAIN", "BWD_CHAIN", "FLAG_SYNC", "LANE_EAGER", "TARGET_AHEAD", "BWD_CHAIN_FC"):
        assert getattr(E, "V_" + name) == getattr(ops, "VAR_" + name), name
    for c in E.IN_ORDER_CASES + E.PIPELINED_CASES:
        pipelined = "draw_seed" in c
        got = E.expected_flags(c, default & ~ops.VAR_CU_PARTITION, pipelined)
        for k, v in c["reaches"].items():
            assert got[k] == v, "%s is named for %s = %s, the conditions give %s" % (c["name"], k, v, got[k])
        assert not any(E.expected_flags(c, 0, pipelined).values()), "variant 0 takes none of the paths"
        # the late fold's condition on the slabs: the one-pass conv2 / conv3 weight gradients write at most 32 of them
        slabs = [ops.conv_wgrad_slabs(layer, c["B"], 16, default) for layer in (2, 3)]
        assert (max(slabs) <= 32) == (c["B"] <= 32), (c["name"], slabs)
        lo, hi = E.late_partials(c)
        assert got["late"] == (c["B"] <= 32 and hi <= E.LATE_PARTIALS_MAX)
        if pipelined:
            assert c["chained"] == (got["fchain"] and got["bchain"] and got["fs"]) and c["head"] == "vanilla" and not c["double_q"]
            opt_in = E.expected_flags(c, default | E.V_HEAD_CHAIN | E.V_TARGET_AHEAD, True)
            assert opt_in["head_chain"] == opt_in["ah"] == c["chained"] and not (opt_in["head_chain"] and opt_in["head_pf"])
            cleared = E.expected_flags(c, default & ~E.CHAIN_BITS, True)
            assert not any(cleared[k] for k in ("defer", "fchain", "bchain", "fs", "ah", "head_chain"))
    # both sides of every switch the query can see, at the library default
    f = lambda name, pipelined=False: E.expected_flags(E.by_name(name), default, pipelined)
    assert not f("batch16-last-small-conv-shape")["fchain"] and f("batch17-first-chained-batch")["fchain"]
    assert f("batch31-head-wgrad-remainder")["late"] and not f("batch33-late-fold-off")["late"]
    assert f("batch24-w4-prefetch-on")["head_pf"] and not f("batch17-first-chained-batch")["head_pf"]
    assert f("batch17-first-chained-batch")["defer"] and not f("batch16-last-small-conv-shape")["defer"] and not f("batch33-late-fold-off")["defer"]
    assert f("c51-batch17-actions18")["late"] and not f("c51-batch32-actions64-atoms64-n-out-limit")["late"]
    assert not f("double-q-actions5-head-weights-in-registers")["fchain"]
    # ... and the head's register / fallback switch (not a flag: nz * A <= 16)
    reg = E.head_weights_in_registers
    assert reg(E.by_name("actions8-head-weights-in-registers")) and not reg(E.by_name("actions9-head-fallback-loop"))
    assert reg(E.by_name("double-q-actions5-head-weights-in-registers")) and not reg(E.by_name("double-q-actions6-head-fallback-loop"))
    assert reg(E.by_name("batch17-first-chained-batch")) and not reg(E.by_name("pipe-batch32-actions9-head-fallback-loop"))


def test_double_q_cases_have_rows_whose_online_and_target_argmax_differ():
    for c in E.DOUBLE_Q_CASES:
        s0 = E.initial_state(c)
        ns = E.gather(c, E.case_indices(c)[0])[3]
        xn = torch.from_numpy(NUM.image_normalize_sync(ns)).double()
        with torch.no_grad():
            on, tg = ({k: torch.from_numpy(v).double() for k, v in s0[w].items()} for w in ("params", "target"))
            a_on = E.action_values(c, on, N.nature_conv_body(on, xn)).argmax(-1)
            a_tg = E.action_values(c, tg, N.nature_conv_body(tg, xn)).argmax(-1)
        assert int((a_on != a_tg).sum()) >= 1, c["name"]


def test_minibatches_hold_the_actions_and_terminals_the_cases_need():
    for c in E.IN_ORDER_CASES:
        batches = [E.gather(c, idx) for idx in E.case_indices(c)]
        assert len(batches) == c["updates"] and all(len(b[1]) == c["B"] for b in batches)
        masks = np.concatenate([b[4] for b in batches])
        actions = np.concatenate([np.asarray(b[1]).reshape(-1) for b in batches])
        assert masks.min() == 0 and masks.max() == 1, "%s: terminal and non-terminal transitions" % c["name"]
        if c["B"] >= 5:
            assert batches[0][4].min() == 0 and batches[0][4].max() == 1, "%s: ... in the first minibatch" % c["name"]
        assert actions.min() >= 0 and actions.max() < c["A"]
        if c in E.ACTION_CASES or c["A"] > 4:
            assert actions.min() == 0 and actions.max() == c["A"] - 1, "%s: stored actions 0 and A - 1" % c["name"]
        # the ring-wrapping stack of the actor check and the draws stay inside the ring
        assert all(3 <= i < E.CAP - 1 for idx in E.case_indices(c) for i in idx)


def test_the_bar_notices_a_wrong_gradient_element_and_a_wrong_sample():
    """What the suite is for: ONE gradient element with the wrong sign (the optimizer state after the first update is a multiple of
    the gradient: a centered RMSprop step alone is nearly a sign function of it), one sample's gradient left out, one head output
    of one sample off by 1e-4 -- each is beyond the bar although the float32 run itself is within it."""
    c = E.by_name("batch17-first-chained-batch")
    wide, narrow = E.first_update(c["name"], True), E.first_update(c["name"], False)
    E.judge(c, E.measure(c, narrow, wide, True), False, "float32")

    def altered(key, name, f):
        got = dict(narrow)
        got[key] = dict(got[key]) if name else got[key]
        if name:
            got[key][name] = f(got[key][name].copy())
        else:
            got[key] = f(got[key].copy())
        return got

    def flip(a):
        i = np.unravel_index(np.argsort(np.abs(a).ravel())[a.size // 2], a.shape)      # a median-sized element, not the largest
        a[i] = -a[i]
        return a

    for name in ("body.conv1.weight", "body.fc4.weight", "fc_head.bias"):
        with pytest.raises(AssertionError, match="state2:" + name.replace(".", r"\.")):
            E.judge(c, E.measure(c, altered("state2", name, flip), wide, True), False, "one sign flipped")
    with pytest.raises(AssertionError, match="state2:body.conv2.weight"):      # 16 of 17 samples: the slab of one left out of the fold
        E.judge(c, E.measure(c, altered("state2", "body.conv2.weight", lambda a: a * (16.0 / 17.0)), wide, True), False, "a sample short")
    with pytest.raises(AssertionError, match="out"):
        E.judge(c, E.measure(c, altered("out", None, lambda a: a + 1e-4 * (np.arange(a.size).reshape(a.shape) == 5)), wide, True), False, "one q off")
