"""CPU proof for tests/replay_edge_cases.py (runs everywhere, no GPU), so that a failure of tests/test_gpu_replay_edges.py is a
finding about a kernel and not about the test:

  paths       every case reaches the path it is named for: the launchers' dispatch conditions restated in Python (16-byte or
              byte path, trips of the copy loop and the values its `second` guard takes, the streaming threshold, the grid caps
              of the table kernels, chunks of the row gather, leaves on two depths, the exactness bound
              capacity * hi > 2^(53 + ilogb(lo) - 23), batch + add_n > NT, n_nodes against kTopNodes, an add on a committed
              leaf, a descent that meets s == tree[left])
  references  the numpy references agree with the reference project's own SumTree / UniformReplay (where its tree is
              present) and with the goldens generated from them (tests/golden/sumtree.npz, uniform_replay.npz)
  mutants     for every class of cases a deliberately WRONG restatement differs from the reference on that class's inputs:
              the `second` guard dropped, descent with < for <=, add by recompute instead of delta, action copy capped at 256
              bytes, fold associated as m * (gamma * cum), last writer wins, stratum seg * (i + u)"""
import numpy as np
import pytest

import ref_shim
import replay_edge_cases as E
from golden.make_golden_cases import UNIFORM_CASES, stream
from oracle.replay_oracle import UniformReplayOracle
from oracle.sumtree_oracle import SumTreeOracle


def _ids(cases):
    return [c["name"] for c in cases]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


# ================================================================================================ paths
@pytest.mark.parametrize("case", E.GATHER_CASES, ids=_ids(E.GATHER_CASES))
def test_gather_case_reaches_its_path(case):
    assert case["capacity"] <= 64
    lo, hi = E.index_range(case["capacity"], case["history"], case["n_step"])
    idx = E.gather_indices(case["capacity"], case["history"], case["n_step"], case["batch"], case["seed"])
    assert lo <= idx.min() and idx.max() <= hi and hi == idx[0] and len(idx) == case["batch"]
    assert idx.min() - case["history"] + 1 >= 0 and idx.max() + case["n_step"] <= case["capacity"] - 1
    for block in (False, True):
        d = E.gather_dispatch(case["frame_bytes"], case["history"], case["n_step"], case["batch"], block, not case["misaligned"])
        assert not d["stream"]
        if case["name"].startswith(("vec_", "pairs_vec")):
            assert d["path"] == "vec"
        else:
            assert d["path"] == "byte"
        if case["name"].startswith("vec_"):
            nv = case["frame_bytes"] // 16
            trips, seen_true, seen_false = E.VEC_EXPECT[nv]
            assert (d["trips"], True in d["second"], False in d["second"]) == (trips, seen_true, seen_false), nv
    if case["misaligned"]:
        assert case["frame_bytes"] % 16 == 0
        assert E.gather_dispatch(case["frame_bytes"], case["history"], case["n_step"], case["batch"], False, True)["path"] == "vec"
        assert E.gather_dispatch(case["frame_bytes"], case["history"], case["n_step"], case["batch"], False, False)["byte_trips"] == 16


def test_gather_cases_cover_the_issue():
    vec = sorted(c["frame_bytes"] // 16 for c in E.GATHER_CASES if c["name"].startswith("vec_"))
    assert vec == [1, 255, 256, 257, 511, 512, 513, 1025] and sorted(E.VEC_EXPECT) == vec
    assert sorted(c["frame_bytes"] for c in E.GATHER_CASES if c["name"].startswith("byte_") and not c["misaligned"]) == [1, 15, 17, 255, 257, 513]
    for path in ("pairs_vec", "pairs_byte"):
        assert sorted((c["history"], c["n_step"]) for c in E.GATHER_CASES if c["name"].startswith(path)) == sorted(E._PAIRS)
    assert any(c["batch"] == 1 for c in E.GATHER_CASES) and any(c["batch"] > c["capacity"] for c in E.GATHER_CASES)
    # (2, 5): frames [H, n) of the run belong to neither state nor next_state in the two-tensor form
    assert [j for j in range(2 + 5) if not j < 2 and not j >= 5] == [2, 3, 4]
    assert max(E.gather_dispatch(16 * nv, 1, 1, 1, False)["trips"] for nv in E.VEC_NV) >= 2


def test_streaming_threshold():
    want = {"stream_two_2048": 268697600, "stream_two_2046_below": 268435200, "stream_block_3274": 3274 * 5 * 16400}
    for c in E.STREAM_CASES:
        d = E.gather_dispatch(c["frame_bytes"], c["history"], c["n_step"], c["batch"], c["block"])
        assert d["path"] == "vec" and d["out_bytes"] == want[c["name"]] and d["stream"] == c["stream"], c["name"]
        assert (d["out_bytes"] >= 256 << 20) == c["stream"]
        assert c["capacity"] <= 64
    assert not E.gather_dispatch(16400, 4, 1, 3273, True)["stream"] and E.gather_dispatch(16400, 4, 1, 2047, False)["stream"]


@pytest.mark.parametrize("case", E.FOLD_CASES, ids=_ids(E.FOLD_CASES))
def test_fold_case_has_a_terminal_at_every_position(case):
    n = case["n_step"]
    assert set(E.terminal_positions(case)) == set(range(-1, n))
    r = case["rewards"]
    with np.errstate(over="ignore"):
        not_f32 = r.astype(np.float32).astype(np.float64) != r
    assert not_f32.sum() >= len(r) - 6
    assert np.signbit(r[r == 0.0]).all() and (r == 0.0).sum() == 3 and (r == 1e300).any() and (r == -1e300).any()
    lo, hi = E.index_range(case["capacity"], 1, n)
    assert case["idx"].min() == lo and case["idx"].max() == hi


def test_fold_cases_cover_the_issue():
    plain = [c for c in E.FOLD_CASES if not c["name"].endswith("_wide")]
    assert sorted((c["n_step"], c["discount"]) for c in plain) == sorted((n, g) for n in range(1, 6) for g in (0.0, 1.0, 0.99))
    assert all(set(np.unique(c["masks"])) <= {0, 1} for c in plain)


def test_table_kernel_cases_reach_the_grid_caps():
    assert E.LUT_N[:5] == [1, 15, 16, 17, 4097] and E.LUT_N[5] == 16 * (2048 * 256) + 16 + 5
    d = [E.lut_blocks(n) for n in E.LUT_N]
    assert [x["trips"] for x in d] == [0, 0, 1, 1, 1, 2] and [x["tail"] for x in d] == [1, 15, 0, 1, 1, 5]
    assert [x["capped"] for x in d] == [False] * 5 + [True] and d[5]["blocks"] == 2048 and d[0]["blocks"] == 1
    for n in E.LUT_N:
        if n >= 256:
            assert len(np.unique(E.lut_input(n))) == 256
    big, small = (E.lut_rows_blocks(c["rows"], c["elems"]) for c in E.LUT_ROWS)
    assert big["vectors"] == 1054720 > 4096 * 256 and big["capped"] and big["blocks"] == 4096 and big["trips"] == 2
    assert not small["capped"] and small["vectors"] == 3
    for c in E.LUT_ROWS:
        assert c["stride"] % 16 == 0 and c["stride"] >= c["elems"] and c["elems"] % 16 == 0


def test_gather_rows_cases():
    d = {rb: E.gather_rows_dispatch(rb) for rb in E.GATHER_ROWS_BYTES}
    assert [d[rb]["chunks"] for rb in (4096, 4097, 4112, 8192)] == [1, 2, 2, 2]
    assert [d[rb]["vec"] for rb in (4096, 4097, 4112, 8192)] == [True, False, True, True]
    assert d[4097]["byte_trips"] == 16 and E.gather_rows_dispatch(4096, aligned=False)["byte_trips"] == 16
    assert min(E.GATHER_ROWS_IDX) == -E.GATHER_ROWS_SRC and max(E.GATHER_ROWS_IDX) == E.GATHER_ROWS_SRC - 1


def test_tree_capacities_and_depths():
    assert E.TREE_CAPS == [1, 2, 3, 5, 7, 8, 9, 1000, 1023, 1024, 1025]
    for cap in E.TREE_CAPS:
        two = len(E.leaf_depths(cap)) == 2
        assert two == (cap & (cap - 1) != 0), cap
    ucases = E.update_cases()
    assert [n for c, n in ucases if c == 1025] == [65, 1024]
    assert all(n == c for c, n in ucases if c <= 1024) and sorted(c for c, n in ucases if c <= 1024) == E.TREE_CAPS[:-1]
    # small trees with leaves on two depths where ALL leaves change in one launch
    assert any(n == c and len(E.leaf_depths(c)) == 2 and c < 10 for c, n in ucases)
    for cap, n in ucases:
        leaves, prio = E.update_inputs(cap, n, ordered=False)
        assert len(set(leaves.tolist())) == n and leaves.min() >= cap - 1 and leaves.max() <= 2 * cap - 2
        assert np.array_equal(prio.astype(np.float32).astype(np.float64), prio)
        init = E.filled_oracle(cap, cap).tree[cap - 1:]
        assert E.exact_regime(cap, max(prio.max(), init.max()), min(prio.min(), init.min()))
        _, wide = E.update_inputs(cap, n, ordered=True)
        if n >= 8:
            assert not E.exact_regime(cap, wide.max(), wide.min())
    for cap in E.TREE_CAPS:
        write0, n = E.many_add_plan(cap)
        assert 0 <= write0 < cap and 1 <= n <= 64 and n <= cap and (cap == 1 or write0 + n > cap)
        assert n == (64 if cap >= 64 else cap)


def test_exactness_bound_restated():
    # capacity * hi > 2^(53 + ilogb(lo) - 23), at the bound and on either side of it
    assert E.exact_regime(1 << 10, 1.0, 2.0 ** -20) and not E.exact_regime((1 << 10) + 1, 1.0, 2.0 ** -20)
    assert E.exact_regime(1 << 10, 1.0, 1.9 * 2.0 ** -20) and not E.exact_regime(1 << 10, 1.0, 2.0 ** -20 * (1 - 2.0 ** -30))
    assert not E.exact_regime(8, 1.0, 0.0) and not E.exact_regime(8, np.inf, 1.0)


@pytest.mark.parametrize("cap", E.FALLBACK_CAPS)
def test_fallback_rounds_leave_the_exact_regime(cap):
    hi, lo = 1.0, 1.0
    for k, (leaves, prio) in enumerate(E.fallback_rounds(cap)):
        assert len(set(leaves.tolist())) == len(leaves)
        hi, lo = max(hi, float(prio.max())), min(lo, float(prio.min()))
        assert not E.exact_regime(cap, hi, lo), k
    assert lo < 2.0 ** -30 and hi > 2.0 ** 15


def test_sample_cases_meet_ties_and_zero_leaves():
    trees = E.sample_trees()
    assert E.SAMPLE_BATCHES == [1, 63, 64, 65, 1024]
    for b in E.SAMPLE_BATCHES:
        t = trees["ones%d" % b]
        r = E.ref_sample(t, np.zeros(b))
        if b > 1:
            assert r["ties"] >= 1, b          # at least one descent meets s == tree[left]
    for cap in (1000, 1025):
        t = trees["zeros_interleaved%d" % cap]
        leaves = t[cap - 1:]
        assert (leaves == 0).sum() >= cap // 2 and (leaves > 0).sum() >= cap // 2 - 1
        for b in E.SAMPLE_BATCHES:
            for u in E.sample_us(b, 1).values():
                r = E.ref_sample(t, u)
                assert (r["p"][E.strata(t[0], b, u) > 0.0] > 0).all()       # never a zero-priority leaf (s = 0 takes the leftmost)
    r = E.ref_sample(trees["all_zero9"], np.zeros(5))
    assert r["total"] == 0.0 and (r["p"] == 0).all()
    assert E.U_TOP < 1.0 and E.U_TOP == np.nextafter(1.0, 0.0)


@pytest.mark.parametrize("case", E.PER_CASES, ids=_ids(E.PER_CASES))
def test_per_case_reaches_its_branch(case):
    assert 6 <= case["rounds"] <= 12
    run = E.PerRun(case)
    outs = []
    for r in range(case["rounds"]):
        inp = run.begin()
        outs.append(run.finish(E.ref_priorities(inp["loss"], case["eps"], case["alpha"])))
    name = case["name"]
    final = case.get("final")
    body = outs[:-1] if final else outs
    assert all(o["n_valid"] >= 1 and o["flags"] == 0 for o in body), [o["n_valid"] for o in outs]
    want = "ordered" if "unforced_ordered" in name else ("level" if "level_by_level" in name else "atomic")
    assert all(o["branch"] == want for o in outs), [o["branch"] for o in outs]
    if want == "level":
        assert case["batch"] + case["add_n"] > E.NT
    if want == "ordered":
        assert case["eps"] == 0.0 and case["add_n"] > 0
        loss = np.abs(E.per_losses(case, np.random.RandomState(0), 0))
        assert loss.min() <= 1e-30 * 1.001 and loss.max() >= 1e6 * 0.999
    if case["collide"]:
        assert sum(1 for o in outs if o["collisions"]) >= 2
    if "duplicates" in name:
        assert case["cap"] < case["batch"] and all(o["duplicates"] > 0 for o in outs)
    if "top_exact" in name:
        assert 2 * case["cap"] - 1 == E.K_TOP_NODES
    if "top_plus2" in name:
        assert 2 * case["cap"] - 1 == E.K_TOP_NODES + 2
    if final == "dry":
        assert outs[-1]["flags"] & 1
    if final == "no_valid":
        assert outs[-1]["flags"] == 2 and outs[-1]["n_valid"] == 0
        assert set(outs[-1]["idx"]) == {case["cap"] - 1 + case["history"]} and case["history"] < case["cap"]


def test_per_cases_cover_the_issue():
    got = {(c["cap"], c["batch"], c["add_n"]) for c in E.PER_CASES}
    assert {(300, 1, 1), (300, 8, 0), (300, 9, 4), (8, 32, 2), (1024, 64, 8), (1025, 64, 8), (4096, 1024, 0), (4096, 1024, 8)} <= got
    assert any(c["alpha"] == 0.7 for c in E.PER_CASES) and any(c["collide"] for c in E.PER_CASES)
    assert {c.get("final") for c in E.PER_CASES} >= {"dry", "no_valid"}


# ================================================================================================ references
def test_descent_and_gather_agree_with_the_goldens(golden):
    g = golden("sumtree")
    for cap in (8, 13, 50):
        tree = SumTreeOracle(cap)
        for op, x, p_out, idx in g["cap%d_log" % cap]:
            op, idx = int(op), int(idx)
            if op == 0:
                tree.add(np.float32(x))
            elif op == 1:
                leaf, _ = E.descend(tree.tree, x)
                assert leaf == idx and tree.tree[leaf] == p_out
                tree.get(x)
            else:
                tree.update(idx, np.float32(x))
        assert np.array_equal(tree.tree, g["cap%d_tree" % cap])
    g = golden("uniform_replay")
    for name, mem, b, h, n, disc, shape, kind, t_len, cps in UNIFORM_CASES:
        if kind != "u8":
            continue
        states, actions, rewards, masks = stream(np.random.RandomState(1000 + ord(name)), t_len, shape, kind, 4, 0.1)
        rep = UniformReplayOracle(mem, b, n, disc, h)
        for t in range(t_len):
            rep.feed_one(states[t], actions[t], rewards[t], masks[t])
            if t in cps:
                k = "%s_t%d_" % (name, t)
                c = E.RingContents(mem, int(np.prod(shape)), 8, 0, rewards=rep.reward, masks=rep.mask)
                c.frames = rep.state.reshape(mem, -1).copy()
                c.actions = rep.action.astype("<i8").view(np.uint8).reshape(mem, 8)
                want = E.ref_gather(c, g[k + "idx"], h, n, disc)
                assert np.array_equal(want["state"].reshape(g[k + "state"].shape), g[k + "state"])
                assert np.array_equal(want["next_state"].reshape(g[k + "next_state"].shape), g[k + "next_state"])
                assert np.array_equal(_bits(want["reward"]), _bits(g[k + "reward"])) and np.array_equal(want["mask"], g[k + "mask"])
                assert np.array_equal(want["action"].view("<i8").ravel(), g[k + "action"])


needs_reference = pytest.mark.skipif(not ref_shim.available(), reason="the reference tree is not on this machine")


@needs_reference
@pytest.mark.parametrize("cap", [c for c in E.TREE_CAPS if 2 <= c <= 9] + E.FALLBACK_CAPS[:1])
def test_tree_references_agree_with_the_reference_sumtree(cap):
    ref = ref_shim.load()
    rt, orc, plain = ref.SumTree(cap), E.TreeRef(cap), SumTreeOracle(cap)
    rs = np.random.RandomState(cap)
    bare = np.zeros(2 * cap - 1)
    for p in E.f32_priorities(rs, cap + 3):
        leaf = orc.write + cap - 1
        rt.add(float(p), None)
        orc.add(float(p))
        plain.add(float(p))
        E.delta_add(bare, leaf, float(p))
        assert np.array_equal(_bits(rt.tree), _bits(orc.tree)) and np.array_equal(_bits(bare), _bits(orc.tree))
        assert np.array_equal(_bits(plain.tree), _bits(orc.tree))
    # wide float64 priorities in the reference's own order, then adds: the delta walk is the reference's add
    leaves, prio = E.update_inputs(cap, cap, ordered=True)
    for leaf, p in zip(leaves, prio):
        rt.pending_idx.add(int(leaf))
        rt.update(int(leaf), float(p))
    E.oracle_updates(orc, leaves, prio)
    assert np.array_equal(_bits(rt.tree), _bits(orc.tree))
    bare = orc.tree.copy()
    for _ in range(3):
        leaf = orc.write + cap - 1
        rt.add(float(prio.max()), None)
        orc.add(float(prio.max()))
        E.delta_add(bare, leaf, float(prio.max()))
    assert np.array_equal(_bits(rt.tree), _bits(orc.tree)) and np.array_equal(_bits(bare), _bits(orc.tree))
    for u in E.sample_us(7, cap)["mix"]:
        s = u * rt.total()
        assert rt.get(s)[0] == E.descend(orc.tree, s)[0]


def _reference_replay(ref, c, history, n_step, discount):
    rep = ref.UniformReplay(memory_size=c.capacity, batch_size=1, n_step=n_step, discount=discount, history_length=history)
    for t in range(c.capacity):
        rep.feed(dict(state=c.frames[t][None], action=c.actions[t].view("<i8")[:1] if c.action_bytes == 8 else [c.actions[t]],
                      reward=[c.rewards[t]], mask=c.masks[t:t + 1]))
    return rep


@needs_reference
@pytest.mark.parametrize("case", [c for c in E.GATHER_CASES if c["frame_bytes"] <= 48] + E.FOLD_CASES,
                         ids=_ids([c for c in E.GATHER_CASES if c["frame_bytes"] <= 48] + E.FOLD_CASES))
def test_gather_reference_agrees_with_the_reference_replay(case):
    ref = ref_shim.load()
    c = E.RingContents(case["capacity"], case["frame_bytes"], case["action_bytes"], case["seed"], case.get("rewards"), case.get("masks"))
    h, n = case["history"], case["n_step"]
    rep = _reference_replay(ref, c, h, n, case["discount"])
    idx = case["idx"] if "idx" in case else E.gather_indices(case["capacity"], h, n, case["batch"], case["seed"])
    want = E.ref_gather(c, idx, h, n, case["discount"])
    for b, i in enumerate(idx):
        if not rep.valid_index(int(i)):
            # the reference refuses an index whose run touches the write head (pos = 0 after `capacity` feeds): only i + n <
            # size matters here and that is our range
            continue
        tr = rep.construct_transition(int(i))
        assert np.array_equal(np.asarray(tr.state).reshape(h, -1), want["state"][b])
        assert np.array_equal(np.asarray(tr.next_state).reshape(h, -1), want["next_state"][b])
        assert np.array_equal(_bits(tr.reward), _bits(want["reward"][b])) and int(tr.mask) == int(want["mask"][b])
    assert sum(rep.valid_index(int(i)) for i in idx) >= max(1, len(idx) - 2 * sum(int(i) == idx[0] for i in idx))


# ================================================================================================ mutants
def _copy_loop(src, nv, guard=True):
    """The 16-byte copy loop of ring_gather_kernel over ONE frame of nv vectors, into a buffer with 256 vectors of 0xA5
    behind it.  src: [nv + 512, 16] (what lies behind the frame in the ring).  guard=False: `second` taken as true."""
    out = np.full((nv + 512, 16), E.SLACK_BYTE, dtype=np.uint8)
    for lane in range(E.WG):
        t = lane
        while t < nv:
            t2 = t + E.WG
            second = (t2 < nv) if guard else True
            out[t] = src[t]
            if second:
                out[t2] = src[t2]
            t += 2 * E.WG
    return out


@pytest.mark.parametrize("nv", [nv for nv in E.VEC_NV if E.VEC_EXPECT[nv][2]])
def test_mutant_second_guard_dropped(nv):
    """Over the sizes at which some lane meets second == false (512, where every lane's second vector exists, has nothing
    to guard: it is a path case only)."""
    rs = np.random.RandomState(nv)
    src = rs.randint(0, 256, size=(nv + 512, 16)).astype(np.uint8)
    src[src == E.SLACK_BYTE] = 0
    right, wrong = _copy_loop(src, nv), _copy_loop(src, nv, guard=False)
    assert np.array_equal(right[:nv], src[:nv]) and (right[nv:] == E.SLACK_BYTE).all()
    # some lane meets second == false: without the guard it writes behind the frame
    assert not np.array_equal(right, wrong)
    assert (wrong[nv:] != E.SLACK_BYTE).any() and np.array_equal(wrong[:nv], src[:nv])


def test_mutant_descent_strict_comparison():
    trees = E.sample_trees()
    for b in E.SAMPLE_BATCHES[1:]:
        t = trees["ones%d" % b]
        u = np.zeros(b)
        assert not np.array_equal(E.ref_sample(t, u)["idx"], E.ref_sample(t, u, strict=True)["idx"]), b


def _after_fallback(cap):
    orc = E.filled_oracle(cap, cap)
    hi = float(orc.tree[cap - 1:].max())
    for leaves, prio in E.fallback_rounds(cap):
        E.oracle_updates(orc, leaves, prio.astype(np.float64))
        hi = max(hi, float(prio.max()))
    return orc, hi


@pytest.mark.parametrize("cap", E.FALLBACK_CAPS)
def test_mutant_add_by_recompute(cap):
    orc, hi = _after_fallback(cap)
    assert not np.array_equal(orc.tree, orc.rebuilt())          # the ordered rounds left the heap off left + right
    write0, n = E.fallback_many_add(cap)
    assert write0 + n > cap and n < cap
    # the three feeds of the GPU test, each from the same post-fallback tree: one add (set / set_from), n adds (set_many_from)
    for leaves in ([cap - 1], [(write0 + k) % cap + cap - 1 for k in range(n)]):
        right, wrong = orc.tree.copy(), orc.tree.copy()
        for leaf in leaves:
            E.delta_add(right, leaf, hi)
            E.recompute_add(wrong, leaf, hi)
        assert not np.array_equal(_bits(right), _bits(wrong)), leaves[:3]


@pytest.mark.parametrize("case", [c for c in E.PER_CASES if "unforced_ordered" in c["name"]],
                         ids=_ids([c for c in E.PER_CASES if "unforced_ordered" in c["name"]]))
def test_mutant_per_chain2_adds_by_recompute(case):
    right, wrong = E.PerRun(case), E.PerRun(case, recompute_adds=True)
    differs = False
    for r in range(case["rounds"]):
        prio = E.ref_priorities(right.begin()["loss"], case["eps"], case["alpha"])
        wrong.begin()
        differs = differs or not np.array_equal(_bits(right.finish(prio)["tree"]), _bits(wrong.finish(prio)["tree"]))
        if differs:
            break
    assert differs


def test_mutant_action_copy_capped_at_256_bytes():
    for ab in E.PUT_ACTION_BYTES:
        c = E.RingContents(E.PUT_CAP, 16, ab, ab)
        stored = np.zeros_like(c.actions)
        stored[:, :256] = c.actions[:, :256]         # one lane per byte of a 256-thread workgroup, no loop
        assert np.array_equal(stored, c.actions) == (ab <= 256), ab
    assert max(E.PUT_ACTION_BYTES) == 264 and 256 in E.PUT_ACTION_BYTES


def _fold_wrong(rewards, masks, i, n, discount):
    cum_r = 0.0
    for k in range(n - 1, -1, -1):
        cum_r = float(rewards[i + k]) + int(masks[i + k]) * (float(discount) * cum_r)
    return cum_r


def test_mutant_fold_association():
    wide = [c for c in E.FOLD_CASES if c["name"].endswith("_wide")]
    assert sorted(c["n_step"] for c in wide) == [2, 3, 4, 5]
    for c in wide:
        right = [E.fold(c["rewards"], c["masks"], int(i), c["n_step"], c["discount"])[0] for i in c["idx"]]
        wrong = [_fold_wrong(c["rewards"], c["masks"], int(i), c["n_step"], c["discount"]) for i in c["idx"]]
        assert not np.array_equal(_bits(right), _bits(wrong)), c["name"]


def test_mutant_last_writer_wins():
    case = [c for c in E.PER_CASES if "duplicates" in c["name"]][0]
    right, wrong = E.PerRun(case), E.PerRun(case, last_writer=True)
    prio = E.ref_priorities(right.begin()["loss"], case["eps"], case["alpha"])
    wrong.begin()
    assert not np.array_equal(_bits(right.finish(prio)["tree"]), _bits(wrong.finish(prio)["tree"]))


def test_mutant_stratum_formula():
    t = E.sample_trees()["ones_cap1000"]
    for b in (63, 65):
        u = E.boundary_us(t[0], b)
        assert not np.array_equal(E.ref_sample(t, u)["idx"], E.ref_sample(t, u, wrong_strata=True)["idx"]), b
