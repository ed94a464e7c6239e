"""CPU proofs about tests/a2c_mlp_edge_cases.py, before anything runs on a GPU: every rollout case is inside the kernel's supported
range and reaches the path it is named for (instantiation, row-block geometry, fold path, clip, terminals, the environment's action
clamp); the float32 CPU run of the reference stays within 0.3 x every bar against the float64 run (the inputs carry the bars); the
head cases reach the saturated tanh and both sides of softplus's threshold; the restatement's new keywords leave its defaults as
they were."""
import numpy as np
import pytest
import torch

import a2c_mlp_cases as K
import a2c_mlp_edge_cases as E
import a2c_mlp_restatement as R

_IDS = [E.case_id(c) for c in E.ROLLOUT_CASES]


# ------------------------------------------------------------------------------------------------ the tables
def test_rollout_table_is_the_stated_one_and_inside_the_supported_range():
    assert E.ROLLOUT_CASES == ((64, 2, 64, 16, 64, "tanh", "meanstd-update", 2, 10.0),
                               (33, 3, 3, 1, 32, "relu", "meanstd-readonly", 2, 0.5),
                               (9, 2, 1, 16, 64, "tanh", "identity", 1, float("inf")),
                               (63, 1, 64, 1, 32, "tanh", "meanstd-update", 5, 0.5),
                               (1, 40, 2, 16, 32, "relu", "meanstd-update", 3, 10.0),
                               (17, 6, 64, 16, 32, "relu", "meanstd-update", 3, 1.0))
    assert E.HEAD_CASES == ((257, 3), (320, 6), (1000, 64), (300, 1))
    assert E.REWARD_COEF == 0.1 and E.PRE_STEP_PERIOD == 3
    assert not E.BAR_OVERRIDES and all(g in E.BAR_GROUPS for _, g in E.BAR_OVERRIDES)
    for c in E.ROLLOUT_CASES:
        assert E.supported(c[2], c[3], c[4], c[0], E.GATE_CODES[c[5]]), c
    # the corner: the largest request the launcher ever makes of dra_grant_lds, and nothing past it is supported
    assert E.rollout_lds_bytes(64, 16, 64, 64) == 158692 <= E.LDS_BYTES_MAX
    assert max(E.rollout_lds_bytes(c[2], c[3], c[4], c[0]) for c in E.ROLLOUT_CASES) == 158692
    assert max(E.rollout_lds_bytes(c[2], c[3], c[4], c[0]) for c in K.ROLLOUT_CASES) == 116228       # (what ran before)
    for bad in ((65, 16, 64, 64, 1), (0, 16, 64, 64, 1), (64, 17, 64, 64, 1), (64, 0, 64, 64, 1), (64, 16, 16, 64, 1), (64, 16, 48, 64, 1),
                (64, 16, 128, 64, 1), (64, 16, 64, 65, 1), (64, 16, 64, 0, 1), (64, 16, 64, 64, 0), (64, 16, 64, 64, 3)):
        assert not E.supported(*bad), bad


def test_supported_restatement_agrees_with_the_library():
    """The python restatement of dra_a2c_mlp_supported against the library's own answer, over the range's edges."""
    from deeprl_amd import a2c_mlp
    for S in (0, 1, 17, 64, 65):
        for A in (0, 1, 16, 17):
            for H in (16, 32, 48, 64, 128):
                for N in (0, 1, 63, 64, 65):
                    for gate in (0, 1, 2, 3):
                        assert a2c_mlp.supported(S, A, H, N, gate) == E.supported(S, A, H, N, gate), (S, A, H, N, gate)


def test_rollout_table_reaches_every_instantiation_and_geometry():
    shapes = [E.rollout_shape(c) for c in E.ROLLOUT_CASES]
    inst = {s['instantiation'] for s in shapes}
    assert {g for _, g in inst} == {"relu", "tanh"} and {h for h, _ in inst} == {32, 64}
    # the two instantiations that tests/a2c_mlp_cases.py never launches; with its <64, relu> and <32, tanh>: all four
    assert {(32, "relu"), (64, "tanh")} <= inst and {(c[4], c[5]) for c in K.ROLLOUT_CASES} == {(64, "relu"), (32, "tanh")}
    assert {(c[4], c[5]) for c in K.ROLLOUT_CASES} | inst == {(h, g) for h in (32, 64) for g in ("relu", "tanh")}
    assert any(s['N'] > 8 and s['N'] % 8 for s in shapes if s['H'] == 32) and any(s['N'] > 8 and s['N'] % 8 for s in shapes if s['H'] == 64)
    assert any(s['blocks'] > s['groups'] and s['live_last'] == 1 and s['H'] == 32 for s in shapes)      # a second pass over one live row
    assert any(s['blocks'] == 2 and s['live_last'] == 1 and s['H'] == 64 for s in shapes)
    assert any(s['blocks'] == 3 and s['live_last'] == 1 for s in shapes)
    assert {1, 64} <= {s['S'] for s in shapes} and {1, 16} <= {s['A'] for s in shapes} and {1, 63, 64} <= {s['N'] for s in shapes}
    assert any(s['A'] == 1 and s['N'] > 1 for s in shapes) and any(s['T'] == 1 for s in shapes) and any(s['horizon'] == 1 for s in shapes)
    # both paths of the fold's division, all 64 feature lanes, a batch of one row
    upd = [s for s in shapes if s['folds']]
    assert any(s['pow2'] and s['N'] > 1 for s in upd) and any(not s['pow2'] for s in upd) and any(s['N'] == 1 and s['folds'] == 41 for s in upd)
    assert any(s['S'] == 64 and s['pow2'] for s in upd) and any(s['S'] == 64 and not s['pow2'] for s in upd)
    assert any(s['noise'] == 640 and s['N'] == 1 for s in shapes) and any(s['noise'] < 256 for s in shapes)
    assert {s['kind'] for s in shapes} == {"meanstd-update", "meanstd-readonly", "identity"}


# ------------------------------------------------------------------------------------------------ what the references hold
@pytest.mark.parametrize("case", E.ROLLOUT_CASES, ids=_IDS)
def test_rollout_case_reaches_its_path_and_its_inputs_carry_the_bars(case):
    """A condition, not a measurement: a case whose float32 CPU run of the reference exceeds 0.3 x a bar is replaced."""
    n, t_len, S, A, H, gate, kind, horizon, clip = case
    want, envs, norm, start = E.rollout_reference(case)
    narrow, envs32, norm32, start32 = E.run_rollout(case, torch.float32)
    cid = E.case_id(case)
    # the start: counters i % 3, seeds apart, and the counters the rollout ends on
    assert start["counters"] == [i % 3 for i in range(n)] and len(set(start["seeds"])) == n
    assert [e.c for e in envs] == [i % 3 + t_len for i in range(n)] == [e.c for e in envs32]
    assert np.array_equal(start["raw"], start32["raw"]) and np.array_equal(start["rms"], start32["rms"])
    assert want["state"].shape == (t_len, n, S) and want["action"].shape == (t_len, n, A) and want["v"].shape == (t_len + 1, n)
    # float32 forwards against float64 forwards
    for key, r in E.compare_rollout(narrow, want).items():
        assert r <= E.HOST_FRACTION * E.bar(cid, "rollout"), (key, r)
    assert E.fraction("raw", narrow["raw_states"], want["raw_states"]) <= E.HOST_FRACTION * E.bar(cid, "raw")
    f_mean, f_var, same_count = E.compare_stats(E.final_stats(norm32, start), E.final_stats(norm, start), S)
    assert f_mean <= E.HOST_FRACTION * E.bar(cid, "stats") and f_var <= E.HOST_FRACTION * E.bar(cid, "stats") and same_count
    # rewards and terminals do not depend on the actions: the same bits in both runs; the rewards carry reward_coef
    assert want["reward"].dtype == np.float32 and want["mask"].dtype == np.float32
    assert np.array_equal(want["reward"].view(np.uint32), narrow["reward"].view(np.uint32)) and np.array_equal(want["mask"], narrow["mask"])
    assert np.abs(want["reward"]).max() <= 0.1 * 2.0 * 1.7320508075688772 and np.abs(want["reward"]).max() > 0.0
    # terminals
    if horizon == 1:
        assert not want["mask"].any()
    elif t_len * n >= 40:
        assert (want["mask"] == 0).any() and (want["mask"] == 1).any()
    # the environment's clamp of the actions to [-1, 1] is at work
    assert (want["action"] > 1.0).any() and (want["action"] < -1.0).any()
    # the clip: reached on both sides where the case narrows it, never at the real configuration's 10
    up, down = E.clip_census(case)
    x = np.concatenate([want["state"].reshape(-1), want["cur_state"].reshape(-1)])
    if kind != "identity" and clip < 10.0:
        assert up >= 10 and down >= 10 and float(np.abs(x).max()) == clip, (up, down)
        assert 0.2 * x.size <= (np.abs(x) < clip).sum()          # (and enough elements stay inside it)
    else:
        assert up == 0 and down == 0 and float(np.abs(x).max()) < 10.0
    # the statistics
    if kind == "meanstd-update":
        count = start["rms"][2 * S]
        for _ in range(t_len + 1):
            count = count + n
        assert norm.rms.count == count
        assert not np.array_equal(E.final_stats(norm, start)[:2 * S], start["rms"][:2 * S])
    elif kind == "meanstd-readonly":
        assert np.array_equal(E.final_stats(norm, start), start["rms"]) and start["rms"][2 * S] == E.WARM_ROWS + 1e-4
    else:
        assert norm is None and np.array_equal(want["state"][0], start["raw"].astype(np.float32))


def test_counters_that_differ_change_the_rollout():
    """The pre-stepped start is not the fresh start: rewards and masks (hashes of seed and counter) differ, so a kernel that read
    the wrong environment's counter, or none, would miss them."""
    case = E.ROLLOUT_CASES[1]
    n, t_len, S, A, H, gate, kind, horizon, clip = case
    want = E.rollout_reference(case)[0]
    envs, raw = R.start_envs([E.ENV_SEED0 + i for i in range(n)], S, A, horizon)
    assert [e.c for e in envs] == [0] * n
    norm, _ = R.warm_normalizer(kind, S, E.WARM_ROWS, clip=clip)
    fresh = R.rollout(R.init_params(S, A, H, seed=12 + n), envs, raw, norm, t_len, E.NOISE_SEED, E.SAMPLER0, gate=gate,
                      n_global=n + E.ENV0_EXTRA + 1, env0=E.ENV0_EXTRA, reward_coef=E.REWARD_COEF)
    pre = np.arange(n) % 3
    assert np.array_equal(fresh["reward"][:, pre == 0], want["reward"][:, pre == 0])
    assert not np.array_equal(fresh["reward"][:, pre != 0], want["reward"][:, pre != 0])
    # environment i pre-stepped k times sees at step t what the fresh one sees at step t + k
    assert np.array_equal(fresh["reward"][1:, pre == 1], want["reward"][:-1, pre == 1])
    assert np.array_equal(fresh["mask"][2:, pre == 2], want["mask"][:-2, pre == 2])


def test_restatement_defaults_are_what_they_were():
    """start_envs / warm_normalizer build what tests/a2c_mlp_cases.py builds by hand, and rollout's dtype keyword at its default
    gives the bits of the call without it: the workload-shape suite's references did not move."""
    case = K.ROLLOUT_CASES[1]
    n, t_len, S, A, H, gate, kind, horizon = case
    params, envs, raw, norm, rms0 = K._setup(case)
    envs2, raw2 = R.start_envs([K.ENV_SEED0 + i for i in range(n)], S, A, horizon)
    norm2, rms2 = R.warm_normalizer(kind, S, K.WARM_ROWS)
    assert np.array_equal(raw, raw2) and np.array_equal(rms0, rms2) and norm2.clip == norm.clip == 10.0 and norm2.read_only == norm.read_only
    want = K.restated_rollout(case)[0]
    got = R.rollout(params, envs2, raw2, norm2, t_len, K.NOISE_SEED, K.SAMPLER0, gate=gate, n_global=n + K.ENV0_EXTRA + 1, env0=K.ENV0_EXTRA,
                    dtype=torch.float64)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert np.asarray(got[k]).dtype == np.asarray(v).dtype and np.array_equal(got[k], v), k
    none, rms_id = R.warm_normalizer("identity", S, K.WARM_ROWS)
    assert none is None and np.array_equal(rms_id, np.concatenate([np.zeros(S), np.ones(S), [0.0]]))


# ------------------------------------------------------------------------------------------------ head cases
@pytest.mark.parametrize("n,a", E.HEAD_CASES)
def test_head_case_reaches_the_saturated_tanh_and_the_softplus_threshold(n, a):
    z, std, action, g_lp, g_ent = E.head_case(n, a)
    ref = E.head_reference(n, a)
    assert z.shape == action.shape == (n, a) and std.shape == (a,) and g_lp.shape == g_ent.shape == (n, 1)
    assert n > 256 and 1 <= a <= E.K_HEAD_MAX_A                  # a second workgroup forward, a second trip round `row += 256`
    assert np.abs(ref["mean"]).max() > 0.999
    assert ref["mean"].shape == ref["dz"].shape == (n, a) and ref["log_pi_a"].shape == ref["entropy"].shape == (n, 1) and ref["dstd"].shape == (a,)
    assert all(np.isfinite(v).all() for v in ref.values()) and np.abs(ref["dstd"]).min() > 0.0
    if a >= 3:
        assert (std > 20.0).any() and (std < 20.0).any()
    else:
        assert std.tolist() == [-8.0]                            # one dimension: the smallest scale, where log_pi_a is hardest


def test_head_table_covers_both_sides_of_the_threshold_and_the_widest_head():
    stds = np.concatenate([E.head_case(n, a)[1] for n, a in E.HEAD_CASES])
    assert set(np.unique(stds).tolist()) == {float(np.float32(s)) for s in E.STD_VALUES}
    assert (stds > 20.0).any() and (stds < 20.0).any() and np.float32(19.9) in stds and np.float32(20.1) in stds
    assert max(a for _, a in E.HEAD_CASES) == E.K_HEAD_MAX_A == 64 and min(a for _, a in E.HEAD_CASES) == 1
    assert (320, 6) in E.HEAD_CASES                              # 64 workers x 5 steps of the a2c_continuous head
