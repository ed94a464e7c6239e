"""CPU proof for tests/stream_stat_cases.py: the statistics compute what they say, every case of the restatements meets the tighter
CPU margins (|z| <= 4, D sqrt(n) <= 2.4), every negative control fails the bar it is aimed at, the stride / cap sets are
collision-free inside the documented caps and collide one step past them, the restatements use 64-bit arithmetic at the far
counters, and the product's host statements (envs.SyntheticContinuous, envs.synthetic_reward_done_vec, envs.synthetic_frame,
envs.cenv_reset_state, dist.gumbel_argmax, oracle.ppo_mlp_oracle.gauss_noise) draw the values the statistics ran on -- so the CPU
result speaks for the product formula.  tests/test_gpu_stream_stats.py draws the same cases through the kernels."""
import math

import numpy as np
import pytest

import stream_stat_cases as S

HOST = (S.Z_HOST, S.KS_HOST)


def _ids(cases):
    return [c["name"] for c in cases]


def _hold(tag, stats, bars=HOST):
    print("%s: %s" % (tag, "  ".join("%s %.2f" % (n, v) for n, _, v in stats)))
    bad = S.failures(stats, bars)
    assert not bad, "%s: %s beyond the bars %s" % (tag, bad, bars)


def _fails(tag, stats, target):
    """The control fails the FULL bar of the statistic it is aimed at."""
    got = {n: (kind, v) for n, kind, v in stats}
    kind, v = got[target]
    print("control %s: %s = %.2f" % (tag, target, v))
    assert not abs(v) <= (S.KS_BAR if kind == "ks" else S.Z_BAR), "%s: the control passes %s (%.2f)" % (tag, target, v)


# ------------------------------------------------------------------------------------------------------------ the statistics
def test_statistics_have_their_closed_forms():
    # Wilson-Hilferty at X2 = df is 2 / (9 df) above its mean, in units of its standard deviation
    e = np.full(5, 100.0)
    assert S.chi2_z(e, e) == pytest.approx(-(1.0 - 2.0 / 36.0) / math.sqrt(2.0 / 36.0))
    c = np.asarray([110.0, 90.0, 100.0, 105.0, 95.0])      # X2 = (100 + 100 + 0 + 25 + 25) / 100 = 2.5, df 4
    assert S.chi2_z(c, e) == pytest.approx(((2.5 / 4) ** (1 / 3.0) - (1 - 2 / 36.0)) / math.sqrt(2 / 36.0))
    # cells under 20 expected counts are merged, smallest first; totals are kept
    mc, me = S.merge_cells([1, 2, 3, 50, 60], [5.0, 6.0, 12.0, 40.0, 57.0])
    assert list(me) == [23.0, 40.0, 57.0] and list(mc) == [6.0, 50.0, 60.0]
    mc, me = S.merge_cells([50, 60, 1], [40.0, 57.0, 3.0])
    assert list(me) == [43.0, 57.0] and list(mc) == [51.0, 60.0]
    # KS: one point at the median is D = 1/2; an exact grid of n points is D = 1 / (2 n)
    assert S.ks_stat([0.5], S.uniform_cdf(0.0, 1.0)) == pytest.approx(0.5)
    grid = (np.arange(100) + 0.5) / 100
    assert S.ks_stat(grid, S.uniform_cdf(0.0, 1.0)) == pytest.approx(0.005 * 10)
    assert S.normal_cdf([0.0])[0] == 0.5 and S.normal_cdf([1.959963984540054])[0] == pytest.approx(0.975, abs=1e-12)
    assert S.gumbel_cdf([0.0])[0] == pytest.approx(math.exp(-1.0))
    # moments: the reward (four uniforms, scaled by sqrt 3) has variance 1 and fourth moment 3 - 1.2 / 4
    assert S._REWARD[2] == pytest.approx(1.0) and S._REWARD[4] == pytest.approx(2.7) and S._REWARD[1] == S._REWARD[3] == 0.0
    assert S.sum_moments([1.0, 0.0, 1.0, 0.0, 3.0], 2)[4] == pytest.approx(12.0)      # N(0, 2): 3 sigma^4
    assert S._UNI_NOISE[2] == pytest.approx(0.04 ** 2 / 12) and S._UNI_RESET[4] == pytest.approx(0.05 ** 4 / 5)
    # z statistics on samples with the answer built in
    x = np.asarray([1.0, -1.0] * 50)
    assert S.z_mean(x, 0.0, 1.0) == 0.0 and S.z_mean(x + 0.3, 0.0, 1.0) == pytest.approx(3.0)
    assert S.z_corr(x, x, 0.0, 1.0, 0.0, 1.0) == pytest.approx(10.0) and S.z_corr(x, -x, 0.0, 1.0, 0.0, 1.0) == pytest.approx(-10.0)
    assert S.z_lag(x.reshape(10, 10), 1, 0.0, 1.0) == pytest.approx(-math.sqrt(90.0))
    assert S.z_lag(x.reshape(10, 10), 0, 0.0, 1.0) == pytest.approx(math.sqrt(90.0))
    assert S.z_moment(x, 0.0, 2, 1.0, 3.0) == 0.0 and S.z_rate(60, 100, 0.5) == pytest.approx(2.0)
    assert S.worst([("a", "z", -4.0), ("b", "ks", 2.1)]) == ("a", 0.8) and S.failures([("a", "z", float("nan"))])


def test_bars_are_the_derived_ones():
    assert S.Z_BAR == 5.0 and S.KS_BAR == 2.8 and S.Z_HOST == 4.0 and S.KS_HOST == 2.4 and S.MIN_EXPECTED == 20.0
    assert math.erfc(5.0 / math.sqrt(2.0)) < 6e-7 and 2 * math.exp(-2 * 2.8 ** 2) < 3.2e-7
    import loss_edge_cases as L
    assert (S.SCORE_GAP, S.EXEMPT_CAP) == (L.SCORE_GAP, L.EXEMPT_CAP)


# -------------------------------------------------------------------------------------------------------------------- gumbel
@pytest.mark.parametrize("c", S.gumbel_cases(), ids=_ids(S.gumbel_cases()))
def test_gumbel_restatement_meets_the_margins(c):
    a, gap, noise = S.gumbel_sample(c, noise=True)
    a2, _, noise2 = S.gumbel_sample(c, seed=c["seed2"], noise=True)
    _hold("gumbel[%s]" % c["name"], S.gumbel_action_stats(c, a, a2) + S.gumbel_noise_stats(noise, noise2))
    # the kernel's float32 scores may decide a row under SCORE_GAP differently: the restatement alone stays inside the 1 % cap
    under = (gap < S.SCORE_GAP).sum(axis=1)
    print("gumbel[%s]: at most %d of %d rows of a launch under the margin" % (c["name"], under.max(), c["rows"]))
    assert under.max() <= int(S.EXEMPT_CAP * c["rows"])


def test_gumbel_controls_fail():
    c = [x for x in S.gumbel_cases() if x["name"] == "a6_peaked"][0]
    a2, _ = S.gumbel_sample(c, seed=c["seed2"])
    a, _ = S.gumbel_sample(c, row_stride=1)
    _fails("gumbel row stride 1", S.gumbel_action_stats(c, a, a2), "lag_row")
    # the 24-bit uniform: invisible to any sample, visible at the one word that reaches u == 1
    e = S.GUMBEL_EXTREME
    h = S.mix64(S.gumbel_words(e["seed"], e["step"], [e["row"]], e["A"]))[0, e["action"]]
    assert int(h) >> 40 == (1 << 24) - 1, "GUMBEL_EXTREME is no longer a word with its top 24 bits set"
    assert S.gumbel_uniform_of_hash(h, 23) == 1.0 - 2.0 ** -24 and S.gumbel_uniform_of_hash(h, 24) == 1.0
    assert S.gumbel_uniform_of_hash(np.uint64(0), 23) == 2.0 ** -24 and S.gumbel_uniform_of_hash(np.uint64(S.M64), 23) < 1.0
    logits = S.gumbel_extreme_logits(e["rows"], e["A"], e["action"])
    good, gap, noise = S.gumbel_draw(logits, e["seed"], e["step"], e["lo"])
    bad, _, bad_noise = S.gumbel_draw(logits, e["seed"], e["step"], e["lo"], bits=24)
    r = e["row"] - e["lo"]
    assert np.isfinite(noise).all() and noise[r, e["action"]] == pytest.approx(-math.log(-math.log(1.0 - 2.0 ** -24)))
    assert not (good == e["action"]).any() and gap.min() >= S.SCORE_GAP
    assert np.isinf(bad_noise[r, e["action"]]) and bad[r] == e["action"], "the control (u == 1) does not win its row"
    _fails("gumbel 24-bit uniform", S.gumbel_noise_stats(bad_noise[None], noise[None]), "noise_finite")


# --------------------------------------------------------------------------------------------------------------------- gauss
@pytest.mark.parametrize("c", S.gauss_cases(), ids=_ids(S.gauss_cases()))
def test_gauss_restatement_meets_the_margins(c):
    _hold("gauss[%s]" % c["name"], S.gauss_stats(S.gauss_sample(c), S.gauss_sample(c, seed=c["seed2"])))


def test_gauss_controls_fail():
    c = [x for x in S.gauss_cases() if x["name"] == "a16"][0]
    z2 = S.gauss_sample(c, seed=c["seed2"])
    for name, variant, target in S.GAUSS_CONTROLS:
        _fails("gauss " + name, S.gauss_stats(S.gauss_sample(c, **variant), z2), target)
    # the range of Box-Muller's inputs: u1 in (0, 1] keeps the logarithm finite, the largest |z| is sqrt(48 log 2) = 5.77
    f = np.float32
    assert np.sqrt(f(-2.0) * np.log(f(1.0) * f(5.9604644775390625e-8))) == pytest.approx(math.sqrt(48 * math.log(2.0)), rel=1e-6)
    assert f((1 << 24) - 1 + 1) * f(5.9604644775390625e-8) == f(1.0) and f((1 << 24) - 1) * f(5.9604644775390625e-8) < f(1.0)


# ---------------------------------------------------------------------------------------------------- continuous environment
@pytest.mark.parametrize("c", S.cenv_cases(), ids=_ids(S.cenv_cases()))
def test_cenv_restatement_meets_the_margins(c):
    r = S.cenv_rollout(c["seeds"], c["S"], S.cenv_actions(c), c["horizon"])
    assert 0 < r["done"].sum() < r["done"].size
    _hold("cenv[%s]" % c["name"], S.cenv_stats(c, r["states"], r["reward"], r["done"], r["mean_a"]))


def test_cenv_streams_are_mutually_uncorrelated():
    _hold("cenv streams", S.cenv_stream_stats(S.cenv_cases()[0]["seeds"], list(range(1, 2049))))
    bad = S.cenv_stream_stats(S.cenv_cases()[0]["seeds"], list(range(1, 2049)), with_stream=False)
    for name, _, _ in bad:
        _fails("cenv without the stream term", bad, name)


def test_cenv_controls_fail():
    c = S.cenv_cases()[1]
    act = S.cenv_actions(c)
    for name, variant, target in S.CENV_CONTROLS:
        r = S.cenv_rollout(c["seeds"], c["S"], act, c["horizon"], **variant)
        stats = S.cenv_stats(c, r["states"], r["reward"], r["done"], r["mean_a"])
        _fails("cenv " + name, stats, target)
        if name == "no_stream_term":
            _fails("cenv " + name, stats, "reset_vs_reward")


def test_cartpole_resets_meet_the_margins():
    c = S.CARTPOLE_CASE
    _hold("cartpole resets", S.reset_stats(S.cartpole_resets(c["seeds"], 0, c["steps"])))


# ----------------------------------------------------------------------------------------------------------- synthetic Atari
@pytest.mark.parametrize("c", S.ATARI_CASES, ids=_ids(S.ATARI_CASES))
def test_atari_restatement_meets_the_margins(c):
    r, d = S.atari_reward_done(c["seeds"], [c["counter0"] + k for k in range(c["count"])], c["done_period"])
    _hold("atari[%s]" % c["name"], S.atari_stats(c, r, d))


def test_atari_frames_meet_the_margins_and_the_cross_statistic_has_power():
    c = S.ATARI_FRAME_CASE
    _hold("atari frames", S.frame_stats(S.atari_frames(c["seed"], [c["counter0"] + k for k in range(c["count"])], c["frame_bytes"])))
    # control for the overlap's cross statistic: a terminal read from the SAME part of the shared word as the reward
    c = S.ATARI_CASES[1]
    counters = [c["counter0"] + k for k in range(c["count"])]
    r, d = S.atari_reward_done(c["seeds"], counters, 10)
    u = (S.mix64(S.atari_mask_words(c["seeds"], counters)) >> np.uint64(32)) % np.uint64(10)
    _fails("atari terminal from the reward's bits", S.atari_stats(dict(c, done_period=10), r, u == 0), "done_vs_next_seed_reward")


# ------------------------------------------------------------------------------------------------------------ stride and cap
def test_positions_inside_the_caps_are_distinct_and_one_past_them_collides():
    assert (S.GUMBEL_STRIDE, S.GUMBEL_CAP, S.GAUSS_STRIDE, S.GAUSS_CAP, S.CENV_STRIDE, S.CENV_CAP) == (64, 64, 64, 32, 64, 64)
    assert S.collisions(S.gumbel_position_words(7, 3, 300, S.GUMBEL_CAP)) == 0
    assert S.collisions(S.gumbel_position_words(7, 3, 300, S.GUMBEL_CAP + 1)) == 299          # (r, 64) is (r + 1, 0)
    assert S.collisions(S.gauss_position_words(7, 3, 300, S.GAUSS_CAP)) == 0
    assert S.collisions(S.gauss_position_words(7, 3, 300, S.GAUSS_CAP + 1)) == 2 * 299
    assert S.collisions(S.cenv_position_words(7, 300, S.CENV_CAP)) == 0
    assert S.collisions(S.cenv_position_words(7, 300, S.CENV_CAP + 1)) == S.CENV_STREAMS * 299
    assert S.collisions(S.atari_position_words(7, 300, S.ATARI_WORDS)) == 0
    assert S.collisions(S.atari_position_words(7, 300, S.ATARI_WORDS + 1)) == 299
    # the caps the entry points refuse at are these strides (csrc: n_actions > 64, a_dim > 32, s_dim > 64 -> EINVAL); the GPU
    # file checks the refusals themselves
    import ppo_mlp_edge_cases as P
    assert P.GAUSS_REFUSED_A == S.GAUSS_CAP + 1 and P.ENV_REFUSED_S == S.CENV_CAP + 1


def test_atari_overlap_between_consecutive_seeds_is_what_the_table_says():
    c = [5, 900, 12345]
    mask_i = S.atari_mask_words([20], c)[0]
    assert np.array_equal(mask_i, S.atari_reward_words([21], c)[0])
    frames = S.atari_frame_words(22, [x // S.ATARI_WORDS for x in c])
    assert all(frames[k, x % S.ATARI_WORDS] == mask_i[k] for k, x in enumerate(c))


# -------------------------------------------------------------------------------------------------------------- far counters
def test_restatements_use_64_bit_positions_at_the_far_counters():
    """A restatement that truncated a counter, row or seed to 32 bits would draw the same values at c and c + 2^32."""
    w = 1 << 32
    logits = S.far_logits(*S.FAR_GUMBEL_SHAPE, key=1)
    for step, lo, seed in S.FAR_GUMBEL:
        a, gap, noise = S.gumbel_draw(logits, seed, step, lo)
        assert gap.min() >= S.SCORE_GAP, "far gumbel (%d, %d, %d): a row under the margin, 65 rows allow none" % (step, lo, seed)
        for other in ((seed, step + w, lo), (seed, step, lo + w), (seed + w, step, lo)):
            assert not np.array_equal(noise, S.gumbel_draw(logits, other[0], other[1], other[2])[2])
    n, a_dim = S.FAR_GAUSS_SHAPE
    for t, ng, e0, seed in S.FAR_GAUSS:
        z = S.gauss_draw(seed, t, ng, [e0 + i for i in range(n)], a_dim)
        assert np.isfinite(z).all()
        for t2, ng2, e2, s2 in ((t + w, ng, e0, seed), (t, ng + w, e0, seed), (t, ng, e0 + w, seed), (t, ng, e0, seed + w)):
            assert not np.array_equal(z, S.gauss_draw(s2, t2, ng2, [e2 + i for i in range(n)], a_dim))
    for c0 in S.FAR_COUNTERS:
        seeds = list(S.FAR_SEEDS) + [3]
        act = np.zeros((3, len(seeds), 2), dtype=np.float32)
        r = S.cenv_rollout(seeds, 5, act, 7, c0=c0)
        r2 = S.cenv_rollout(seeds, 5, act, 7, c0=c0 + w)
        assert r["counters"] == [c0 + 3] * len(seeds)
        assert not np.array_equal(r["reward"], r2["reward"]) and not np.array_equal(r["states"], r2["states"])
        assert not np.array_equal(S.cartpole_resets(seeds, c0, 3), S.cartpole_resets(seeds, c0 + w, 3))
        ctr = [c0 + k for k in range(4)]
        assert not np.array_equal(S.atari_frames(5, ctr, 64), S.atari_frames(5, [x + w for x in ctr], 64))
        assert not np.array_equal(S.mix64(S.atari_reward_words([5], ctr)), S.mix64(S.atari_reward_words([5], [x + w for x in ctr])))
    assert S.as_i64(-3) == -3 and S.as_i64((1 << 63) + 7) == -(1 << 63) + 7 and int(S.u64(-3)) == (1 << 64) - 3


# ------------------------------------------------------------------------------------- the product's host statements draw the same
def test_envs_synthetic_continuous_draws_the_restatement():
    from deeprl_amd.envs import SyntheticContinuous
    for seed, s_dim, a_dim, horizon in ((40, 17, 3, 7), (S.FAR_SEEDS[1], 64, 2, 1), ((1 << 35) + 1, 1, 1, 1000)):
        act = (np.random.RandomState(s_dim).standard_normal((40, 1, a_dim)) * 0.8).astype(np.float32)
        want = S.cenv_rollout([seed], s_dim, act, horizon)
        env = SyntheticContinuous(seed, s_dim, a_dim, horizon)
        s = env.reset()
        assert np.array_equal(s, want["states"][0, 0])
        for t in range(40):
            s, r, d, _ = env.step(act[t, 0])
            if d:
                s = env.reset()
            assert np.array_equal(s, want["states"][t + 1, 0]) and r == want["reward"][t, 0] and d == want["done"][t, 0], (seed, t)


def test_envs_reset_state_and_cartpole_reset_draw_the_restatement():
    from deeprl_amd.envs import CartPole, cenv_reset_state, cenv_u3
    for seed in (50, 113) + S.FAR_SEEDS:
        for c in (0, 1, 1023) + S.FAR_POINTS:
            want = S.cenv_reset([seed], [c], 64)[0]
            assert all(cenv_reset_state(seed & S.M64, c, j) == want[j] for j in (0, 1, 3, 17, 63))
            assert -0.05 + 0.1 * cenv_u3(seed & S.M64, c, 5) == want[5]
    env = CartPole(57, 1)
    env.reset()
    for k in range(5):          # horizon 1: every step ends in the reset at the advanced counter
        s, _, d, _ = env.step(1)
        assert d and np.array_equal(env.reset(), S.cartpole_resets([57], 0, 5)[k, 0])


def test_envs_synthetic_atari_draws_the_restatement():
    from deeprl_amd import envs
    c = S.ATARI_CASES[1]
    counters = np.asarray([c["counter0"] + k for k in range(512)] + [x - 1 for x in S.FAR_POINTS], dtype=np.int64)
    for seed in c["seeds"][:2] + [S.FAR_SEEDS[0]]:
        want_r, want_d = S.atari_reward_done([seed], counters, c["done_period"])
        r, d = envs.synthetic_reward_done_vec(counters, np.full(counters.size, seed, dtype=np.int64), np.full(counters.size, c["done_period"]))
        assert np.array_equal(r, want_r[0]) and np.array_equal(d, want_d[0])
        assert envs.synthetic_reward_done(int(counters[3]), seed, c["done_period"]) == (want_r[0, 3], want_d[0, 3])
        assert np.array_equal(envs.synthetic_frame(int(counters[7]), seed), S.atari_frames(seed, [int(counters[7])])[0])


def test_dist_gumbel_argmax_and_the_other_restatements_draw_the_restatement():
    import torch
    from deeprl_amd.dist import gumbel_argmax
    import loss_edge_cases as L
    c = [x for x in S.gumbel_cases() if x["name"] == "a18_peaked"][0]
    for k in (0, 1):
        want, gap, noise = S.gumbel_draw(c["logits"], c["seed"], c["step0"] + k, c["lo"])
        a, g, u = L.gumbel_ref(c["logits"], c["seed"], c["step0"] + k, c["lo"])
        assert np.array_equal(a, want) and np.array_equal(-np.log(-np.log(u)), noise)
        got = gumbel_argmax(torch.from_numpy(c["logits"]).double(), torch.from_numpy(u)).numpy()
        # (its clamp of u at 1 - 1e-7 moves only the largest of the 2^23 uniforms, 1 - 2^-24, by 4e-8)
        assert np.array_equal(got[gap >= S.SCORE_GAP], want[gap >= S.SCORE_GAP])


def test_oracle_gauss_noise_draws_the_restatement():
    from oracle.ppo_mlp_oracle import gauss_noise
    for c in S.gauss_cases():
        envs = [c["env0"] + i for i in range(c["rows"])]
        for t in (c["step0"], c["step0"] + 255):
            assert np.array_equal(gauss_noise(c["seed"], t, c["n_global"], envs, c["A"]), S.gauss_draw(c["seed"], t, c["n_global"], envs, c["A"]))
