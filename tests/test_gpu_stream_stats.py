"""The device-drawn random streams as SAMPLES: the cases of tests/stream_stat_cases.py drawn through the kernels (dra_gumbel_sample,
dra_gauss_sample, dra_cont_env_step, dra_cartpole_step, dra_ring_fill_synthetic).  Every test asserts two things:
  1. the WHOLE sample equals the restatement's (integer and fp64 streams bit for bit; the fp32 Gaussian within dra_gauss_sample's
     1e-5 absolute bar; a Gumbel decision may differ only in rows whose float64 score gap is under SCORE_GAP, at most 1 % of a launch);
  2. the statistics of the device's own draws meet the full bars (|z| <= 5, D sqrt(n) <= 2.8), each recorded in the parity log as a
     fraction of its bar.
tests/test_stream_stats_host.py proves on the CPU that the restatements meet the tighter margins, that the negative controls fail
and that the restatements are the product's host formulas.  The far-counter tests compare kernel and restatement exactly at sampler
steps, rows, counters and seeds around 2^31, 2^32 and at 2^40, where a 32-bit truncation in a kernel would first show."""
import numpy as np
import pytest
import torch

import stream_stat_cases as S
from parity_log import record_parity

pytestmark = pytest.mark.gpu
EINVAL = -22


def _ids(cases):
    return [c["name"] for c in cases]


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """A test that left the device in error ends the session: nothing more is launched on a faulted GPU."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test, nothing more is launched: %s" % e, returncode=3)


def _hold(tag, stats):
    """The device's own draws against the full bars; every statistic to the parity log as a fraction of its bar."""
    print("%s: %s" % (tag, "  ".join("%s %.2f" % (n, v) for n, _, v in stats)))
    record_parity("stream_stats " + tag, **{n: abs(v) / (S.KS_BAR if kind == "ks" else S.Z_BAR) for n, kind, v in stats})
    bad = S.failures(stats)
    assert not bad, "%s: %s beyond |z| <= %g / KS <= %g" % (tag, bad, S.Z_BAR, S.KS_BAR)


def _dev(x, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = np.nonzero(got.view(view).reshape(-1) != want.view(view).reshape(-1))[0]
    assert diff.size == 0, "%s: %d of %d elements differ, first at %d (got %r, want %r)" % (
        what, diff.size, got.size, diff[0], got.reshape(-1)[diff[0]], want.reshape(-1)[diff[0]])


# -------------------------------------------------------------------------------------------------------------------- gumbel
def _gumbel_launches(dra, logits, seed, step0, lo, steps):
    """`steps` launches of dra_gumbel_sample, the device step counter advancing by itself -> actions [steps, n]."""
    from deeprl_amd import ops
    dev = dra.Config.DEVICE
    step_dev = torch.full((1,), step0, dtype=torch.int64, device=dev)
    lg = _dev(logits, dev)
    got = torch.stack([ops.gumbel_sample(lg, seed, step_dev, lo) for _ in range(steps)])
    assert int(step_dev.cpu()[0]) == step0 + steps
    return got.cpu().numpy()


def _gumbel_equal(tag, got, want, gap, exact=False):
    """Per launch: the float64 decision in every row whose gap is at least SCORE_GAP, at most 1 % of the rows under it."""
    cap = 0 if exact else int(S.EXEMPT_CAP * got.shape[1])
    under = gap < S.SCORE_GAP
    assert under.sum(axis=1).max() <= cap, "%s: %d rows of a launch under the margin, cap %d" % (tag, under.sum(axis=1).max(), cap)
    bad = np.argwhere((got != want) & ~under)
    assert bad.size == 0, "%s: %d draws differ from the float64 decision, first (launch, row) %s: got %d want %d gap %.3g" % (
        tag, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])], gap[tuple(bad[0])])
    return int(((got != want) & under).sum())


@pytest.mark.parametrize("c", S.gumbel_cases(), ids=_ids(S.gumbel_cases()))
def test_gumbel_sample_is_the_restatements_sample_and_follows_the_softmax(dra, c):
    got = _gumbel_launches(dra, c["logits"], c["seed"], c["step0"], c["lo"], c["steps"])
    got2 = _gumbel_launches(dra, c["logits"], c["seed2"], c["step0"], c["lo"], c["steps"])
    for g, seed in ((got, c["seed"]), (got2, c["seed2"])):
        want, gap = S.gumbel_sample(c, seed=seed)
        used = _gumbel_equal("gumbel[%s] seed %d" % (c["name"], seed), g, want, gap)
        record_parity("stream_stats gumbel[%s] seed %d" % (c["name"], seed), exemptions_used=used, draws=g.size)
    _hold("gumbel[%s]" % c["name"], S.gumbel_action_stats(c, got, got2))


def test_gumbel_uniform_stays_below_one_at_the_largest_word(dra):
    """The position whose hashed word has its top 24 bits set: with u == 1 (the 24-bit formula) its action would win against
    logits 30 above it; the kernel's 23-bit uniform gives it noise 16.6 and it loses."""
    e = S.GUMBEL_EXTREME
    logits = S.gumbel_extreme_logits(e["rows"], e["A"], e["action"])
    got = _gumbel_launches(dra, logits, e["seed"], e["step"], e["lo"], 1)
    want, gap, _ = S.gumbel_draw(logits, e["seed"], e["step"], e["lo"])
    bad, _, _ = S.gumbel_draw(logits, e["seed"], e["step"], e["lo"], bits=24)
    assert bad[e["row"] - e["lo"]] == e["action"] and gap.min() >= S.SCORE_GAP
    assert not (got[0] == e["action"]).any() and np.array_equal(got[0], want)


def test_gumbel_far_steps_rows_and_seeds(dra):
    n, a = S.FAR_GUMBEL_SHAPE
    logits = S.far_logits(n, a, key=1)
    for step, lo, seed in S.FAR_GUMBEL:
        got = _gumbel_launches(dra, logits, seed, step, lo, 3)
        want, gap = zip(*[S.gumbel_draw(logits, seed, step + k, lo)[:2] for k in range(3)])
        _gumbel_equal("far gumbel (step %d, lo %d, seed %d)" % (step, lo, seed), got, np.stack(want), np.stack(gap), exact=True)


def test_entry_points_refuse_one_past_each_stride(dra):
    """n_actions 65, a_dim 33 and s_dim 65 would make (row r, last component) reuse the word of (row r + 1, component 0)."""
    from deeprl_amd._lib import lib, ptr, stream_ptr
    dev = dra.Config.DEVICE
    step = torch.full((1,), 4, dtype=torch.int64, device=dev)
    a = S.GUMBEL_CAP + 1
    out = torch.full((2,), -7, dtype=torch.int64, device=dev)
    assert lib.dra_gumbel_sample.raw(ptr(torch.zeros(2, a, device=dev)), 2, a, 5, ptr(step), 0, ptr(out), stream_ptr()) == EINVAL
    a = S.GAUSS_CAP + 1
    act = torch.full((2, a), float("nan"), device=dev)
    assert lib.dra_gauss_sample.raw(ptr(torch.zeros(2, a, device=dev)), ptr(torch.ones(a, device=dev)), 2, a, 5, ptr(step), 2, 0, ptr(act),
                                    stream_ptr()) == EINVAL
    s = S.CENV_CAP + 1
    state, counter = torch.zeros(2, s, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    rew, done = torch.full((2,), float("nan"), dtype=torch.float64, device=dev), torch.full((2,), -3, dtype=torch.int32, device=dev)
    assert lib.dra_cont_env_step.raw(ptr(state), ptr(counter), ptr(torch.ones(2, dtype=torch.int64, device=dev)), ptr(torch.zeros(2, 2, device=dev)),
                                     2, s, 2, 5, ptr(rew), ptr(done), stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert int(step.cpu()[0]) == 4 and (out.cpu().numpy() == -7).all() and np.isnan(act.cpu().numpy()).all()
    assert np.isnan(rew.cpu().numpy()).all() and not counter.cpu().numpy().any()


# --------------------------------------------------------------------------------------------------------------------- gauss
def _gauss_launches(dra, n, a_dim, seed, step0, n_global, env0, steps):
    """`steps` launches of dra_gauss_sample with mean 0 and scale 1 -> the noise itself [steps, n, a_dim]."""
    from deeprl_amd import ppo_mlp
    dev = dra.Config.DEVICE
    step_dev = torch.full((1,), step0, dtype=torch.int64, device=dev)
    mean, scale = torch.zeros(n, a_dim, device=dev), torch.ones(a_dim, device=dev)
    got = torch.stack([ppo_mlp.gauss_sample(mean, scale, int(seed) & S.M64, step_dev, n_global=n_global, env0=env0) for _ in range(steps)])
    assert int(step_dev.cpu()[0]) == step0 + steps
    return got.cpu().numpy()


@pytest.mark.parametrize("c", S.gauss_cases(), ids=_ids(S.gauss_cases()))
def test_gauss_sample_is_the_restatements_sample_and_standard_normal(dra, c):
    got = _gauss_launches(dra, c["rows"], c["A"], c["seed"], c["step0"], c["n_global"], c["env0"], c["steps"])
    got2 = _gauss_launches(dra, c["rows"], c["A"], c["seed2"], c["step0"], c["n_global"], c["env0"], c["steps"])
    for g, seed in ((got, c["seed"]), (got2, c["seed2"])):
        want = S.gauss_sample(c, seed=seed)
        assert g.shape == want.shape and np.isfinite(g).all()
        err = float(np.abs(g.astype(np.float64) - want.astype(np.float64)).max())
        record_parity("stream_stats gauss[%s] seed %d" % (c["name"], seed), sample=err / S.GAUSS_ABS, draws=g.size)
        assert err <= S.GAUSS_ABS, "gauss[%s] seed %d: max abs error %.3g over the whole sample" % (c["name"], seed, err)
    _hold("gauss[%s]" % c["name"], S.gauss_stats(got, got2))


def test_gauss_far_steps_environments_and_seeds(dra):
    n, a_dim = S.FAR_GAUSS_SHAPE
    for t, n_global, env0, seed in S.FAR_GAUSS:
        got = _gauss_launches(dra, n, a_dim, seed, t, n_global, env0, 3)
        want = np.stack([S.gauss_draw(seed, t + k, n_global, [env0 + i for i in range(n)], a_dim) for k in range(3)])
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        assert err <= S.GAUSS_ABS, "far gauss (t %d, n_global %d, env0 %d, seed %d): max abs error %.3g" % (t, n_global, env0, seed, err)


# ---------------------------------------------------------------------------------------------------- continuous environment
def _cenv_run(dra, seeds, s_dim, actions, horizon, c0, state0):
    """T steps of dra_cont_env_step from (state0, counters c0) -> states [T + 1, n, S], reward [T, n], done [T, n], counters [n]."""
    from deeprl_amd import ppo_mlp
    dev = dra.Config.DEVICE
    t_len, n = actions.shape[:2]
    state = _dev(state0, dev)
    counter = torch.full((n,), c0, dtype=torch.int64, device=dev)
    seed = torch.tensor([S.as_i64(x) for x in seeds], dtype=torch.int64, device=dev)
    act = _dev(actions, dev)
    traj = torch.empty((t_len + 1, n, s_dim), dtype=torch.float64, device=dev)
    rew = torch.empty((t_len, n), dtype=torch.float64, device=dev)
    done = torch.empty((t_len, n), dtype=torch.int32, device=dev)
    traj[0].copy_(state)
    for t in range(t_len):
        r, d = ppo_mlp.cont_env_step(state, counter, seed, act[t], horizon)
        traj[t + 1].copy_(state), rew[t].copy_(r), done[t].copy_(d)
    return traj.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), counter.cpu().numpy()


@pytest.mark.parametrize("c", S.cenv_cases(), ids=_ids(S.cenv_cases()))
def test_cont_env_step_is_the_restatements_trajectory_and_follows_its_laws(dra, c):
    act = S.cenv_actions(c)
    want = S.cenv_rollout(c["seeds"], c["S"], act, c["horizon"])
    states, rew, done, counters = _cenv_run(dra, c["seeds"], c["S"], act, c["horizon"], 0, want["states"][0])
    _same_bits(states, want["states"], "cenv[%s] states" % c["name"])
    _same_bits(rew, want["reward"], "cenv[%s] reward" % c["name"])
    assert np.array_equal(done.astype(bool), want["done"]) and set(np.unique(done)) <= {0, 1}
    assert counters.tolist() == want["counters"]
    _hold("cenv[%s]" % c["name"], S.cenv_stats(c, states, rew, done, S.cenv_mean_action(act)))


def test_cont_env_far_counters_and_seeds(dra):
    seeds = list(S.FAR_SEEDS) + [3]
    act = (np.random.RandomState(5).standard_normal((3, len(seeds), 2)) * 0.8).astype(np.float32)
    for c0 in S.FAR_COUNTERS:
        want = S.cenv_rollout(seeds, 5, act, 7, c0=c0)
        states, rew, done, counters = _cenv_run(dra, seeds, 5, act, 7, c0, want["states"][0])
        _same_bits(states, want["states"], "far cenv %d states" % c0)
        _same_bits(rew, want["reward"], "far cenv %d reward" % c0)
        assert np.array_equal(done.astype(bool), want["done"]) and counters.tolist() == want["counters"]
    # horizon 1: every step takes the reset stream at the far counter
    want = S.cenv_rollout(seeds, 64, act, 1, c0=S.FAR_COUNTERS[1])
    states, _, done, _ = _cenv_run(dra, seeds, 64, act, 1, S.FAR_COUNTERS[1], want["states"][0])
    _same_bits(states, want["states"], "far cenv resets")
    assert done.all()


# ----------------------------------------------------------------------------------------------------------- cart-pole resets
def _cartpole_run(dra, seeds, c0, steps):
    """`steps` launches of dra_cartpole_step at horizon 1 (every step ends its episode) -> the states they leave [steps, n, 4]."""
    from deeprl_amd import ops
    dev = dra.Config.DEVICE
    n = len(seeds)
    state = _dev(S.cenv_reset(seeds, [c0] * n, 4), dev)
    counter = torch.full((n,), c0, dtype=torch.int64, device=dev)
    ep_steps, ep_return = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    seed = torch.tensor([S.as_i64(x) for x in seeds], dtype=torch.int64, device=dev)
    action = _dev(np.arange(n) % 2, dev, torch.int64)
    traj = torch.empty((steps, n, 4), dtype=torch.float64, device=dev)
    dones = torch.empty((steps, n), dtype=torch.int32, device=dev)
    for t in range(steps):
        _, d = ops.cartpole_step(state, counter, ep_steps, ep_return, seed, action, 1)
        traj[t].copy_(state), dones[t].copy_(d)
    assert dones.cpu().numpy().all() and counter.cpu().numpy().tolist() == [c0 + steps] * n
    return traj.cpu().numpy()


def test_cartpole_resets_are_the_restatements_and_uniform(dra):
    c = S.CARTPOLE_CASE
    got = _cartpole_run(dra, c["seeds"], 0, c["steps"])
    _same_bits(got, S.cartpole_resets(c["seeds"], 0, c["steps"]), "cart-pole resets")
    _hold("cartpole resets", S.reset_stats(got))


def test_cartpole_far_counters_and_seeds(dra):
    seeds = list(S.FAR_SEEDS) + [3]
    for c0 in S.FAR_COUNTERS:
        _same_bits(_cartpole_run(dra, seeds, c0, 3), S.cartpole_resets(seeds, c0, 3), "far cart-pole resets %d" % c0)


# ----------------------------------------------------------------------------------------------------------- synthetic Atari
def _fill(dra, seed, counter0, count, frame_bytes, done_period, n_actions=4):
    """dra_ring_fill_synthetic into a fresh ring, read back through the gather (history 1, one step: a sample IS its slot)
    -> frames u8 [count, frame_bytes], actions i64 [count], rewards f64 [count], masks i32 [count]."""
    from deeprl_amd import ops
    ring = ops.Ring(count + 1, frame_bytes, 8, 1, 1, 0.99)
    ring.fill_synthetic(0, count + 1, counter0, int(seed) & S.M64, n_actions=n_actions, done_period=done_period)
    idx = torch.arange(count, dtype=torch.int64, device=dra.Config.DEVICE)
    got = ring.gather(idx, (frame_bytes,), torch.uint8, torch.int64)
    torch.cuda.synchronize()
    out = [got[k].cpu().numpy() for k in ("state", "action", "reward", "mask")]
    ring.close()
    return out[0].reshape(count, frame_bytes), out[1], out[2], out[3]


def _atari_actions(seed, counters, n_actions):
    return ((S.mix64(S.atari_reward_words([seed], counters))[0] & np.uint64(0xFFFFFFFF)) % np.uint64(n_actions)).astype(np.int64)


@pytest.mark.parametrize("c", S.ATARI_CASES, ids=_ids(S.ATARI_CASES))
def test_fill_synthetic_is_the_restatements_and_follows_its_laws(dra, c):
    counters = [c["counter0"] + k for k in range(c["count"])]
    want_r, want_d = S.atari_reward_done(c["seeds"], counters, c["done_period"])
    rewards, dones = [], []
    for i, seed in enumerate(c["seeds"]):
        frames, act, rew, mask = _fill(dra, seed, c["counter0"], c["count"], 8, c["done_period"])
        _same_bits(rew, want_r[i], "atari[%s] seed %d reward" % (c["name"], seed))
        assert np.array_equal(mask, 1 - want_d[i].astype(np.int32)) and np.array_equal(act, _atari_actions(seed, counters, 4))
        _same_bits(frames, S.atari_frames(seed, counters, 8), "atari[%s] seed %d one-word frames" % (c["name"], seed))
        rewards.append(rew), dones.append(mask == 0)
    _hold("atari[%s]" % c["name"], S.atari_stats(c, np.stack(rewards), np.stack(dones)))


def test_fill_synthetic_frames_are_the_restatements_and_uniform_bytes(dra):
    c = S.ATARI_FRAME_CASE
    counters = [c["counter0"] + k for k in range(c["count"])]
    frames, _, _, _ = _fill(dra, c["seed"], c["counter0"], c["count"], c["frame_bytes"], 37)
    _same_bits(frames, S.atari_frames(c["seed"], counters, c["frame_bytes"]), "atari frames")
    _hold("atari frames", S.frame_stats(frames))


def test_fill_synthetic_far_counters_and_seeds(dra):
    for counter0, seed in [(c0, 11) for c0 in S.FAR_COUNTERS] + [(5, s) for s in S.FAR_SEEDS]:
        counters = [counter0 + k for k in range(4)]
        frames, act, rew, mask = _fill(dra, seed, counter0, 4, 7056, 3)
        want_r, want_d = S.atari_reward_done([seed], counters, 3)
        _same_bits(frames, S.atari_frames(seed, counters, 7056), "far atari (%d, %d) frames" % (counter0, seed))
        _same_bits(rew, want_r[0], "far atari (%d, %d) reward" % (counter0, seed))
        assert np.array_equal(mask, 1 - want_d[0].astype(np.int32)) and np.array_equal(act, _atari_actions(seed, counters, 4))


# ------------------------------------------------------------------------------------------------------- rollout-level draws
def test_ppo_rollout_draws_the_gauss_stream(dra):
    """One dra_ppo_mlp_rollout (the edge suite's 64 x 16 x 3 case): the stored actions, standardised with the float64 means of the
    stored observations and the policy's scale, are the restatement's normals of (noise seed, sampler step, global environment,
    dimension).  Bar: the kernel forms mean + scale * noise in fp32; its mean is within the project's fp32 bar (1e-5 of
    max(|mean|, 1) = 1e-5, the mean being a tanh) of the float64 forward, the noise within dra_gauss_sample's 1e-5, and the
    action's own rounding is 2^-24 |action|: |z - noise| <= (1e-5 + 2^-24 max|action|) / min scale + 1e-5."""
    import ctypes
    import ppo_mlp_edge_cases as E
    from deeprl_amd._lib import lib, stream_ptr
    from oracle import ppo_mlp_oracle as O
    from test_gpu_ppo_mlp_edges import _Rollout
    c = E.ROLLOUTS_BY_NAME["h16-n64-s17-three-component-tiers-idle-head-waves"]
    r = _Rollout(dra, c)
    lib.dra_ppo_mlp_rollout(ctypes.byref(r.cfg), ctypes.byref(r.actor.net), ctypes.byref(r.critic.net), ctypes.byref(r.io), stream_ptr())
    torch.cuda.synchronize()
    state, action = r.o["state"].cpu().double(), r.o["action"].cpu().double().numpy()
    t_len, n, a_dim = action.shape
    actor = {k: v.detach().double() for k, v in r.ref["actor"].items()}
    critic = {k: v.detach().double() for k, v in r.ref["critic"].items()}
    with torch.no_grad():
        mean = O.gaussian_forward(actor, critic, state.reshape(t_len * n, -1), noise=torch.zeros(t_len * n, a_dim, dtype=torch.float64))["mean"]
        scale = torch.nn.functional.softplus(actor["std"]).numpy().reshape(-1)
    z = (action - mean.numpy().reshape(t_len, n, a_dim)) / scale
    envs = [c["env0"] + i for i in range(n)]
    want = np.stack([S.gauss_draw(c["noise_seed"], c["sampler_step0"] + t, c["n_global"], envs, a_dim) for t in range(t_len)]).astype(np.float64)
    other = np.stack([S.gauss_draw(c["noise_seed"] + 1, c["sampler_step0"] + t, c["n_global"], envs, a_dim) for t in range(t_len)])
    bar = (1e-5 + 2.0 ** -24 * np.abs(action).max()) / scale.min() + S.GAUSS_ABS
    err = float(np.abs(z - want).max())
    print("ppo rollout: max |z - noise| %.3g (bar %.3g), %d draws, scale %.3g .. %.3g" % (err, bar, z.size, scale.min(), scale.max()))
    record_parity("stream_stats ppo_rollout gauss", z_minus_noise=err / bar, draws=z.size)
    assert err <= bar
    _hold("ppo_rollout gauss", S.gauss_stats(z, other))


def test_cat_rollout_draws_the_gumbel_stream(dra):
    """One dra_cat_mlp_rollout (the a2c_feature suite's 17 environments x 33 steps): every stored action is the float64 argmax of
    (logits of the stored observation + the restatement's Gumbel noise of (noise seed, sampler step, global environment)) -- the host
    suite holds every score gap of these cases above 1e-4, so no row is exempt -- and the actions, standardised with the float64
    softmax of those logits, have mean zero and no lag correlation."""
    import a2c_feature_cases as K
    import a2c_feature_restatement as R
    from feature_kernel_harness import _body
    from test_gpu_a2c_feature import _launch
    case = K.ROLLOUT_CASES[2]
    hidden, gate, n, t_len, horizon, padded, _ = case
    _, _, start = K.restated_rollout(case)
    out, _ = _launch(dra, case, start)
    assert out["rc"] == 0
    state, action = _body(out, "state"), _body(out, "action")
    with torch.no_grad():
        logits = R.forward(R.to_t(start["params"]), state.reshape(t_len * n, 4).astype(np.float64), gate)[0].numpy().reshape(t_len, n, 2)
    x = np.empty((t_len, n))
    for t in range(t_len):
        want, gap, _ = S.gumbel_draw(logits[t], K.NOISE_SEED, K.SAMPLER0 + t, K.ENV0_EXTRA)
        assert gap.min() >= K.MARGIN and np.array_equal(action[t], want), "cat rollout step %d" % t
        p1 = np.asarray([S.softmax64(l)[1] for l in logits[t]])
        x[t] = (action[t] - p1) / np.sqrt(p1 * (1.0 - p1))
    _hold("cat_rollout gumbel", [("mean", "z", S.z_mean(x, 0.0, 1.0)), ("lag_env", "z", S.z_lag(x, 1, 0.0, 1.0)),
                                 ("lag_step", "z", S.z_lag(x, 0, 0.0, 1.0))])
