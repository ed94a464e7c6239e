"""a2c_feature, host side (no GPU): envs.CartPole against an independent statement of the physics with libm trigonometry, its
terminations and resets, the Task names, the zoo entry against the Config the reference's examples.py::a2c_feature builds, the
committed fixtures against a live run of the reference (tests/golden/make_golden_a2c_feature.py), the restatement the GPU tests
lean on (tests/a2c_feature_restatement.py) against the reference's recorded A2CAgent.step, the Gumbel margins the GPU action
comparisons rest on, the ctypes mirrors of the rollout kernel's structs, and which configurations A2CAgent moves to the device."""
import ctypes
import json
import math
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import a2c_feature_cases as K
import a2c_feature_restatement as R
import ref_shim
from golden import crosscheck_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "a2c_feature")
RECORD = os.path.join(GOLDEN, "a2c_feature_config.json")
FIXTURE = os.path.join(GOLDEN, "a2c_feature_step.npz")
RANDOM = os.path.join(GOLDEN, "random_policy.json")
LEARNING = os.path.join(GOLDEN, "learning_reference.json")
TAGS = ("t5n5", "t3n2")

needs_ref = pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    """These tests seed np.random and switch the package's device; the tests after them see what they saw before."""
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


# ------------------------------------------------------------------------------------------ the environment
def _libm_step(s, a):
    """The published cart-pole equations, written independently of envs.CartPole: libm sine / cosine, the textbook grouping."""
    x, xd, th, thd = s
    gravity, m_cart, m_pole, length, f_mag, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
    total, pml = m_cart + m_pole, m_pole * length
    force = f_mag if a == 1 else -f_mag
    c, sn = math.cos(th), math.sin(th)
    temp = (force + pml * thd * thd * sn) / total
    thacc = (gravity * sn - c * temp) / (length * (4.0 / 3.0 - m_pole * c * c / total))
    xacc = temp - pml * thacc * c / total
    return (x + tau * xd, xd + tau * xacc, th + tau * thd, thd + tau * thacc)


def test_polynomials_are_sine_and_cosine():
    from deeprl_amd.envs import pcos, psin
    th = np.linspace(-0.45, 0.45, 10001)
    es = max(abs(psin(float(t)) - math.sin(float(t))) for t in th)
    ec = max(abs(pcos(float(t)) - math.cos(float(t))) for t in th)
    print("psin %.3e, pcos %.3e" % (es, ec))
    assert es <= 2e-16 and ec <= 2e-16


def test_physics_against_independent_trigonometry():
    """200 fixed actions from one start, limits lifted (the comparison is of the dynamics): every component within 1e-12."""
    from deeprl_amd.envs import CartPole
    e = CartPole(seed=7, horizon=10 ** 9)
    e.X = e.THETA = float("inf")
    s = tuple(float(v) for v in e.reset())
    # (a balancing controller with every seventh action flipped: the pole stays in the polynomials' range for 200 steps)
    worst = 0.0
    for t in range(200):
        a = int(s[2] + 0.5 * s[3] > 0.0) ^ int(t % 7 == 3)
        obs, reward, done, _ = e.step(a)
        s = _libm_step(s, a)
        worst = max(worst, float(np.abs(obs - np.asarray(s)).max()))
        assert reward == 1.0 and not done and abs(s[2]) < 0.45
        s = tuple(float(v) for v in s)
    print("worst component difference over 200 steps: %.3e" % worst)
    assert worst <= 1e-12 and e.c == 200


@pytest.mark.parametrize("which,value", [("x", 2.4000001), ("x", -2.4000001), ("th", 0.2094396), ("th", -0.2094396)])
def test_termination_at_each_threshold(which, value):
    from deeprl_amd.envs import CartPole
    for scale, want in ((1.0, True), (0.999, False)):
        e = CartPole(seed=1)
        e.reset()
        e.s = np.zeros(4)
        # the position moves with the OLD velocity: start one Euler step short of the threshold
        i = 0 if which == "x" else 2
        e.s[i], e.s[i + 1] = 0.0, value * scale / 0.02
        _, reward, done, info = e.step(1)
        assert done is want and reward == 1.0
        assert info['episodic_return'] == (1.0 if want else None)


def test_termination_at_the_horizon_and_auto_reset():
    from deeprl_amd.envs import CartPole, DummyVecEnv, cenv_reset_state
    envs = [CartPole(seed=5 + i, horizon=3) for i in range(2)]
    vec = DummyVecEnv(envs)
    first = vec.reset()
    for i, e in enumerate(envs):
        assert np.array_equal(first[i], [cenv_reset_state(5 + i, 0, j) for j in range(4)])
    for t in range(1, 8):
        obs, rew, done, info = vec.step([t % 2, 1 - t % 2])
        assert np.array_equal(rew, [1.0, 1.0])
        for i, e in enumerate(envs):
            assert done[i] == (t % 3 == 0) and e.c == t
            if done[i]:
                assert info[i]['episodic_return'] == 3.0 and e.steps == 0 and e.ret == 0.0
                assert np.array_equal(obs[i], [cenv_reset_state(5 + i, t, j) for j in range(4)])     # the reset stream's position: c
            else:
                assert info[i]['episodic_return'] is None


def test_task_names():
    import deeprl_amd.envs as envs
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t = envs.Task('classic-CartPole-v0', num_envs=3, seed=4)
    assert [type(e) for e in t.env.envs] == [envs.CartPole] * 3 and [e.seed for e in t.env.envs] == [4, 5, 6]
    assert t.observation_space.shape == (4,) and t.observation_space.low == -np.inf and t.observation_space.high == np.inf
    assert isinstance(t.action_space, envs.Discrete) and t.action_space.n == 2 and (t.state_dim, t.action_dim) == (4, 2)
    assert np.asarray(t.reset()).shape == (3, 4)
    envs._WARNED.discard('CartPole-v0')
    with pytest.warns(UserWarning, match="SYNTHETIC"):
        old = envs.Task('CartPole-v0', seed=4)
    assert type(old.env.envs[0]) is envs.SyntheticVector


def test_random_policy_mean_is_the_committed_one():
    rec = json.load(open(RANDOM))
    assert rec["episodes"] == 2000 and rec["mean"] == K.random_policy_mean(rec["episodes"], rec["seed"], rec["env_seed"])
    assert 15.0 < rec["mean"] < 30.0


def test_learning_reference_record():
    """The hand-regenerated record of the reference's own learning runs: at the chosen length its median is >= 2 x the bar, the
    bar is 2 x the committed random-policy mean, at least 5 seeds."""
    rec, rnd = json.load(open(LEARNING)), json.load(open(RANDOM))
    assert rec["random_policy_mean"] == rnd["mean"] and rec["bar"] == 2.0 * rnd["mean"] and len(rec["seeds"]) >= 5
    n = rec["n_learn"]
    assert n in (150000, 200000, 250000, 300000)
    assert rec["medians"][str(n)] >= 2.0 * rec["bar"]
    assert all(rec["medians"][str(m)] < 2.0 * rec["bar"] for m in (150000, 200000, 250000, 300000) if m < n)
    assert rec["medians"][str(n)] == float(np.median([r["ends"][str(n)]["last_mean"] for r in rec["runs"]]))


# ------------------------------------------------------------------------------------------ zoo and fixtures
def test_zoo_a2c_feature_equals_reference_example():
    import deeprl_amd as d
    from deeprl_amd import zoo
    rec = json.load(open(RECORD))
    want = rec["config"]
    assert rec["agent"] == zoo.ZOO["a2c_feature"]["agent"] == "A2CAgent"
    d.select_device(-1)
    np.random.seed(0)
    have = C.describe_config(zoo.config("a2c_feature", game=rec["game"]))
    assert rec["game"] == "classic-CartPole-v0"
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert want[k] == have[k], "%s: reference %s, zoo %s" % (k, want[k], have[k])
    assert callable(zoo.a2c_feature)


@needs_ref
def test_a2c_feature_fixtures_are_the_reference_output(tmp_path):
    """tests/golden/make_golden_a2c_feature.py run live in a fresh interpreter (importing the reference installs stand-in
    modules that must not leak into the other tests): the same records, the same arrays, bit for bit."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable] + flags + [os.path.join(ROOT, "tests", "golden", "make_golden_a2c_feature.py")],
                          env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = os.path.join(str(tmp_path), "a2c_feature")
    assert json.load(open(os.path.join(out, "a2c_feature_config.json"))) == json.load(open(RECORD))
    assert json.load(open(os.path.join(out, "random_policy.json"))) == json.load(open(RANDOM))
    fresh, committed = dict(np.load(os.path.join(out, "a2c_feature_step.npz"))), dict(np.load(FIXTURE))
    assert sorted(fresh) == sorted(committed)
    for k in committed:
        assert fresh[k].dtype == committed[k].dtype and np.array_equal(fresh[k], committed[k]), k


def test_fixture_holds_data_only_and_is_small():
    assert os.path.getsize(FIXTURE) < 256 * 1024 and os.path.getsize(RECORD) < 16 * 1024
    g = np.load(FIXTURE, allow_pickle=False)
    for tag in TAGS:
        t_len, n = int(g[tag + "_cfg"][6]), int(g[tag + "_cfg"][7])
        assert g[tag + "_states"].shape == (t_len + 1, n, 4) and g[tag + "_action"].shape == (t_len, n)
        assert (g[tag + "_reward"] == 1.0).all()
    assert (int(g["t5n5_cfg"][6]), int(g["t5n5_cfg"][7])) == (5, 5)
    assert (g["t3n2_mask"] == 0).any() and (g["t3n2_mask"] == 1).any()      # an episode ends inside the rollout


def _params(g, tag, which):
    pre = "%s_%s_" % (tag, which)
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_step(tag):
    """The fp64 restatement on the fixture's states, actions, rewards and masks: log_pi_a, entropy, v, advantage and return within
    1e-5 of each tensor's largest magnitude (floor 1: the reference ran in fp32), the parameters after the update within
    rtol 2e-5 / atol 2e-6 (the bars of the GPU update test, which compares the device path with the same fixture)."""
    g = np.load(FIXTURE)
    discount, tau, ent_w, v_w, clip, lr = [float(x) for x in g[tag + "_cfg"][:6]]
    init = _params(g, tag, "init")
    assert set(init) == set(R.KEYS)
    new, keep = R.a2c_update(init, g[tag + "_states"], g[tag + "_action"], g[tag + "_reward"], g[tag + "_mask"], discount, tau,
                             ent_w, v_w, clip, lr)
    for key in ("log_pi_a", "entropy", "v", "adv", "ret"):
        want = g["%s_%s" % (tag, key)].astype(np.float64)
        err = np.abs(keep[key] - want).max()
        assert err <= 1e-5 * max(1.0, np.abs(want).max()), (key, err)
    final = _params(g, tag, "final")
    assert set(final) == set(new)
    moved = 0
    for k in final:
        np.testing.assert_allclose(new[k], final[k], rtol=2e-5, atol=2e-6, err_msg=k)
        moved += int((final[k] != g["%s_init_%s" % (tag, k)]).sum())
    assert moved > 100          # the update moved the parameters: the comparison above is not of two copies of the start


def test_restatement_head_and_noise_match_torch():
    """head() against torch.distributions.Categorical; gumbel_noise() against the fp32 expression the kernels evaluate."""
    rs = np.random.RandomState(3)
    logits = torch.tensor(rs.randn(9, 2) * 2, dtype=torch.float64)
    action = rs.randint(0, 2, size=9)
    dist = torch.distributions.Categorical(logits=logits)
    lp, ent = R.head(logits, action)
    np.testing.assert_allclose(lp.numpy().reshape(-1), dist.log_prob(torch.tensor(action)).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ent.numpy().reshape(-1), dist.entropy().numpy(), rtol=1e-12, atol=1e-12)
    g = R.gumbel_noise(11, 5, np.arange(64), 2)
    assert g.shape == (64, 2) and np.isfinite(g).all() and len(np.unique(g)) == 128
    assert not np.array_equal(g, R.gumbel_noise(11, 6, np.arange(64), 2))
    assert np.array_equal(g[3:5], R.gumbel_noise(11, 5, np.arange(3, 5), 2))         # a row's noise does not depend on the shard


# ------------------------------------------------------------------------------------------ margins
@pytest.mark.parametrize("case", K.ROLLOUT_CASES, ids=K.case_id)
def test_rollout_cases_have_margin_and_cover_their_edges(case):
    """The smallest gap between the two Gumbel-perturbed logits of the fp64 restatement is >= 1e-4 (fp32 forwards differ from it
    by ~1e-6: no correct implementation picks another action), an fp32 run of the restatement picks the same actions, and the
    short-horizon cases do end episodes inside the rollout."""
    hidden, gate, n, t_len, horizon, padded, _ = case
    want, envs, start = K.restated_rollout(case)
    print("%s: margin %.3e, %d episodes ended" % (K.case_id(case), want["margin"], len(want["events"])))
    assert want["margin"] >= K.MARGIN and want["fp32_same_actions"]
    assert [e.c for e in envs] == [t_len] * n
    if horizon <= t_len:
        assert len(want["events"]) >= n * (t_len // horizon) and (want["mask"] == 0).sum() == len(want["events"])
        assert want["events"] == sorted(want["events"])                            # (step, environment) order
        assert all(r <= horizon for _, _, r in want["events"])
    if horizon == 3:
        assert len(want["events"]) > K.RING_CAP - K.RING_COUNT0                     # the GPU test's short ring wraps
    assert set(np.unique(want["action"])) <= {0, 1} and (len(np.unique(want["action"])) == 2 or n * t_len < 4)


def test_agent_case_has_margin():
    run = K.restated_agent_run()
    print("agent case: margin %.3e, %d episodes" % (run["margin"], len(run["events"])))
    assert run["margin"] >= K.MARGIN and run["fp32_same_actions"]
    assert len(run["events"]) >= 8 and (run["masks"] == 0).sum() == len(run["events"])
    moved = sum(int((np.asarray(run["params"][k], dtype=np.float32) != run["init"][k]).sum()) for k in run["init"])
    assert moved > 100


# ------------------------------------------------------------------------------------------ C ABI mirrors
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_cat_mlp_net", "dra_cat_mlp_rollout_io"])
def test_ctypes_mirror_matches_the_header(tmp_path, which):
    from deeprl_amd import cat_mlp
    from test_struct_layouts import _c_layout
    mirror = {"dra_cat_mlp_net": cat_mlp.Net, "dra_cat_mlp_rollout_io": cat_mlp.RolloutIO}[which]
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, which, names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_supported_shapes():
    from deeprl_amd import cat_mlp
    ok = cat_mlp.supported
    assert ok(4, 2, 64, 5, 2) and ok(4, 2, 16, 1, 1) and ok(4, 2, 32, 64, 2) and ok(4, 2, 64, 64, 1)
    assert not ok(5, 2, 64, 5, 2) and not ok(3, 2, 64, 5, 2) and not ok(4, 3, 64, 5, 2) and not ok(4, 1, 64, 5, 2)
    assert not ok(4, 2, 48, 5, 2) and not ok(4, 2, 128, 5, 2) and not ok(4, 2, 8, 5, 2)
    assert not ok(4, 2, 64, 65, 2) and not ok(4, 2, 64, 0, 2) and not ok(4, 2, 64, 5, 0) and not ok(4, 2, 64, 5, 3)


def test_ops_refuse_cpu_tensors():
    from deeprl_amd import ops
    from deeprl_amd._lib import DraError
    n = 3
    with pytest.raises(DraError):
        ops.cartpole_step(torch.zeros(n, 4, dtype=torch.float64), torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int32),
                          torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64), 200)


def test_rollout_refuses_unsupported_shapes_before_any_launch():
    """dra_cat_mlp_rollout validates on the host: null pointers and shapes outside the table are DRA_EINVAL without a device."""
    from deeprl_amd import cat_mlp
    from deeprl_amd._lib import lib
    net, io = cat_mlp.Net(), cat_mlp.RolloutIO()
    assert lib.dra_cat_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    net.param = 4096
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, 48, 2
    io.n_env, io.t_len, io.horizon, io.ring_cap, io.n_global = 5, 5, 200, 64, 5
    assert lib.dra_cat_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), None) == -22


# ------------------------------------------------------------------------------------------ eligibility
class _Dp:
    active = False


class _Flat:
    def __init__(self, params):
        self.params = list(params)


class _Fused:
    def __init__(self, params):
        self.flat = _Flat(params)


class _Agent:
    """What cat_mlp.why_not reads of an A2CAgent."""

    def __init__(self, d, network, **cfg):
        self.config = d.Config()
        self.config.num_workers = 5
        for k, v in cfg.items():
            setattr(self.config, k, v)
        self.network, self.dp, self.grad_hook = network, _Dp(), None
        self._fused = _Fused(network.parameters())


def _net(d, s=4, a=2, hidden=(64, 64), gate=torch.tanh, noisy=False, actor=None):
    return d.CategoricalActorCriticNet(s, a, d.FCBody(s, hidden_units=hidden, gate=gate, noisy_linear=noisy), actor_body=actor)


def test_eligibility_logic():
    """The network shapes and switches that keep A2CAgent on the host path, one at a time, each with its reason."""
    import torch.nn.functional as F
    import deeprl_amd as d
    from deeprl_amd import cat_mlp
    d.select_device(-1)
    yes = lambda *a: True
    assert cat_mlp.shape(_net(d)) == (4, 2, 64, 2)
    assert cat_mlp.shape(_net(d, gate=F.tanh)) == (4, 2, 64, 2) and cat_mlp.shape(_net(d, gate=F.relu, hidden=(16, 16))) == (4, 2, 16, 1)
    assert cat_mlp.why_not(_Agent(d, _net(d)), yes) is None and cat_mlp.eligible(_Agent(d, _net(d)), yes) == (4, 2, 64, 2)
    assert cat_mlp.shape(_net(d, hidden=(64, 64, 64))) is None                                   # a three-layer body
    assert cat_mlp.shape(_net(d, hidden=(64,))) is None                                          # a one-layer body
    assert cat_mlp.shape(_net(d, hidden=(64, 32))) is None                                       # unequal widths
    assert cat_mlp.shape(_net(d, noisy=True)) is None                                            # noisy layers
    assert cat_mlp.shape(_net(d, gate=torch.sigmoid)) is None                                    # a gate the kernel does not have
    assert cat_mlp.shape(_net(d, actor=d.FCBody(64, hidden_units=(64,)))) is None                # a parameterised actor body
    assert cat_mlp.shape(d.GaussianActorCriticNet(4, 2, actor_body=d.FCBody(4), critic_body=d.FCBody(4))) is None
    assert "network" in cat_mlp.why_not(_Agent(d, _net(d, hidden=(64, 32))), yes)
    assert "fused_a2c_cat" in cat_mlp.why_not(_Agent(d, _net(d), fused_a2c_cat=False), yes)
    seen = []
    no = lambda *a: seen.append(a) or False
    assert "not built for" in cat_mlp.why_not(_Agent(d, _net(d, s=6, a=3), num_workers=7), no) and seen == [(6, 3, 64, 7, 2)]
    assert cat_mlp.eligible(_Agent(d, _net(d, hidden=(48, 48)))) is None                         # the library's own table
    assert cat_mlp.eligible(_Agent(d, _net(d), num_workers=65)) is None
    hooked = _Agent(d, _net(d))
    hooked.grad_hook = lambda g: None
    assert "grad_hook" in cat_mlp.why_not(hooked, yes)
    parallel = _Agent(d, _net(d))
    parallel.dp = type("Dp", (), {"active": True})()
    assert "data parallel" in cat_mlp.why_not(parallel, yes)
    partial = _Agent(d, _net(d))
    partial._fused = _Fused(list(partial.network.parameters())[1:])     # an optimiser that does not own every parameter
    assert "optimiser" in cat_mlp.why_not(partial, yes)


def test_task_eligibility():
    """DeviceCartPoleVec.eligible: refuses without a device, and (with one pretended) each condition on the task and the
    normalisers."""
    import deeprl_amd as d
    from deeprl_amd import envs
    from deeprl_amd.device_env import DeviceCartPoleVec
    d.select_device(-1)
    cfg = d.Config()
    task = envs.Task('classic-CartPole-v0', num_envs=5, seed=1)
    assert DeviceCartPoleVec.eligible(task, cfg) is False               # no device
    d.Config.DEVICE = torch.device('cuda')                              # (pretended: eligible() builds nothing)
    assert DeviceCartPoleVec.eligible(task, cfg) is True
    cfg.device_env = False
    assert DeviceCartPoleVec.eligible(task, cfg) is False
    cfg.device_env = True
    cfg.state_normalizer = d.RescaleNormalizer(0.5)
    assert DeviceCartPoleVec.eligible(task, cfg) is False
    cfg.state_normalizer = d.MeanStdNormalizer()
    assert DeviceCartPoleVec.eligible(task, cfg) is False
    cfg.state_normalizer = d.RescaleNormalizer()
    cfg.reward_normalizer = d.SignNormalizer()
    assert DeviceCartPoleVec.eligible(task, cfg) is False
    cfg.reward_normalizer = d.RescaleNormalizer(0.1)
    assert DeviceCartPoleVec.eligible(task, cfg) is True
    assert DeviceCartPoleVec.eligible(envs.Task('classic-CartPole-v0', num_envs=65, seed=1), cfg) is False
    mixed = envs.Task('classic-CartPole-v0', num_envs=2, seed=1)
    mixed.env.envs[1].horizon = 7
    assert DeviceCartPoleVec.eligible(mixed, cfg) is False

    class Sub(envs.Task):
        pass
    assert DeviceCartPoleVec.eligible(Sub('classic-CartPole-v0', num_envs=2, seed=1), cfg) is False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert DeviceCartPoleVec.eligible(envs.Task('CartPole-v0', num_envs=2, seed=1), cfg) is False


def test_agent_without_a_device_keeps_the_host_path(monkeypatch):
    """On the CPU A2CAgent on the zoo configuration keeps host environments (the path the parent commit ran)."""
    import deeprl_amd as d
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import envs, zoo
    from deeprl_amd.device_env import DeviceCartPoleVec
    d.select_device(-1)

    class _Quiet:
        def info(self, *a, **k):
            pass
        add_scalar = add_histogram = warning = info

    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Quiet())
    cfg = zoo.config("a2c_feature", game="classic-CartPole-v0")
    agent = d.A2CAgent(cfg)
    assert not isinstance(agent.task, DeviceCartPoleVec) and agent._cat_rollout is None and agent._mlp_rollout is None
    assert type(agent.task.env.envs[0]) is envs.CartPole and len(agent.task.env.envs) == 5
    assert np.asarray(agent.states).shape == (5, 4) and agent.episodes() == []
    agent.close()
