"""a2c_continuous, host side (no GPU): the zoo entry against the Config the reference's examples.py::a2c_continuous builds, the
committed fixtures against a live run of the reference (tests/golden/make_golden_a2c_continuous.py), the fp64 restatement the GPU
tests lean on (tests/a2c_mlp_restatement.py) against the reference's recorded A2CAgent.step, the ctypes mirrors of the rollout
kernel's structs, and which configurations A2CAgent moves to the device."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import a2c_mlp_restatement as R
import ref_shim
from golden import crosscheck_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "a2c_continuous")
RECORD = os.path.join(GOLDEN, "a2c_continuous_config.json")
FIXTURE = os.path.join(GOLDEN, "a2c_continuous_step.npz")
TAGS = ("t5n16", "t3n2")

needs_ref = pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    """These tests seed np.random and switch the package's device; the tests after them see what they saw before."""
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


def test_zoo_a2c_continuous_equals_reference_example():
    import deeprl_amd as d
    from deeprl_amd import zoo
    rec = json.load(open(RECORD))
    want = rec["config"]
    assert rec["agent"] == zoo.ZOO["a2c_continuous"]["agent"] == "A2CAgent"
    d.select_device(-1)
    np.random.seed(0)
    have = C.describe_config(zoo.config("a2c_continuous", game=rec["game"]))
    assert rec["game"] == "HalfCheetah-v2"
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert want[k] == have[k], "%s: reference %s, zoo %s" % (k, want[k], have[k])
    assert callable(zoo.a2c_continuous)


@needs_ref
def test_a2c_continuous_fixtures_are_the_reference_output(tmp_path):
    """tests/golden/make_golden_a2c_continuous.py run live in a fresh interpreter (importing the reference installs stand-in
    modules that must not leak into the other tests): the same record, the same arrays, bit for bit."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable] + flags + [os.path.join(ROOT, "tests", "golden", "make_golden_a2c_continuous.py")],
                          env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = os.path.join(str(tmp_path), "a2c_continuous")
    assert json.load(open(os.path.join(out, "a2c_continuous_config.json"))) == json.load(open(RECORD))
    fresh, committed = dict(np.load(os.path.join(out, "a2c_continuous_step.npz"))), dict(np.load(FIXTURE))
    assert sorted(fresh) == sorted(committed)
    for k in committed:
        assert fresh[k].dtype == committed[k].dtype and np.array_equal(fresh[k], committed[k]), k


def test_fixture_holds_data_only_and_is_small():
    assert os.path.getsize(FIXTURE) < 256 * 1024 and os.path.getsize(RECORD) < 16 * 1024
    g = np.load(FIXTURE, allow_pickle=False)
    for tag in TAGS:
        t_len, n = int(g[tag + "_cfg"][6]), int(g[tag + "_cfg"][7])
        assert g[tag + "_states"].shape[:2] == (t_len + 1, n) and g[tag + "_action"].shape[:2] == (t_len, n)
        assert (g[tag + "_mask"] == 0).any() and (g[tag + "_mask"] == 1).any()      # an episode ends inside the rollout


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
    new, keep = R.a2c_update(_params(g, tag, "init"), g[tag + "_states"], g[tag + "_action"], g[tag + "_reward"], g[tag + "_mask"],
                             discount, tau, ent_w, v_w, clip, lr)
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


def test_restatement_head_matches_torch_distributions():
    """head() / head_grads() against torch.distributions.Normal in fp64, softplus on both sides of its threshold."""
    rs = np.random.RandomState(3)
    n, a = 9, 6
    z = torch.tensor(rs.randn(n, a) * 2, dtype=torch.float64, requires_grad=True)
    std = torch.tensor([-8.0, 0.0, 3.0, 19.9, 20.1, 30.0], dtype=torch.float64, requires_grad=True)
    scale = torch.nn.functional.softplus(std)
    action = (torch.tanh(z) + scale * torch.tensor(rs.randn(n, a), dtype=torch.float64)).detach()
    dist = torch.distributions.Normal(torch.tanh(z), scale)
    lp, ent = dist.log_prob(action).sum(-1, keepdim=True), dist.entropy().sum(-1, keepdim=True)
    mean, lp2, ent2 = R.head(z, std, action)
    np.testing.assert_allclose(lp2.detach().numpy(), lp.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ent2.detach().numpy(), ent.detach().numpy(), rtol=1e-12, atol=1e-12)
    g_lp, g_ent = rs.randn(n, 1), rs.randn(n, 1)
    torch.autograd.backward([lp, ent], [torch.tensor(g_lp), torch.tensor(g_ent)])
    dz, dstd = R.head_grads(z.detach().numpy(), std.detach().numpy(), action.numpy(), g_lp, g_ent)
    np.testing.assert_allclose(dz, z.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(dstd, std.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_restatement_rollout_case_with_short_horizon_has_terminals():
    """The second rollout case of tests/a2c_mlp_cases.py, which tests/test_gpu_a2c_continuous.py runs (5 environments, 7 steps,
    horizon 3): the restatement alone produces at least 3 terminals there, and the counters / statistics advance as stated."""
    import a2c_mlp_cases as G
    case = G.ROLLOUT_CASES[1]
    assert (case[0], case[1], case[5], case[6]) == (5, 7, "tanh", "meanstd-update")
    want, envs, norm, _ = G.restated_rollout(case)
    assert want["terminals"] >= 3
    assert [e.c for e in envs] == [case[1]] * case[0]
    assert norm.rms.count == pytest.approx(G.WARM_ROWS + 1e-4 + (case[1] + 1) * case[0])


# ------------------------------------------------------------------------------------------ C ABI mirrors
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_a2c_mlp_net", "dra_a2c_mlp_rollout_io"])
def test_ctypes_mirror_matches_the_header(tmp_path, which):
    from deeprl_amd import a2c_mlp
    from test_struct_layouts import _c_layout
    mirror = {"dra_a2c_mlp_net": a2c_mlp.Net, "dra_a2c_mlp_rollout_io": a2c_mlp.RolloutIO}[which]
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, which, names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_supported_shapes():
    from deeprl_amd import a2c_mlp
    ok = a2c_mlp.supported
    assert ok(17, 6, 64, 16, 1) and ok(17, 6, 64, 16, 2) and ok(64, 16, 64, 64, 1) and ok(1, 1, 32, 1, 2)
    assert not ok(65, 6, 64, 16, 1) and not ok(17, 17, 64, 16, 1) and not ok(17, 6, 48, 16, 1) and not ok(17, 6, 16, 16, 1)
    assert not ok(17, 6, 64, 65, 1) and not ok(17, 6, 64, 0, 1) and not ok(17, 6, 64, 16, 0) and not ok(17, 6, 64, 16, 3)


def test_ops_refuse_cpu_tensors():
    from deeprl_amd import ops
    from deeprl_amd._lib import DraError
    z, std, a = torch.zeros(4, 2), torch.zeros(2), torch.zeros(4, 2)
    with pytest.raises(DraError):
        ops.gauss_head_fwd(z, std, a)
    with pytest.raises(DraError):
        ops.gauss_head_bwd(z, std, a, torch.zeros(4, 1), torch.zeros(4, 1))


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
    """What a2c_mlp.eligible reads of an A2CAgent."""

    def __init__(self, d, network, **cfg):
        self.config = d.Config()
        self.config.num_workers = 16
        for k, v in cfg.items():
            setattr(self.config, k, v)
        self.network, self.dp, self.grad_hook = network, _Dp(), None
        self._fused = _Fused(network.parameters())


def _net(d, s=17, a=6, actor=(64, 64), critic=(64, 64), gates=(torch.relu, torch.relu), phi=None, noisy=False):
    feat = s if phi is None else phi.feature_dim
    return d.GaussianActorCriticNet(s, a, phi_body=phi,
                                    actor_body=d.FCBody(feat, hidden_units=actor, gate=gates[0], noisy_linear=noisy),
                                    critic_body=d.FCBody(feat, hidden_units=critic, gate=gates[1]))


def test_eligibility_logic():
    """The network shapes and switches that keep A2CAgent on the host path, one at a time."""
    import torch.nn.functional as F
    import deeprl_amd as d
    from deeprl_amd import a2c_mlp
    d.select_device(-1)
    assert a2c_mlp.shape(_net(d)) == (17, 6, 64, 1)
    assert a2c_mlp.shape(_net(d, gates=(F.relu, torch.relu))) == (17, 6, 64, 1)
    assert a2c_mlp.shape(_net(d, s=5, a=2, actor=(32, 32), critic=(32, 32), gates=(torch.tanh, torch.tanh))) == (5, 2, 32, 2)
    assert a2c_mlp.eligible(_Agent(d, _net(d))) == (17, 6, 64, 1)
    assert a2c_mlp.shape(_net(d, gates=(torch.tanh, torch.relu))) is None                       # a tanh / relu mix
    assert a2c_mlp.shape(_net(d, actor=(64, 64, 64), critic=(64, 64, 64))) is None              # three-layer bodies
    assert a2c_mlp.shape(_net(d, actor=(64, 32), critic=(64, 32))) is None                      # unequal widths inside a body
    assert a2c_mlp.shape(_net(d, actor=(64, 64), critic=(32, 32))) is None                      # unequal widths across bodies
    assert a2c_mlp.shape(_net(d, phi=d.FCBody(17, hidden_units=(17,)))) is None                 # a parameterised phi_body
    assert a2c_mlp.shape(_net(d, noisy=True)) is None                                           # noisy layers
    assert a2c_mlp.shape(_net(d, gates=(torch.sigmoid, torch.sigmoid))) is None                 # a gate the kernel does not have
    assert a2c_mlp.shape(d.CategoricalActorCriticNet(17, 6, d.FCBody(17))) is None
    assert a2c_mlp.eligible(_Agent(d, _net(d), fused_a2c_mlp=False)) is None
    assert a2c_mlp.eligible(_Agent(d, _net(d, actor=(48, 48), critic=(48, 48)))) is None        # a width the kernel is not built for
    assert a2c_mlp.eligible(_Agent(d, _net(d), num_workers=65)) is None
    hooked = _Agent(d, _net(d))
    hooked.grad_hook = lambda g: None
    assert a2c_mlp.eligible(hooked) is None
    parallel = _Agent(d, _net(d))
    parallel.dp = type("Dp", (), {"active": True})()
    assert a2c_mlp.eligible(parallel) is None
    partial = _Agent(d, _net(d))
    partial._fused = _Fused(list(partial.network.parameters())[1:])     # an optimiser that does not own every parameter
    assert a2c_mlp.eligible(partial) is None


def test_agent_without_a_device_keeps_the_host_path_and_the_module_head(monkeypatch):
    """On the CPU A2CAgent on the zoo configuration steps host environments (the path the parent commit ran); the network's
    fused head stays off and forward() is torch.distributions' arithmetic."""
    import deeprl_amd as d
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    from deeprl_amd.device_env import DeviceContinuousVec
    d.select_device(-1)

    class _Quiet:
        def info(self, *a, **k):
            pass
        add_scalar = add_histogram = info

    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Quiet())
    cfg = zoo.config("a2c_continuous", game="synthetic-continuous-HalfCheetah", overrides=dict(num_workers=2))
    agent = d.A2CAgent(cfg)
    assert not isinstance(agent.task, DeviceContinuousVec) and agent._mlp_rollout is None
    assert agent.network.fused_gauss_head is False
    agent.close()
