"""CPU checks of the fused DDPG / TD3 update's host side: the fixture is the reference's own output, the fp64 restatement
(tests/dpg_restatement.py: what the GPU tests hold csrc/dpg_mlp.hip to) reproduces the recorded reference updates, dpg_mlp's
shape / eligibility decisions, the ctypes mirrors, and dra_dpg_supported at the edges of its range."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dpg_cases as K
import dpg_restatement as R
import ref_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


@needs_ref
def test_fixture_is_the_reference_output(tmp_path):
    """tests/golden/make_golden_ddpg_td3_update.py run live in a fresh interpreter: the same arrays, bit for bit."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable] + flags + [os.path.join(ROOT, "tests", "golden", "make_golden_ddpg_td3_update.py")],
                          env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    fresh = dict(np.load(os.path.join(str(tmp_path), "ddpg_td3", "ddpg_td3_update.npz")))
    committed = dict(np.load(K.FIXTURE))
    assert sorted(fresh) == sorted(committed)
    for k in committed:
        assert fresh[k].dtype == committed[k].dtype and np.array_equal(fresh[k], committed[k]), k


def test_fixture_holds_data_only_and_covers_the_edges():
    assert os.path.getsize(K.FIXTURE) < 1024 * 1024
    g = np.load(K.FIXTURE, allow_pickle=False)
    hp, delay = K.fixture_hyper(g)
    assert (hp["td3_noise"], hp["td3_noise_clip"], delay) == (0.2, 0.3, 2)
    assert [int(x) for x in g["b8_dims"]] == [8, 5, 2, 16, 16] and [int(x) for x in g["b20_dims"]] == [20, 7, 3, 20, 12]
    for case, (nc, policy) in K.FIXTURE_CASES.items():
        mask = g[case + "_batch_mask"]
        assert (mask == 0).any() and (mask == 1).any()
        assert int(g[case + "_before_t_critic"]) >= 1                    # Adam's moments are not the zero start
        if nc == 2:
            bound = np.abs(g[case + "_noise"] * hp["td3_noise"]) > hp["td3_noise_clip"]
            assert bound.any() and not bound.all()
            assert bool(int(g[case + "_total_steps"]) % delay) == policy     # the cadence test of TD3_agent.py:100


@pytest.mark.parametrize("case", sorted(K.FIXTURE_CASES))
def test_restatement_reproduces_the_reference_update(case):
    """The restatement from the recorded "before" state on the recorded batch (and noise): every "after" tensor -- online and
    target parameters, both Adam moments -- within rtol 2e-5 / atol 2e-6 (the bar test_a2c_continuous_host.py holds its
    restatement to), the step counts exactly; a critic-only step leaves actor and targets bit-unchanged."""
    g = np.load(K.FIXTURE)
    hp, _ = K.fixture_hyper(g)
    st, batch, noise, after = K.fixture_case(g, case)
    nc, policy = K.FIXTURE_CASES[case]
    before_online = {k: v.clone() for k, v in st.online.items()}
    before_target = {k: v.clone() for k, v in st.target.items()}
    st.update(batch, hp, policy_step=policy, noise=noise)
    assert (st.t_actor, st.t_critic) == (after["t_actor"], after["t_critic"])
    moved = 0
    for name, have in (("online", st.online), ("target", st.target), ("m", st.m), ("v", st.v)):
        assert set(have) == set(after[name])
        for k in have:
            np.testing.assert_allclose(have[k].numpy(), after[name][k].numpy(), rtol=2e-5, atol=2e-6, err_msg="%s %s" % (name, k))
    for k in st.online:
        moved += int((after["online"][k] != before_online[k]).sum())
        if not policy:
            assert torch.equal(after["target"][k], before_target[k])
            if k.startswith("a."):
                assert torch.equal(after["online"][k], before_online[k]) and torch.equal(st.online[k], before_online[k])
    assert moved > 100


def test_restatement_noise_stream_is_the_kernels():
    """hash_noise is oracle.ppo_mlp_oracle.gauss_noise at (seed, t = counter, n_global = B, rows, A): consecutive counters give
    different draws, the same counter the same draw."""
    a, b, c = R.hash_noise(7, 3, 17, 2), R.hash_noise(7, 4, 17, 2), R.hash_noise(7, 3, 17, 2)
    assert a.shape == (17, 2) and a.dtype == np.float32 and np.array_equal(a, c) and not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ shape / eligibility
def _ddpg_net(d, s=17, a=6, actor=(400, 300), critic=(400, 300), gates=(torch.relu, torch.relu), opt=None, **kw):
    opt = opt or (lambda p: torch.optim.Adam(p, lr=1e-3))
    return d.DeterministicActorCriticNet(s, a, actor_opt_fn=opt, critic_opt_fn=opt, actor_body=d.FCBody(s, actor, gate=gates[0]),
                                         critic_body=d.FCBody(s + a, critic, gate=gates[1]), **kw)


def _td3_net(d, s=17, a=6, actor=(400, 300), critics=((400, 300), (400, 300)), gate=torch.relu, noisy=False):
    opt = lambda p: torch.optim.Adam(p, lr=1e-3)
    widths = iter(critics)
    return d.TD3Net(a, actor_body_fn=lambda: d.FCBody(s, actor, gate=gate, noisy_linear=noisy),
                    critic_body_fn=lambda: d.FCBody(s + a, next(widths), gate=gate), actor_opt_fn=opt, critic_opt_fn=opt)


class _Space:
    def __init__(self, low, high):
        self.low, self.high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)


class _Agent:
    """What dpg_mlp.why_not reads of a DDPGAgent / TD3Agent."""

    def __init__(self, d, make_net, batch=100, space=None, wrap=False, **cfg):
        self.config = d.Config()
        self.config.fused_dpg_update = True
        for k, v in cfg.items():
            setattr(self.config, k, v)
        self.network, self.target_network = make_net(), make_net()
        rp = d.UniformReplay(memory_size=1000, batch_size=batch)
        self.replay = type("Wrap", (), {"replay": rp})() if wrap else rp
        self.task = type("Task", (), {"action_space": space or _Space(-np.ones(6), np.ones(6))})()


def test_shape_decisions():
    import torch.nn.functional as F
    import deeprl_amd as d
    from deeprl_amd import dpg_mlp
    d.select_device(-1)
    assert dpg_mlp.shape(_ddpg_net(d)) == (17, 6, 400, 300, 1, 1)
    assert dpg_mlp.shape(_td3_net(d)) == (17, 6, 400, 300, 1, 2)
    assert dpg_mlp.shape(_ddpg_net(d, s=5, a=2, actor=(16, 12), critic=(16, 12), gates=(torch.tanh, F.tanh))) == (5, 2, 16, 12, 2, 1)
    assert dpg_mlp.shape(_td3_net(d, noisy=True)) is None                                            # a noisy layer
    assert dpg_mlp.shape(_ddpg_net(d, gates=(torch.relu, torch.tanh))) is None                       # two gates
    assert dpg_mlp.shape(_ddpg_net(d, gates=(torch.sigmoid, torch.sigmoid))) is None                 # another gate
    assert dpg_mlp.shape(_ddpg_net(d, phi_body=d.FCBody(17, (17,)))) is None                         # a non-identity phi_body
    assert dpg_mlp.shape(_td3_net(d, critics=((400, 300), (400, 200)))) is None                      # unequal critic bodies
    assert dpg_mlp.shape(_ddpg_net(d, actor=(400, 300), critic=(300, 300))) is None                  # actor and critic widths differ
    assert dpg_mlp.shape(_ddpg_net(d, actor=(64, 64, 64), critic=(64, 64, 64))) is None              # three-layer bodies
    no_bias = _ddpg_net(d)
    no_bias.critic_body.layers[1].bias = None
    assert dpg_mlp.shape(no_bias) is None                                                            # a missing bias
    assert dpg_mlp.shape(d.VanillaNet(4, d.FCBody(17))) is None


def test_eligibility_decisions():
    import deeprl_amd as d
    from deeprl_amd import dpg_mlp
    d.select_device(-1)
    assert getattr(d.Config(), "fused_dpg_update", False) is False                                   # the switch defaults off
    ddpg, td3 = (lambda: _ddpg_net(d)), (lambda: _td3_net(d))
    assert dpg_mlp.why_not(_Agent(d, ddpg)) is None and dpg_mlp.eligible(_Agent(d, td3, wrap=True))
    assert "off" in dpg_mlp.why_not(_Agent(d, ddpg, fused_dpg_update=False))
    assert "off" in dpg_mlp.why_not(_Agent(d, ddpg, fused_dpg_update=1))                             # True itself, nothing truthy
    assert "network" in dpg_mlp.why_not(_Agent(d, lambda: _td3_net(d, noisy=True)))
    for bad in (lambda p: torch.optim.Adam(p, lr=1e-3, amsgrad=True), lambda p: torch.optim.Adam(p, lr=1e-3, weight_decay=1e-2),
                lambda p: torch.optim.Adam(p, lr=1e-3, maximize=True), lambda p: torch.optim.RMSprop(p, lr=1e-3),
                lambda p: torch.optim.AdamW(p, lr=1e-3)):
        assert "Adam" in dpg_mlp.why_not(_Agent(d, lambda: _ddpg_net(d, opt=bad)))
    assert "dra_dpg_supported" in dpg_mlp.why_not(_Agent(d, ddpg, batch=129))                        # the replay's batch size
    assert "dra_dpg_supported" in dpg_mlp.why_not(_Agent(d, lambda: _ddpg_net(d, actor=(600, 300), critic=(600, 300))))
    assert "bounds" in dpg_mlp.why_not(_Agent(d, ddpg, space=_Space([-1, -1, -2, -1, -1, -1], np.ones(6))))
    per = _Agent(d, ddpg)
    per.replay = d.PrioritizedReplay(memory_size=1000, batch_size=100)
    assert "UniformReplay" in dpg_mlp.why_not(per)
    # the decision itself does not need the library: a refusing dra_dpg_supported is reported as such
    assert "dra_dpg_supported" in dpg_mlp.why_not(_Agent(d, ddpg), supported_fn=lambda *a: False)


# ------------------------------------------------------------------------------------------ C ABI
@pytest.mark.parametrize("which", ["dra_dpg_net", "dra_dpg_batch", "dra_dpg_step"])
def test_ctypes_mirror_matches_the_header(tmp_path, which):
    import ctypes
    from deeprl_amd import dpg_mlp
    from test_struct_layouts import _c_layout
    mirror = {"dra_dpg_net": dpg_mlp.Net, "dra_dpg_batch": dpg_mlp.Batch, "dra_dpg_step": dpg_mlp.Step}[which]
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, which, names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_supported_range_edges():
    """dra_dpg_supported (host-only) returns 0 exactly for 1 <= B <= 128, S <= 64, A <= 16, H1, H2 <= 512, gate relu / tanh,
    one or two critics; dra_dpg_workspace_floats refuses the same shapes and otherwise covers what the kernels store."""
    import ctypes
    from deeprl_amd import dpg_mlp
    from deeprl_amd._lib import lib
    ok = dpg_mlp.supported
    good = dict(batch=100, state_dim=17, action_dim=6, h1=400, h2=300, gate=1, n_critics=1)
    assert ok(**good) and ok(**dict(good, n_critics=2, gate=2))
    assert ok(1, 1, 1, 1, 1, 1, 1) and ok(128, 64, 16, 512, 512, 2, 2)
    for key, lo, hi in (("batch", 1, 128), ("state_dim", 1, 64), ("action_dim", 1, 16), ("h1", 1, 512), ("h2", 1, 512),
                        ("gate", 1, 2), ("n_critics", 1, 2)):
        assert ok(**dict(good, **{key: lo})) and ok(**dict(good, **{key: hi}))
        assert not ok(**dict(good, **{key: lo - 1})) and not ok(**dict(good, **{key: hi + 1}))
        assert lib.dra_dpg_supported.raw(*[dict(good, **{key: hi + 1})[k] for k in good]) == -22
    n = ctypes.c_int64(-1)
    assert lib.dra_dpg_workspace_floats.raw(129, 17, 6, 400, 300, 1, ctypes.byref(n)) == -22 and n.value == -1
    assert lib.dra_dpg_workspace_floats.raw(100, 17, 6, 400, 300, 1, None) == -22
    for nc in (1, 2):
        b, s, a, h1, h2 = 100, 17, 6, 400, 300
        want = 4 * b + b * (s + a) + nc * (2 * b * (h1 + h2) + b) + 2 * b * (h1 + h2) + 2 * b * a
        assert dpg_mlp.workspace_floats(b, (s, a, h1, h2, 1, nc)) == want


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every other entry point returns -EINVAL outside the range (checked before anything touches a device)."""
    import ctypes
    from deeprl_amd import dpg_mlp
    from deeprl_amd._lib import lib
    net = dpg_mlp.Net()
    net.param = 4096
    net.state_dim, net.action_dim, net.h1, net.h2, net.gate, net.n_critics = 17, 6, 513, 300, 1, 1
    batch, step = dpg_mlp.Batch(), dpg_mlp.Step()
    batch.state = batch.next_state = batch.action = batch.reward = batch.mask = 4096
    batch.state_stride = batch.next_state_stride = 17
    batch.action_stride, batch.batch = 6, 100
    step.exp_avg = step.exp_avg_sq = 4096
    step.step_size, step.inv_sqrt_bc2, step.beta1, step.beta2, step.eps = 1e-3, 1.0, 0.9, 0.999, 1e-8
    ws = ctypes.c_void_p(4096)
    ref = ctypes.byref
    assert lib.dra_dpg_critic_update.raw(ref(net), ref(net), ref(batch), ref(step), ws, None) == -22     # h1 = 513
    assert lib.dra_dpg_actor_update.raw(ref(net), ref(batch), ref(step), ws, None) == -22
    assert lib.dra_dpg_act.raw(ref(net), ws, 17, 0, 1, ws, None) == -22
    net.h1 = 400
    assert lib.dra_dpg_act.raw(ref(net), ws, 17, 0, 129, ws, None) == -22                                # n = 129
    assert lib.dra_dpg_act.raw(ref(net), ws, 16, 0, 1, ws, None) == -22                                  # rows overlap
    batch.batch = 129
    assert lib.dra_dpg_critic_update.raw(ref(net), ref(net), ref(batch), ref(step), ws, None) == -22
    batch.batch = 100
    net.actor[2] = -4
    assert lib.dra_dpg_actor_update.raw(ref(net), ref(batch), ref(step), ws, None) == -22                # a negative offset
    assert lib.dra_dpg_critic_update.raw(None, ref(net), ref(batch), ref(step), ws, None) == -22
