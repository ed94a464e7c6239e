"""GPU tests of a2c_continuous on device-resident rollouts: the Gaussian head kernels and the rollout kernel of csrc/a2c_mlp.hip
against the fp64 restatement (tests/a2c_mlp_restatement.py, pinned to the reference's own run by
tests/test_a2c_continuous_host.py), the fused head's autograd Function against the module path, one update against the reference's
recorded A2CAgent.step, and A2CAgent's device path against the host path it replaces, graph replay against eager, save / load.
Bars: exact for rewards, masks, counters and stream positions; 1e-5 of a tensor's largest magnitude (floor 1) for fp32 results."""
import ctypes
import os

import numpy as np
import pytest
import torch
from parity_log import record_parity

import a2c_mlp_cases as K
import a2c_mlp_restatement as R
from a2c_mlp_edge_cases import STD_VALUES, head_case as _head_case  # noqa: F401  (one generator for both head suites)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "a2c_continuous", "a2c_continuous_step.npz")


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


class _Rec:
    """A logger that keeps the episodic-return lines."""

    def __init__(self):
        self.lines = []

    def info(self, msg, *a, **k):
        self.lines.append(str(msg))

    def add_scalar(self, *a, **k):
        pass
    add_histogram = add_scalar


def _within(got, want, what):
    """1e-5 of the tensor's largest magnitude, floor 1.0 (the bar of test_rollout_kernel_matches_oracle)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    bar = 1e-5 * max(float(np.abs(want).max()) if want.size else 0.0, 1.0)
    print("%s: max abs error %.3e (bar %.3e)" % (what, err, bar))
    assert err <= bar, (what, err, bar)
    return err / bar


# ------------------------------------------------------------------------------------------ head kernels
@pytest.mark.parametrize("n,a", [(1, 1), (67, 7), (80, 6), (256, 16)])
def test_gauss_head_kernels_match_restatement(dra, n, a):
    """dra_gauss_head_fwd / _bwd against the fp64 restatement: mean, log_pi_a, entropy, dz and dstd within 1e-5 of each tensor's
    largest magnitude (floor 1); two backward launches on the same input give the same dstd bits."""
    from deeprl_amd import ops
    dev = dra.Config.DEVICE
    z, std, action, g_lp, g_ent = _head_case(n, a)
    up = lambda x: torch.from_numpy(x).to(dev)
    zt, st, at, glt, get = up(z), up(std), up(action), up(g_lp), up(g_ent)
    mean, lp, ent = ops.gauss_head_fwd(zt, st, at)
    dz, dstd = ops.gauss_head_bwd(zt, st, at, glt, get)
    dz2, dstd2 = ops.gauss_head_bwd(zt, st, at, glt, get)
    torch.cuda.synchronize()
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)
    w_mean, w_lp, w_ent = R.head(t64(z), t64(std), t64(action))
    w_dz, w_dstd = R.head_grads(z, std, action, g_lp, g_ent)
    errs = dict(mean=_within(mean.cpu().numpy(), w_mean.numpy(), "mean"), log_pi_a=_within(lp.cpu().numpy(), w_lp.numpy(), "log_pi_a"),
                entropy=_within(ent.cpu().numpy(), w_ent.numpy(), "entropy"), dz=_within(dz.cpu().numpy(), w_dz, "dz"),
                dstd=_within(dstd.cpu().numpy(), w_dstd, "dstd"))
    record_parity("gauss head kernels vs fp64 restatement [%d,%d] (fraction of the bar)" % (n, a), **errs)
    assert np.array_equal(dstd.cpu().numpy().view(np.uint32), dstd2.cpu().numpy().view(np.uint32))
    assert np.array_equal(dz.cpu().numpy().view(np.uint32), dz2.cpu().numpy().view(np.uint32))
    assert np.abs(w_mean.numpy()).max() > 0.999 or n * a < 4        # the case does reach the saturated tanh


def _gauss_net(d, s_dim=17, a_dim=6, hidden=64, gate=torch.relu, seed=21):
    torch.manual_seed(seed)
    net = d.GaussianActorCriticNet(s_dim, a_dim, actor_body=d.FCBody(s_dim, hidden_units=(hidden, hidden), gate=gate),
                                   critic_body=d.FCBody(s_dim, hidden_units=(hidden, hidden), gate=gate))
    with torch.no_grad():       # (the heads start at 1e-3 scale and std at 0: move them so that every term matters)
        net.fc_action.weight.mul_(300.0)
        net.fc_critic.weight.mul_(300.0)
        net.std.copy_(torch.linspace(-1.0, 1.5, a_dim))
    return net


def _forward_backward(net, obs, action, g):
    for p in net.parameters():
        p.grad = None
    out = net(obs, action)
    torch.autograd.backward([out['log_pi_a'], out['entropy'], out['v']], list(g))
    return ({k: v.detach().cpu().numpy().copy() for k, v in out.items()},
            {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()})


@pytest.mark.parametrize("n", [80, 320])
def test_fused_head_function_matches_module_path(dra, n):
    """GaussianActorCriticNet.forward(obs, action) with fused_gauss_head on against the same network with it off (torch's
    tanh / softplus / Normal): all five outputs and every parameter's gradient within 1e-5 of scale.  80 rows are the
    a2c_continuous update; 320 rows (64 workers x 5 steps) take the head kernels past one workgroup of rows."""
    dev = dra.Config.DEVICE
    net = _gauss_net(dra)
    rs = np.random.RandomState(8)
    obs = torch.from_numpy(rs.randn(n, 17).astype(np.float32)).to(dev)
    with torch.no_grad():
        action = net(obs)['action'].clone()
    g = [torch.from_numpy(rs.randn(n, 1).astype(np.float32)).to(dev) for _ in range(3)]
    assert net.fused_gauss_head is False
    want_out, want_grad = _forward_backward(net, obs, action, g)
    net.fused_gauss_head = True
    got_out, got_grad = _forward_backward(net, obs, action, g)
    torch.cuda.synchronize()
    assert sorted(got_out) == sorted(want_out) == ['action', 'entropy', 'log_pi_a', 'mean', 'v']
    errs = {k: _within(got_out[k], want_out[k], k) for k in want_out}
    errs.update({"grad " + k: _within(got_grad[k], want_grad[k], "grad " + k) for k in want_grad})
    record_parity("fused gauss head Function vs module path [%d rows] (fraction of the bar)" % n, **errs)
    assert np.abs(want_grad['std']).max() > 1e-3 and np.abs(want_grad['actor_body.layers.0.weight']).max() > 1e-4


def test_network_without_the_switch_is_the_module_path(dra):
    """A GaussianActorCriticNet built without the switch gives, bit for bit, what torch's own operations give on its layers'
    outputs (the path PPO and every existing test see)."""
    dev = dra.Config.DEVICE
    net = _gauss_net(dra, gate=torch.tanh)
    rs = np.random.RandomState(2)
    obs = torch.from_numpy(rs.randn(9, 17).astype(np.float32)).to(dev)
    action = torch.from_numpy(rs.randn(9, 6).astype(np.float32)).to(dev)
    with torch.no_grad():
        out = net(obs, action)
        mean = torch.tanh(net.fc_action(net.actor_body(obs)))
        dist = torch.distributions.Normal(mean, torch.nn.functional.softplus(net.std))
        assert torch.equal(out['mean'], mean) and torch.equal(out['v'], net.fc_critic(net.critic_body(obs)))
        assert torch.equal(out['log_pi_a'], dist.log_prob(action).sum(-1).unsqueeze(-1))
        assert torch.equal(out['entropy'], dist.entropy().sum(-1).unsqueeze(-1))


# ------------------------------------------------------------------------------------------ rollout kernel
_ORDER = ["actor_body.layers.0.weight", "actor_body.layers.0.bias", "actor_body.layers.1.weight", "actor_body.layers.1.bias",
          "fc_action.weight", "fc_action.bias", "critic_body.layers.0.weight", "critic_body.layers.0.bias",
          "critic_body.layers.1.weight", "critic_body.layers.1.bias", "fc_critic.weight", "fc_critic.bias", "std"]


def _net_struct(params, dev, s_dim, a_dim, hidden, gate):
    from deeprl_amd import a2c_mlp
    offs, chunks, off = {}, [], 3          # (a leading gap: the offsets are not assumed to start at zero)
    chunks.append(np.full(3, np.nan, dtype=np.float32))
    for k in _ORDER:
        v = params[k].reshape(-1)
        offs[k] = off
        pad = (-v.size) % 4 + 1
        chunks += [v, np.full(pad, np.nan, dtype=np.float32)]
        off += v.size + pad
    flat = torch.from_numpy(np.concatenate(chunks)).to(dev)
    net = a2c_mlp.Net()
    net.param = flat.data_ptr()
    (net.a_w1, net.a_b1, net.a_w2, net.a_b2, net.a_w3, net.a_b3, net.c_w1, net.c_b1, net.c_w2, net.c_b2, net.c_w3, net.c_b3,
     net.off_std) = [offs[k] for k in _ORDER]
    net.state_dim, net.action_dim, net.hidden, net.gate = s_dim, a_dim, hidden, {"relu": 1, "tanh": 2}[gate]
    return net, flat


@pytest.mark.parametrize("case", K.ROLLOUT_CASES, ids=lambda c: "n%d_t%d_s%d_a%d_h%d_%s_%s" % c[:7])
def test_rollout_kernel_matches_restatement(dra, case):
    """dra_a2c_mlp_rollout against the restatement (fp64 forwards, oracle environment, oracle normaliser, oracle noise): rewards,
    masks, counters and the sampler position exact; stored observations, actions, values and the final normalised observation
    within 1e-5 of the largest magnitude; raw environment state and observation statistics at the relative bars of
    test_rollout_kernel_matches_oracle."""
    from deeprl_amd import a2c_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    n, t_len, s_dim, a_dim, hidden, gate, kind, horizon = case
    want, envs, norm, start = K.restated_rollout(case)
    if t_len == 7:
        assert want["terminals"] >= 3
    assert a2c_mlp.supported(s_dim, a_dim, hidden, n, {"relu": 1, "tanh": 2}[gate])
    net, flat = _net_struct(start["params"], dev, s_dim, a_dim, hidden, gate)
    flat_before = flat.cpu().numpy().view(np.uint32).copy()
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    env_state, env_counter = t(start["raw"], torch.float64), torch.zeros(n, dtype=torch.int64, device=dev)
    env_seed = torch.tensor(start["seeds"], dtype=torch.int64, device=dev)
    rms = t(start["rms"], torch.float64)
    cur_state = torch.full((n, s_dim), float("nan"), dtype=torch.float32, device=dev)
    sampler = torch.full((1,), K.SAMPLER0, dtype=torch.int64, device=dev)
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    o = dict(state=f(t_len, n, s_dim), action=f(t_len, n, a_dim), v=f(t_len + 1, n), reward=f(t_len, n), mask=f(t_len, n))
    io = a2c_mlp.RolloutIO()
    io.env_state, io.env_counter, io.env_seed, io.rms = env_state.data_ptr(), env_counter.data_ptr(), env_seed.data_ptr(), rms.data_ptr()
    io.cur_state, io.sampler_step = cur_state.data_ptr(), sampler.data_ptr()
    io.out_state, io.out_action, io.out_v = o['state'].data_ptr(), o['action'].data_ptr(), o['v'].data_ptr()
    io.out_reward, io.out_mask = o['reward'].data_ptr(), o['mask'].data_ptr()
    io.env0, io.n_global, io.noise_seed, io.horizon = K.ENV0_EXTRA, n + K.ENV0_EXTRA + 1, K.NOISE_SEED, horizon
    io.reward_coef, io.t_len, io.n_env = 1.0, t_len, n
    if kind == "identity":
        io.rms_epsilon, io.rms_clip, io.rms_update = 0.0, float("inf"), 0
    else:
        io.rms_epsilon, io.rms_clip, io.rms_update = 1e-8, 10.0, 1 if kind == "meanstd-update" else 0
    lib.dra_a2c_mlp_rollout(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    assert int(sampler.cpu()[0]) == K.SAMPLER0 + t_len + 1
    assert np.array_equal(env_counter.cpu().numpy(), [e.c for e in envs])
    assert np.array_equal(o['mask'].cpu().numpy(), want['mask'])
    assert np.array_equal(o['reward'].cpu().numpy(), want['reward'])
    errs = {key: _within(o[key].cpu().numpy(), want[key], key) for key in ('state', 'action', 'v')}
    errs['cur_state'] = _within(cur_state.cpu().numpy(), want['cur_state'], 'cur_state')
    record_parity("a2c_mlp rollout kernel vs restatement %s (fraction of the bar)" % (case,), **errs)
    np.testing.assert_allclose(env_state.cpu().numpy(), want['raw_states'], rtol=1e-6, atol=1e-8)
    h = rms.cpu().numpy()
    if kind == "meanstd-update":
        np.testing.assert_allclose(h[:s_dim], norm.rms.mean.reshape(-1), rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(h[s_dim:2 * s_dim], norm.rms.var.reshape(-1), rtol=1e-7)
        assert h[2 * s_dim] == norm.rms.count and norm.rms.count > start["rms"][2 * s_dim]
    else:
        assert np.array_equal(h, start["rms"])
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), flat_before)       # (the parameter buffer is read only)


# ------------------------------------------------------------------------------------------ update against the reference
def _bare_agent(d, g, tag):
    """An A2CAgent with everything _learn_stacked reads and nothing else (no task: the rollout comes from the fixture)."""
    from deeprl_amd.dist import DataParallel
    from deeprl_amd.optim import FusedOptimizer
    discount, tau, ent_w, v_w, clip, lr, t_len, n, s_dim, a_dim, hidden = [float(x) for x in g[tag + "_cfg"]]
    cfg = d.Config()
    cfg.discount, cfg.use_gae, cfg.gae_tau, cfg.entropy_weight, cfg.value_loss_weight = discount, True, tau, ent_w, v_w
    cfg.gradient_clip, cfg.rollout_length, cfg.num_workers = clip, int(t_len), int(n)
    agent = d.A2CAgent.__new__(d.A2CAgent)
    agent.config, agent.grad_hook = cfg, None
    agent.dp = DataParallel(cfg)
    agent.network = d.GaussianActorCriticNet(int(s_dim), int(a_dim),
                                             actor_body=d.FCBody(int(s_dim), hidden_units=(int(hidden), int(hidden))),
                                             critic_body=d.FCBody(int(s_dim), hidden_units=(int(hidden), int(hidden))))
    pre = tag + "_init_"
    agent.network.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    agent.optimizer = torch.optim.RMSprop(agent.network.parameters(), lr=lr)
    agent._fused = FusedOptimizer.adopt(agent.optimizer)
    return agent


@pytest.mark.parametrize("tag", ["t5n16", "t3n2"])
def test_update_with_fused_head_matches_reference_step(dra, tag):
    """The fixture's initial parameters, states, actions, values, rewards and masks through A2CAgent._learn_stacked with the
    fused head on: the parameters after the update against the reference's own A2CAgent.step (rtol 2e-5 / atol 2e-6, the bars
    of test_ppo_optimize_matches_reference for the same network family)."""
    dev = dra.Config.DEVICE
    g = np.load(FIXTURE)
    agent = _bare_agent(dra, g, tag)
    agent.network.fused_gauss_head = True
    t_len, n = g[tag + "_reward"].shape[:2]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    states = up(g[tag + "_states"][:t_len].reshape(t_len * n, -1))
    actions = up(g[tag + "_action"].reshape(t_len * n, -1))
    out4 = agent._learn_stacked(states, actions, up(g[tag + "_v"]), up(g[tag + "_reward"]), up(g[tag + "_mask"]))
    torch.cuda.synchronize()
    assert np.isfinite(out4.cpu().numpy()).all()
    worst = 0.0
    for k, v in agent.network.state_dict().items():
        got, want = v.cpu().numpy(), g["%s_final_%s" % (tag, k)]
        worst = max(worst, float(np.max(np.abs(got - want) / (2e-6 + 2e-5 * np.abs(want)))))
    print("%s: worst parameter error as a fraction of atol + rtol |want|: %.3f" % (tag, worst))
    record_parity("a2c_continuous update (fused head) vs reference step %s (fraction of the bar)" % tag, params=worst)
    for k, v in agent.network.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), g["%s_final_%s" % (tag, k)], rtol=2e-5, atol=2e-6, err_msg=k)
    agent.dp.close()


# ------------------------------------------------------------------------------------------ the agent
N_ENV, T_LEN, DONE_PERIOD, STEPS = 4, 5, 7, 6


def _config(d, device_env, graph=True):
    from deeprl_amd import zoo
    c = zoo.config("a2c_continuous", game="synthetic-continuous-HalfCheetah", tag="a2c_mlp%d%d" % (device_env, graph),
                   device_env=device_env, dp_invariant_sampling=True, dp_noise_seed=11, graph_update=graph,
                   overrides=dict(num_workers=N_ENV, rollout_length=T_LEN))
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=3, synthetic_done_period=DONE_PERIOD)
    c.log_interval = 10 ** 9
    return c


def _make_agent(d, monkeypatch, device_env, graph=True):
    import deeprl_amd.agents as agents_mod
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    d.random_seed(9)
    torch.manual_seed(9)
    torch.cuda.manual_seed_all(9)
    agent = d.A2CAgent(_config(d, device_env, graph))
    return agent, rec


def _snapshot(agent, rec):
    torch.cuda.synchronize()
    return dict(params={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
                total=agent.total_steps, lines=list(rec.lines), sampler=agent.dp.sampler_state(),
                rng=np.random.randint(0, 1 << 30, size=3))


def _run(d, monkeypatch, device_env, graph=True, steps=STEPS):
    from deeprl_amd.device_env import DeviceContinuousVec
    agent, rec = _make_agent(d, monkeypatch, device_env, graph)
    assert isinstance(agent.task, DeviceContinuousVec) == bool(device_env)
    assert agent.network.fused_gauss_head == bool(device_env)
    for _ in range(steps):
        agent.step()
    out = _snapshot(agent, rec)
    out['graphed'] = agent._dev_graph.graph is not None
    out['launches'] = agent._mlp_rollout.launches if agent._mlp_rollout is not None else 0
    agent.close()
    return out


@pytest.fixture(scope="module")
def device_run(dra):
    """Six steps of the device path with graph replay: shared by the tests below, left unchanged."""
    mp = pytest.MonkeyPatch()
    try:
        return _run(dra, mp, True, True)
    finally:
        mp.undo()


def test_agent_device_rollout_equals_host_environments(dra, monkeypatch, device_run):
    """A2CAgent on the a2c_continuous configuration (4 environments, rollout length 5, episodes of about 7 steps) over
    DeviceContinuousVec -- one rollout launch, the fused head, graph replay from the third step -- against the same agent
    stepping envs.SyntheticContinuous from python (the parent commit's path), both on the same hashed action noise: total_steps,
    the episodic-return log lines and the np.random tail equal; parameters within 2e-4 of each tensor's largest magnitude
    (floor 1e-2: the two paths run different forward kernels, the bar of the PPO test of the same name)."""
    a, b = device_run, _run(dra, monkeypatch, False)
    assert a['graphed'] and not b['graphed'] and b['launches'] == 0
    assert a['launches'] == 3          # two eager rollouts and the capture pass; the replays launch from the graph
    assert a['total'] == b['total'] == STEPS * T_LEN * N_ENV
    assert a['lines'] == b['lines'] and len(a['lines']) >= 4
    assert np.array_equal(a['rng'], b['rng'])
    assert a['sampler'] == b['sampler'] == dict(noise_seed=11, step=STEPS * (T_LEN + 1))
    worst = 0.0
    for k in a['params']:
        scale = max(np.abs(b['params'][k]).max(), 1e-2)
        worst = max(worst, float(np.max(np.abs(a['params'][k] - b['params'][k])) / (2e-4 * scale)))
    print("device vs host parameters: worst fraction of the bar %.3f" % worst)
    record_parity("a2c_continuous agent device vs host path (fraction of the bar)", params=worst)
    for k in a['params']:
        scale = max(np.abs(b['params'][k]).max(), 1e-2)
        assert np.max(np.abs(a['params'][k] - b['params'][k])) <= 2e-4 * scale, k


def test_graph_replay_equals_eager(dra, monkeypatch, device_run):
    """config.graph_update = False keeps every step eager: after 6 steps the parameters are equal to the bit."""
    b = _run(dra, monkeypatch, True, graph=False)
    assert device_run['graphed'] and not b['graphed'] and b['launches'] == STEPS
    assert device_run['total'] == b['total'] and device_run['lines'] == b['lines'] and device_run['sampler'] == b['sampler']
    for k in device_run['params']:
        assert np.array_equal(device_run['params'][k].view(np.uint32), b['params'][k].view(np.uint32)), k


def test_save_load_continues_the_run(dra, monkeypatch, device_run, tmp_path):
    """3 steps, save, load into a fresh agent, 3 more steps == 6 uninterrupted steps, on the parameters and the sampler position.
    save() writes what the reference's checkpoint holds (parameters, normaliser statistics) plus the noise stream's seed and
    position; the environments and the optimiser's running averages are no part of a checkpoint, so the test carries them over
    by hand -- what is left to differ is exactly what save / load is responsible for."""
    first, rec = _make_agent(dra, monkeypatch, True)
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    name = str(tmp_path / "ckpt")
    first.save(name)
    assert os.path.isfile(name + ".sampler")
    second, rec2 = _make_agent(dra, monkeypatch, True)
    assert second.dp.sampler_state()['step'] == 0
    second.load(name)
    assert second.dp.sampler_state() == dict(noise_seed=11, step=3 * (T_LEN + 1))
    for key in ("env_state", "env_counter", "cur_state", "rms"):
        getattr(second.task, key).copy_(getattr(first.task, key))
    second.task.counters_host[:], second.task.ret_host[:] = first.task.counters_host, first.task.ret_host
    second._fused.state1.copy_(first._fused.state1)
    second._fused.state2.copy_(first._fused.state2)
    second._fused.steps, second.total_steps = first._fused.steps, first.total_steps
    for _ in range(3):
        second.step()
    got = _snapshot(second, rec2)
    first.close()
    second.close()
    assert got['total'] == device_run['total'] and got['sampler'] == device_run['sampler']
    assert rec.lines + got['lines'] == device_run['lines']
    for k in got['params']:
        assert np.array_equal(got['params'][k].view(np.uint32), device_run['params'][k].view(np.uint32)), k


def test_ppo_agent_keeps_its_own_path(dra, monkeypatch):
    """PPOAgent on the same task and network family still moves the task to the device for ITS rollout kernel
    (dra_ppo_mlp_rollout) and leaves the network's fused head off."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd.device_env import DeviceContinuousVec
    d = dra
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    c = d.Config()
    c.merge(dict(game="synthetic-continuous-HalfCheetah", log_level=0, tag="a2c_mlp_ppo_guard", skip=False, dp_invariant_sampling=True,
                 dp_noise_seed=11))
    c.num_workers = N_ENV
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=3, synthetic_done_period=DONE_PERIOD)
    c.eval_env = d.Task(c.game, seed=4)
    c.network_fn = lambda: d.GaussianActorCriticNet(c.state_dim, c.action_dim, actor_body=d.FCBody(c.state_dim, gate=torch.tanh),
                                                    critic_body=d.FCBody(c.state_dim, gate=torch.tanh))
    c.actor_opt_fn = lambda p: torch.optim.Adam(p, 3e-4)
    c.critic_opt_fn = lambda p: torch.optim.Adam(p, 1e-3)
    c.discount, c.use_gae, c.gae_tau, c.gradient_clip = 0.99, True, 0.95, 0.5
    c.rollout_length, c.optimization_epochs, c.mini_batch_size = 8, 2, 16
    c.ppo_ratio_clip, c.max_steps, c.target_kl = 0.2, 3e6, 0.01
    c.state_normalizer = d.MeanStdNormalizer()
    c.log_interval = 10 ** 9
    d.random_seed(9)
    agent = d.PPOAgent(c)
    assert isinstance(agent.task, DeviceContinuousVec) and agent._mlp.usable()
    assert agent.network.fused_gauss_head is False and not hasattr(agent, "_mlp_rollout")
    before = agent._mlp.launches
    agent.step()
    torch.cuda.synchronize()
    assert agent._mlp.launches == before + 1 and agent.total_steps == 8 * N_ENV
    agent.close()
