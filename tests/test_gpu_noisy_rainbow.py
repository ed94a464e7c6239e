"""Rainbow's noisy layers on csrc/noisy.hip: the kernels against an fp64 restatement of network_utils.py:54-62 written here,
the dueling combination and the device-beta PER weights, RainbowNet against the reference's recorded outputs
(tests/golden/rainbow_dueling.npz), and the `rainbow` agent case of tests/test_gpu_rainbow_dueling.py with the actor forward
and the PER update replayed from captured graphs.

Bars.  Contractions: 1e-5 of each tensor's maximum (the project's bar for contractions; fp32 summation of either arithmetic form
sits 3-5e-7 from fp64 at these shapes).  Module / agent level: the bars of tests/test_gpu_rainbow_dueling.py."""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_envs  # noqa: E402
from golden.make_golden_cases import RAINBOW_SHAPES, HEAD_AGENT_CASES, digest, head_inputs, trajectory_digest  # noqa: E402
from parity_log import check_gated, check_trajectory, record_parity  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rainbow_dueling.npz")
SHAPES = [(1, 3136, 512), (32, 3136, 512), (64, 3136, 512), (1, 512, 204), (32, 512, 51), (32, 512, 204), (32, 512, 918),
          (32, 4, 64), (5, 7, 3)]
BAR = 1e-5


class _Quiet:
    def info(self, *a, **k):
        pass

    def add_scalar(self, *a, **k):
        pass

    def add_histogram(self, *a, **k):
        pass


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


def _f(e):
    return e.sign() * e.abs().sqrt()


def _noisy_ref64(x, wmu, wsig, bmu, bsig, e_in, e_out, e_b, act):
    """network_utils.py:54-62 + transform_noise in fp64 with autograd: y, and a function from the gradient of the pre-activation
    to the gradients of (x, weight_mu, weight_sigma, bias_mu, bias_sigma)."""
    t = [v.double().clone().requires_grad_(True) for v in (x, wmu, wsig, bmu, bsig)]
    x64, wm, ws, bm, bs = t
    w = wm + ws * torch.outer(_f(e_out.double()), _f(e_in.double()))
    b = bm + bs * _f(e_b.double())
    pre = x64 @ w.t() + b
    y = torch.relu(pre) if act == "relu" else pre

    def grads(gpre):
        (pre * gpre.double()).sum().backward()
        return [v.grad for v in t]
    return y.detach(), grads


def _rel(got, want):
    scale = max(float(want.abs().max()), 1e-30)
    return float((got.double().cpu() - want.cpu()).abs().max()) / scale


@pytest.mark.parametrize("std", [0.5, 0.1])
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_noisy_linear_kernels_match_fp64(dra, shape, act, std):
    ops = dra.ops
    rows, k, n = shape
    gen = torch.Generator().manual_seed(1000 * rows + k + n + (7 if act else 0) + int(std * 100))
    r = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    x = r(rows, k)
    if act == "relu":
        x = torch.relu(x)          # the layer below ends in a ReLU: exercises the x_relu mask on real zeros
    bound = 1.0 / np.sqrt(k)
    wmu, bmu = (torch.rand(n, k, generator=gen) * 2 - 1) * bound, (torch.rand(n, generator=gen) * 2 - 1) * bound
    wsig, bsig = torch.full((n, k), 0.5 / np.sqrt(k)) * (1 + 0.1 * r(n, k)), torch.full((n,), 0.5 / np.sqrt(n)) * (1 + 0.1 * r(n))
    e_in, e_out, e_b = r(k) * std, r(n) * std, r(n) * std
    g = r(rows, n)
    y64, grads64 = _noisy_ref64(x, wmu, wsig, bmu, bsig, e_in, e_out, e_b, act)
    c = [v.cuda() for v in (x, wmu, wsig, bmu, bsig, e_in, e_out, e_b)]
    y = ops.noisy_linear_fwd(*c, act=act)
    y2 = ops.noisy_linear_fwd(*c, act=act)
    gpre = g.cuda() * (y > 0) if act == "relu" else g.cuda()       # (ReLU of the output applied by the caller, as _LinearFn does)
    dx64, dwm64, dws64, dbm64, dbs64 = grads64(gpre.cpu())
    args = (gpre.contiguous(), c[0], c[1], c[2], c[5], c[6], c[7])
    out = ops.noisy_linear_bwd(*args)
    out2 = ops.noisy_linear_bwd(*args)
    errs = dict(y=_rel(y, y64))
    for name, got, want in zip(("dx", "dw_mu", "dw_sigma", "db_mu", "db_sigma"), out, (dx64, dwm64, dws64, dbm64, dbs64)):
        errs[name] = _rel(got, want)
    # the mask of the layer below: dx * [x > 0], and another head's input gradient added in the same launch
    add = r(rows, k).cuda()
    dxm = ops.noisy_linear_bwd(*args, x_relu=True, dx_add=add)[0]
    want_m = (dx64 + add.double().cpu()) * (x > 0)
    errs["dx_masked_added"] = float((dxm.double().cpu() - want_m).abs().max()) / max(float(want_m.abs().max()), float(dx64.abs().max()))
    print("noisy %s act=%s std=%s: %s" % (shape, act, std, {a: "%.2e" % b for a, b in errs.items()}))
    record_parity("noisy_linear %dx%dx%d act=%s std=%s" % (rows, k, n, act, std), **errs)
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(out, out2)), "two calls differ"
    for name, e in errs.items():
        assert e <= BAR, (name, e)


@pytest.mark.parametrize("rows", [1, 32])
@pytest.mark.parametrize("n_actions", [4, 6, 18])
def test_dueling_atoms_match_fp64(dra, rows, n_actions):
    ops = dra.ops
    gen = torch.Generator().manual_seed(rows * 100 + n_actions)
    v, a, g = torch.randn(rows, 51, generator=gen), torch.randn(rows, n_actions, 51, generator=gen), torch.randn(rows, n_actions, 51, generator=gen)
    v64, a64 = v.double().requires_grad_(True), a.double().requires_grad_(True)
    want = v64.view(rows, 1, 51) + (a64 - a64.mean(1, keepdim=True))
    (want * g.double()).sum().backward()
    got = ops.dueling_atoms_fwd(v.cuda(), a.cuda())
    dv, da = ops.dueling_atoms_bwd(g.cuda())
    errs = dict(logits=_rel(got, want.detach()), d_value=_rel(dv, v64.grad), d_advantage=_rel(da, a64.grad))
    record_parity("dueling_atoms rows=%d A=%d" % (rows, n_actions), **errs)
    for name, e in errs.items():
        assert e <= BAR, (name, e)


@pytest.mark.parametrize("beta", [0.4, 0.7, 1.0])
def test_per_weights_dev_equals_per_weights(dra, beta):
    ops = dra.ops
    gen = torch.Generator().manual_seed(5)
    loss = torch.rand(32, generator=gen).cuda() * 3
    sp = (torch.rand(32, generator=gen) * 1e-3 + 1e-6).cuda()
    prio, w = ops.per_weights(loss, sp, beta, 0.01, 0.5)
    prio_d, w_d = ops.per_weights_dev(loss, sp, torch.tensor([beta], dtype=torch.float32).cuda(), 0.01, 0.5)
    assert torch.equal(prio, prio_d) and torch.equal(w, w_d)
    _, w_only = ops.per_weights_dev(None, sp, torch.tensor([beta], dtype=torch.float32).cuda(), 0.01, 0.5)
    assert torch.equal(w, w_only)


def _load(net, shapes, seed):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in fake_envs.numpy_params(shapes, seed).items()}, strict=False)


def _module_run(d, fused):
    x, _, wl = head_inputs()
    d.Config.NOISY_LAYER_STD = 0.5
    torch.manual_seed(9)
    net = d.RainbowNet(4, 51, d.NatureConvBody(noisy_linear=True), noisy_linear=True)
    net.set_fused_noisy(fused)
    _load(net, RAINBOW_SHAPES, 33)
    torch.manual_seed(11)
    net.reset_noise()
    net.train()
    o = net(d.ImageNormalizer()(x))
    (o["log_prob"] * torch.from_numpy(wl).cuda()).sum().backward()
    return net, o


def test_rainbow_module_runs_on_the_noisy_kernels(dra, monkeypatch):
    d = dra
    g = np.load(GOLDEN)
    calls = dict(fwd=0, bwd=0, dueling=0, outer=0)
    for name, key in (("noisy_linear_fwd", "fwd"), ("noisy_linear_bwd", "bwd"), ("dueling_atoms_fwd", "dueling")):
        real = getattr(d.ops, name)

        def counted(*a, _real=real, _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(d.ops, name, counted)
    real_outer = torch.outer

    def outer(*a, **k):
        calls["outer"] += 1
        return real_outer(*a, **k)
    net, o = _module_run(d, True)
    monkeypatch.setattr(torch, "outer", outer)
    calls.update(fwd=0, bwd=0, dueling=0, outer=0)
    torch.manual_seed(11)
    net.reset_noise()
    net.zero_grad()
    x, _, wl = head_inputs()
    o = net(d.ImageNormalizer()(x))
    (o["log_prob"] * torch.from_numpy(wl).cuda()).sum().backward()
    assert calls == dict(fwd=3, bwd=3, dueling=1, outer=0), calls
    monkeypatch.setattr(torch, "outer", real_outer)
    np.testing.assert_allclose(o["prob"].detach().cpu().numpy(), g["rainbow_prob"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(o["log_prob"].detach().cpu().numpy(), g["rainbow_log_prob"], rtol=1e-5, atol=1e-6)
    worst = 0.0
    for n, prm in net.named_parameters():
        got, want = digest(prm.grad.detach().cpu().numpy()), g["rainbow_grad_" + n]
        scale = max(float(np.abs(want[2:]).max()), 1e-30)
        worst = max(worst, float(np.abs(got[2:] - want[2:]).max()) / scale)
        np.testing.assert_allclose(got[2:], want[2:], rtol=1e-5, atol=1e-5 * scale, err_msg=n)
        np.testing.assert_allclose(got[:2], want[:2], rtol=1e-4, atol=1e-4 * max(abs(float(want[1])), 1e-30) ** 0.5, err_msg=n + " (sums)")
    # kernels on / off: the same function, within 1e-5 of each tensor's scale
    net_off, o_off = _module_run(d, False)
    on_off = dict(prob=_rel(o["prob"].detach(), o_off["prob"].detach().double()))
    for (n, p), (_, q) in zip(net.named_parameters(), net_off.named_parameters()):
        on_off[n] = _rel(p.grad, q.grad.double())
    record_parity("rainbow_module_fused", grad_rel_to_tensor_max=worst, on_off_max=max(on_off.values()))
    for n, e in on_off.items():
        assert e <= 1e-5, (n, e)
    # the lazily formed products are what the reference keeps in its state dict
    sd = net.state_dict()
    f = d.NoisyLinear.transform_noise
    for layer in ("fc_value", "fc_advantage", "body.fc4"):
        m = net.get_submodule(layer)
        assert torch.equal(sd[layer + ".weight_epsilon"], real_outer(f(m.noise_out_weight), f(m.noise_in)))
        assert torch.equal(sd[layer + ".bias_epsilon"], f(m.noise_out_bias))


def _rainbow_agent(d, monkeypatch, **overrides):
    import deeprl_amd.agents as agents_mod
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Quiet())
    d.Config.NOISY_LAYER_STD = 0.5
    cfg = d.Config()
    cfg.merge(dict(game="synthetic-atari", n_step=1, replay_cls=d.PrioritizedReplay, async_replay=False, log_level=0, tag="rainbow",
                   noisy_linear=True))
    cfg.merge(overrides)
    cfg.task_fn = lambda: d.Task(cfg.game, seed=7, synthetic_done_period=8)
    cfg.eval_env = cfg.task_fn()
    cfg.optimizer_fn = lambda p: torch.optim.Adam(p, lr=0.000625, eps=1.5e-4)
    cfg.categorical_v_max, cfg.categorical_v_min, cfg.categorical_n_atoms = 10, -10, 51
    cfg.network_fn = lambda: d.RainbowNet(cfg.action_dim, cfg.categorical_n_atoms, d.NatureConvBody(noisy_linear=True),
                                          noisy_linear=True)
    cfg.random_action_prob = d.LinearSchedule(1.0, 0.05, 60)
    cfg.batch_size, cfg.discount, cfg.history_length = 32, 0.99, 4
    kw = dict(memory_size=500, batch_size=32, n_step=1, discount=0.99, history_length=4)
    cfg.replay_fn = lambda: d.ReplayWrapper(cfg.replay_cls, kw, cfg.async_replay)
    cfg.replay_eps, cfg.replay_alpha = 0.01, 0.5
    cfg.replay_beta = d.LinearSchedule(0.4, 1.0, 1000)
    cfg.state_normalizer, cfg.reward_normalizer = d.ImageNormalizer(), d.SignNormalizer()
    cfg.target_network_update_freq, cfg.exploration_steps, cfg.sgd_update_frequency = 3, 40, 4
    cfg.gradient_clip, cfg.double_q, cfg.async_actor, cfg.max_steps = 10, True, False, 1e5
    d.random_seed(3)
    random.seed(3)
    agent = d.CategoricalDQNAgent(cfg)
    _load(agent.network, RAINBOW_SHAPES, 35)
    agent.target_network.load_state_dict(agent.network.state_dict())
    torch.manual_seed(5)
    return agent


def _run(agent, steps, upd_steps=()):
    traj = []
    for t in range(steps):
        agent.step()
        if t in upd_steps:
            torch.cuda.synchronize()
            traj.append(trajectory_digest(dict(agent.network.named_parameters())))
    torch.cuda.synchronize()
    return traj


def _final_state(agent):
    rp = agent.replay.replay
    params = {n: v.detach().cpu().clone() for n, v in agent.network.named_parameters()}
    tree = rp.tree.as_tensor().cpu().clone() if getattr(rp, "tree", None) is not None else None
    return params, tree, (float(rp.max_priority) if tree is not None else None)


def test_rainbow_agent_replays_captured_graphs(dra, monkeypatch):
    """The `rainbow` case of tests/test_gpu_rainbow_dueling.py, same configuration and bars, with both graphs captured; then
    the eager run (bit-identical parameters and tree) and a uniform-replay run (captures, stays finite).  Measured use of the
    2e-4 gate: 7.9e-6 over the run's updates (the module path: 6.1e-5)."""
    d = dra
    g = np.load(GOLDEN)
    steps = dict(HEAD_AGENT_CASES)["rainbow"]
    k = "rainbow_"
    upd_steps, upd_want = list(g[k + "update_steps"]), g[k + "update_digests"]
    agent = _rainbow_agent(d, monkeypatch)
    traj = _run(agent, steps, upd_steps)
    assert agent.actor._graphed_q.graph is not None, "the actor forward was not captured"
    assert agent._graphed.graph is not None, "the PER update was not captured"
    gate_atol = 2e-4
    errs = check_trajectory("noisy_rainbow_trajectory graphed", traj, upd_want, gate_atol=gate_atol)
    print("trajectory: max per-update abs error %.3g (gate_atol %.1e)" % (max(errs), gate_atol))
    rp = agent.replay.replay
    n = rp.size()
    assert agent.total_steps == int(g[k + "total_steps"])
    assert [rp.pos, n] == list(g[k + "pos_size"])
    frames, actions, rewards, masks = rp._ring.pointers()
    w = d.ops._wrap_device_pointer
    assert np.array_equal(w(actions, n, torch.int64).cpu().numpy(), g[k + "replay_action"])
    assert np.array_equal(w(rewards, n, torch.float64).cpu().numpy(), g[k + "replay_reward"])
    assert np.array_equal(w(masks, n, torch.int32).cpu().numpy(), g[k + "replay_mask"])
    np.testing.assert_allclose(rp.tree.as_tensor().cpu().numpy(), g[k + "tree"], rtol=3e-4, atol=1e-7)
    np.testing.assert_allclose(float(rp.max_priority), float(g[k + "max_priority"]), rtol=3e-4)
    assert np.array_equal(torch.randint(0, 1 << 30, (4,)).numpy(), g[k + "torch_rng_tail"])
    assert np.array_equal(np.random.randint(0, 1 << 30, size=4), g[k + "np_rng_tail"])
    assert np.array_equal([random.getrandbits(30) for _ in range(2)], g[k + "py_rng_tail"])
    for name, v in agent.network.named_parameters():
        check_gated(digest(v.detach().cpu().numpy())[2:], g[k + "final_" + name][2:], "final_" + name, gate_atol=gate_atol)
    graphed = _final_state(agent)
    agent.close()

    # eager: same kernels, same arguments
    agent = _rainbow_agent(d, monkeypatch, graph_update=False)
    _run(agent, steps)
    assert agent.actor._graphed_q.graph is None and agent._graphed.graph is None
    eager = _final_state(agent)
    agent.close()
    for name in graphed[0]:
        assert torch.equal(graphed[0][name], eager[0][name]), name
    assert torch.equal(graphed[1], eager[1]) and graphed[2] == eager[2]

    # uniform replay + noisy layers capture too
    agent = _rainbow_agent(d, monkeypatch, replay_cls=d.UniformReplay)
    _run(agent, steps)
    assert agent.actor._graphed_q.graph is not None and agent._graphed.graph is not None
    assert all(bool(torch.isfinite(v).all()) for v in agent.network.parameters())
    agent.close()


def test_eager_learn_commits_priorities_on_the_device(dra, monkeypatch):
    """commit_device form of the eager _learn against the host update_priorities form over the case's updates."""
    d = dra
    steps = dict(HEAD_AGENT_CASES)["rainbow"]
    finals = []
    for device_priorities in (True, False):
        agent = _rainbow_agent(d, monkeypatch, graph_update=False, device_priorities=device_priorities)
        _run(agent, steps)
        finals.append(_final_state(agent))
        agent.close()
    assert torch.equal(finals[0][1], finals[1][1]), "tree leaves differ"
    assert finals[0][2] == finals[1][2], "max_priority differs"
