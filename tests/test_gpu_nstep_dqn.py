"""n-step DQN on pixels over device-resident rollouts (agents._QRollout; csrc/nstep_q.hip, conv_v2.hip dra_rollout_conv1_qheads):
the Q-head role against the separate pieces, the max head and the loss + Q-head backward against fp64 numpy, the agent against
the reference's own NStepDQNAgent.step (tests/golden/nstep/n_step_dqn_pixel.npz, written by tests/golden/make_golden_nstep.py),
the device path against the host-emulator path and against itself without graph replay, and the zoo entry through run_steps."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fake_envs
from parity_log import record_parity

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nstep", "n_step_dqn_pixel.npz")
# the fixture's setup (tests/golden/make_golden_nstep.py)
N_ENVS, N_ACTIONS, ENV_SEED, DONE_PERIOD = 4, 4, 7, 6
PARAM_SEED, NP_SEED, STEPS, ROLLOUT = 29, 41, 4, 5
EPS, TARGET_FREQ = (0.6, 0.1, 300), 3


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


def _scale(*arrays):
    return max(1.0, max(float(np.abs(np.asarray(a, dtype=np.float64)).max()) for a in arrays))


def _fold_np(slabs, bias):
    """fc4's finish in float32, slab 0 first, then + bias, ReLU: the kernels' order."""
    v = slabs[0].copy()
    for s in range(1, slabs.shape[0]):
        v = (v + slabs[s]).astype(np.float32)
    v = (v + bias[None, :]).astype(np.float32)
    return np.maximum(v, np.float32(0))


# ---------------------------------------------------------------------------------------------------- 1. the Q-head role
@pytest.mark.parametrize("batch", [1, 4, 16, 32])
def test_conv1_qheads_equal_the_separate_pieces(dra, batch):
    d = dra
    from deeprl_amd._lib import lib, stream_ptr
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 + batch)
    n_act = 6
    frames = torch.randint(0, 256, (batch, 4, 84, 84), dtype=torch.uint8, generator=g).to(dev)
    w1 = (torch.randn(32, 4, 8, 8, generator=g) * 0.05)
    wt1 = w1.permute(1, 2, 3, 0).contiguous().to(dev)
    b1 = (torch.randn(32, generator=g) * 0.05).to(dev)
    slabs = (torch.randn(28, batch, 512, generator=g) * 0.05).to(dev)
    fold_bias = (torch.randn(512, generator=g) * 0.05).to(dev)
    wq = torch.randn(n_act, 512, generator=g) * 0.05
    bq = torch.randn(n_act, generator=g) * 0.05
    wq[3], bq[3] = wq[2], bq[2]                     # duplicate head rows: exact ties, the lower index (2) must win
    wq, bq = wq.to(dev), bq.to(dev)
    explore = (torch.rand(batch, generator=g) < 0.3).to(torch.uint8).to(dev)
    rand = torch.randint(0, n_act, (batch,), generator=g).to(dev)
    coef = 1.0 / 255.0
    y1 = torch.empty(batch, 32, 20, 20, device=dev)
    q = torch.empty(batch, n_act, device=dev)
    act = torch.empty(batch, dtype=torch.int64, device=dev)
    phi = torch.empty(batch, 512, device=dev)
    d.ops.rollout_conv1_qheads(frames, wt1, b1, y1, coef, slabs, fold_bias, wq, bq, explore, rand, out_q=q, out_action=act, out_phi=phi)
    # conv1: the plain launch
    y1_ref = d.ops.conv_fwd_koc(1, [frames], [wt1], [b1], act="relu", u8_coef=coef)[0]
    # phi: the A2C rollout launch's fold (same device function) and the fold in numpy float32
    y1_a2c = torch.empty_like(y1)
    wa, ba = torch.zeros(4, 512, device=dev), torch.zeros(4, device=dev)
    wv, bv = torch.zeros(1, 512, device=dev), torch.zeros(1, device=dev)
    uni = torch.full((batch,), 0.5, device=dev)
    o = [torch.empty(batch, dtype=torch.int64, device=dev)] + [torch.empty(batch, device=dev) for _ in range(3)]
    phi_a2c = torch.empty(batch, 512, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib.dra_rollout_conv1_heads_phi(p(frames), p(wt1), p(b1), p(y1_a2c), batch, coef, p(slabs), p(fold_bias), p(wa), p(ba), p(wv), p(bv),
                                    p(uni), 4, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(phi_a2c), stream_ptr())
    # the stand-alone form (the last row of a rollout) and the max mode
    q2, act2, phi2 = torch.empty_like(q), torch.empty_like(act), torch.empty_like(phi)
    qmax = torch.empty(batch, device=dev)
    d.ops.q_heads_fold28(slabs, fold_bias, wq, bq, explore, rand, out_q=q2, out_action=act2, out_phi=phi2, out_max=qmax)
    torch.cuda.synchronize()
    assert torch.equal(y1, y1_ref) and torch.equal(y1, y1_a2c)
    phi_np = _fold_np(slabs.cpu().numpy(), fold_bias.cpu().numpy())
    assert torch.equal(phi, phi_a2c) and np.array_equal(phi.cpu().numpy(), phi_np)
    q_np = phi_np.astype(np.float64) @ wq.cpu().numpy().astype(np.float64).T + bq.cpu().numpy().astype(np.float64)
    q_h = q.cpu().numpy()
    assert np.abs(q_h - q_np).max() <= 1e-6 * _scale(q_np)
    assert np.array_equal(q_h[:, 2], q_h[:, 3])
    want = np.where(explore.cpu().numpy().astype(bool), rand.cpu().numpy(), np.argmax(q_h, axis=-1))
    assert np.array_equal(act.cpu().numpy(), want)
    greedy = ~explore.cpu().numpy().astype(bool)
    assert not np.any(act.cpu().numpy()[greedy] == 3)           # a tie at the top never resolves to the higher duplicate
    assert torch.equal(q2, q) and torch.equal(act2, act) and torch.equal(phi2, phi)
    assert np.array_equal(qmax.cpu().numpy(), q_h.max(axis=-1))


# ---------------------------------------------------------------------------------------------------- 2. loss + backward
def test_nstep_loss_bwd_equals_fp64_numpy(dra):
    d = dra
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(5)
    t_len, n, n_act, gamma = 5, 7, 6, 0.99
    rows = t_len * n
    q = rs.standard_normal((t_len, n, n_act)).astype(np.float32)
    action = rs.randint(0, n_act, size=(t_len, n)).astype(np.int64)
    reward = np.sign(rs.standard_normal((t_len, n))).astype(np.float32)
    mask = (rs.rand(t_len, n) > 0.25).astype(np.float32)
    assert (mask == 0).any()
    boot = rs.standard_normal(n).astype(np.float32)
    phi = np.maximum(rs.standard_normal((rows, 512)), 0).astype(np.float32)
    w = (rs.standard_normal((n_act, 512)) * 0.05).astype(np.float32)
    T = lambda a: torch.from_numpy(a).to(dev)
    outs = [d.ops.nstep_q_loss_bwd(T(q), T(action), T(reward), T(mask), T(boot), gamma, T(phi), T(w)) for _ in range(2)]
    torch.cuda.synchronize()
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    out = {k: v.cpu().numpy() for k, v in outs[0].items()}
    # fp64 restatement of NStepDQN_agent.py:56-67
    ret = np.zeros((t_len, n))
    r_ = boot.astype(np.float64)
    for t in reversed(range(t_len)):
        r_ = reward[t] + gamma * mask[t] * r_
        ret[t] = r_
    qa = np.take_along_axis(q.astype(np.float64), action[..., None], axis=-1)[..., 0]
    diff = (qa - ret).reshape(-1)
    loss = 0.5 * np.mean(diff ** 2)
    dq = np.zeros((rows, n_act))
    dq[np.arange(rows), action.reshape(-1)] = diff / rows
    dw = dq.T @ phi.astype(np.float64)
    db = dq.sum(0)
    dphi = (dq @ w.astype(np.float64)) * (phi > 0)
    for name, have, want in (("ret", out["ret"], ret), ("loss", out["loss"][0], loss), ("dw", out["dw"], dw), ("db", out["db"], db),
                             ("dphi", out["dphi"], dphi)):
        err = float(np.abs(np.asarray(have, np.float64) - want).max())
        assert err <= 1e-5 * _scale(want), (name, err)
    assert np.all(out["dphi"][phi == 0] == 0)


# ---------------------------------------------------------------------------------------------------- agents
def _config(d, device_env=True, graph_update=True, n_envs=N_ENVS, seed=ENV_SEED, done_period=DONE_PERIOD, eps=EPS,
            target_freq=TARGET_FREQ, tag="ns"):
    from deeprl_amd.envs import SyntheticAtari
    cfg = d.Config()
    cfg.merge(dict(game="synthetic-atari", log_level=0, tag=tag, device_env=device_env, graph_update=graph_update))
    cfg.num_workers = n_envs

    def task_fn():
        task = d.Task(cfg.game, num_envs=n_envs, seed=1, synthetic_done_period=done_period)
        # the fixture's emulators (fake_envs.PixelVectorTask: seed + 1000 e)
        task.env.envs[:] = [SyntheticAtari(seed + 1000 * e, history=4, n_actions=N_ACTIONS, done_period=done_period)
                            for e in range(n_envs)]
        return task
    cfg.task_fn = task_fn
    cfg.eval_env = d.Task(cfg.game, seed=12)
    cfg.network_fn = lambda: d.VanillaNet(N_ACTIONS, d.NatureConvBody())
    cfg.optimizer_fn = lambda p: torch.optim.RMSprop(p, lr=1e-4, alpha=0.99, eps=1e-5)
    cfg.random_action_prob = d.LinearSchedule(*eps)
    cfg.state_normalizer, cfg.reward_normalizer = d.ImageNormalizer(), d.SignNormalizer()
    cfg.discount, cfg.target_network_update_freq, cfg.rollout_length, cfg.gradient_clip = 0.99, target_freq, ROLLOUT, 5
    return cfg


def _agent(d, monkeypatch, **kw):
    import deeprl_amd.agents as agents_mod
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Quiet())
    agent = d.NStepDQNAgent(_config(d, **kw))
    p_np = fake_envs.numpy_params(fake_envs.nature_vanilla_shapes(N_ACTIONS), PARAM_SEED)
    agent.network.load_state_dict({k: torch.from_numpy(v) for k, v in p_np.items()})
    d.ops.copy_f32(agent._target_flat.flat, agent._fused.flat.flat)
    torch.cuda.synchronize()
    return agent


def _params(agent):
    return {k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()}


def _rng_position():
    import zlib
    _, key, pos, _, _ = np.random.get_state()
    return np.asarray([pos, zlib.crc32(np.ascontiguousarray(key).tobytes())], dtype=np.int64)


def test_device_agent_matches_reference_fixture(dra, monkeypatch):
    """Actions and the np.random position exact at every step; q, returns and loss within 1e-5 of scale while the parameters are
    at most two updates away from the shared start, 1e-4 after that (the fp32 summation orders of the two implementations differ
    and RMSprop's first steps amplify sign-level gradient noise); parameters within 1e-5 of scale after every update.  The
    measured maxima go to the parity log."""
    d = dra
    g = np.load(FIXTURE)
    agent = _agent(d, monkeypatch)
    assert getattr(agent.task, "on_device", False), "synthetic Atari + VanillaNet(NatureConvBody) take the device path"
    np.random.seed(NP_SEED)
    errs = []
    for s in range(STEPS):
        agent.step()
        torch.cuda.synchronize()
        out = agent.last_rollout
        k = "s%d_" % s
        q, act, ret = out['q'].cpu().numpy(), out['action'].cpu().numpy(), out['ret'].cpu().numpy()
        assert np.array_equal(act, g[k + "action"]), s
        assert np.array_equal(_rng_position(), g[k + "rng"]), s
        assert agent.total_steps == int(g[k + "total_steps"])
        e = dict(q=float(np.abs(q - g[k + "q"]).max()) / _scale(g[k + "q"]),
                 ret=float(np.abs(ret - g[k + "ret"][..., 0]).max()) / _scale(g[k + "ret"]),
                 loss=abs(float(out['loss'].item()) - float(g[k + "loss"])) / max(1.0, abs(float(g[k + "loss"]))), params=0.0)
        for name, v in _params(agent).items():
            want = g[k + "param_" + name]
            have = v.reshape(-1)[::1009].astype(np.float64)
            e['params'] = max(e['params'], float(np.abs(have - want[2:]).max()) / _scale(want[2:]))
        errs.append(e)
        record_parity("n_step_dqn_pixel_device_vs_reference_step%d" % s, **e)
    for s, e in enumerate(errs):
        tol = 1e-5 if s <= 2 else 1e-4
        assert e['q'] <= tol and e['ret'] <= tol and e['loss'] <= tol, (s, errs)
        assert e['params'] <= 1e-5, (s, errs)
    assert agent._dev_graph.graph is not None and agent._dev_graph.calls == STEPS, "steps after the warm-up replay the graph"
    agent.close()


def _run(d, monkeypatch, steps, **kw):
    agent = _agent(d, monkeypatch, **kw)
    actions = []
    if not getattr(agent.task, "on_device", False):
        step = agent.task.step

        def logged(a):
            actions.append(np.asarray(a).copy())
            return step(a)
        agent.task.step = logged
    np.random.seed(NP_SEED)
    for _ in range(steps):
        agent.step()
        if agent.last_rollout is not None:
            actions.extend(list(agent.last_rollout['action'].cpu().numpy()))
    torch.cuda.synchronize()
    res = (_params(agent), np.stack(actions), agent.total_steps, _rng_position(), agent)
    agent.close()
    return res


def test_device_path_equals_host_path(dra, monkeypatch):
    """Same seeds with config.device_env = False (today's host path: module forwards, host epsilon-greedy, host emulators):
    identical actions, parameters within 1e-5 of scale after six agent steps."""
    d = dra
    dev = _run(d, monkeypatch, 6)
    host = _run(d, monkeypatch, 6, device_env=False)
    assert getattr(dev[4].task, "on_device", False) and not getattr(host[4].task, "on_device", False)
    assert np.array_equal(dev[1], host[1])
    assert dev[2] == host[2] and np.array_equal(dev[3], host[3])
    worst = 0.0
    for k in dev[0]:
        sc = _scale(host[0][k])
        e = float(np.abs(dev[0][k] - host[0][k]).max())
        assert e <= 1e-5 * sc, (k, e)
        worst = max(worst, e / sc)
    record_parity("n_step_dqn_pixel_device_vs_host", params=worst)


def test_graph_replay_equals_eager_device_path(dra, monkeypatch):
    d = dra
    a = _run(d, monkeypatch, 5)
    b = _run(d, monkeypatch, 5, graph_update=False)
    assert a[4]._dev_graph.graph is not None and b[4]._dev_graph.graph is None
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k


def test_launcher_runs_n_step_dqn_pixel_through_run_steps(dra):
    """examples.py::n_step_dqn_pixel (examples.py:427-447: 16 workers, rollouts of 5) through launch.run_entry + run_steps on
    device-resident synthetic Atari."""
    d = dra
    from deeprl_amd import launch
    import deeprl_amd.zoo as zoo
    mod = launch.load_examples(zoo.__file__, "zoo_examples_nstep")
    d.random_seed(3)
    agent = launch.run_entry(mod, "n_step_dqn_pixel", max_steps=1600, game="synthetic-atari", overrides=dict(save_interval=0))
    assert agent.total_steps == 1600
    assert getattr(agent.task, "on_device", False) and agent._dev_graph.graph is not None
    assert all(torch.isfinite(v).all() for v in agent.network.state_dict().values())
