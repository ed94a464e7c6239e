"""dqn_feature on the device (csrc/dqn_mlp.hip, deeprl_amd/dqn_mlp.py, DQNAgent with config.fused_dqn_feature): the two kernels
against the fp64 restatement (tests/dqn_feature_restatement.py, pinned to the reference's own run by
tests/test_dqn_feature_host.py) and against the reference's recorded steps, the agent's device path against the host loop (the
switch off: the parent commit's path) and the restatement, save / load, and the closed loop against the reference's learning
record."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from feature_kernel_harness import (      # noqa: F401  (dra: the fixture)
    GAME, GATE, GUARD, dra, _Rec, _fraction, _within, _bits, _guarded, _flat, _line_events, _launch_replay_act, _check_act_case)
from parity_log import record_parity

import dqn_feature_cases as K
import dqn_feature_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dqn_feature")
FIXTURE = os.path.join(GOLDEN, "dqn_feature_steps.npz")


def _net_struct(params, target, dev, hidden, gate, padded):
    from deeprl_amd import dqn_mlp
    flat, offs = _flat(R.KEYS, params, padded)
    tflat, _ = _flat(R.KEYS, target if target is not None else params, padded)
    flat, tflat = torch.from_numpy(flat).to(dev), torch.from_numpy(tflat).to(dev)
    net = dqn_mlp.Net()
    net.param, net.target = flat.data_ptr(), tflat.data_ptr()
    net.w1, net.b1, net.w2, net.b2, net.wq, net.bq = [offs[k] for k in R.KEYS]
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, hidden, GATE[gate]
    return net, flat, tflat, offs


# ------------------------------------------------------------------------------------------ the acting kernel
def _launch_act(dra, case, start):
    """One dra_dqn_mlp_act from the case's start -> dict of host arrays (guards included) and the return code."""
    from deeprl_amd._lib import lib
    hidden, gate, k_len, cap, slot0, horizon, padded = case[:7]
    net, flat, tflat, _ = _net_struct(start["params"], None, dra.Config.DEVICE, hidden, gate, padded)
    return _launch_replay_act(dra, lib.dra_dqn_mlp_act, net, (flat, tflat), K, start, k_len, cap, slot0, horizon)


@pytest.mark.parametrize("case", K.ACT_CASES, ids=K.act_id)
def test_act_kernel_matches_restatement(dra, case):
    """dra_dqn_mlp_act against the restatement: the ring's four arrays (the rows written AND the rows left alone), the actions
    (the host suite asserts a Q margin >= 1e-4 at every greedy transition of every case), the environment's arrays, the episode
    ring's rows and count and the step counter equal to the bit; q within 1e-5 of scale; the error word still 0; the guard
    elements behind every buffer and both parameter buffers untouched; a second launch from the same start gives the same
    bits everywhere."""
    hidden, gate, k_len, cap, slot0, horizon, padded = case[:7]
    want, env, start = K.restated_act(case)
    _check_act_case(lambda: _launch_act(dra, case, start), want, env, K, k_len, slot0,
                    "dqn_mlp acting kernel vs restatement %s (fraction of the bar)" % K.act_id(case))


# ------------------------------------------------------------------------------------------ the update kernel
def _launch_update(dra, params, target, ring, idx, hidden, gate, double_q, padded=False, launches=1):
    """dra_dqn_mlp_update on host arrays -> dict(q_target, td, loss, grads by name, gaps: the gradient buffer outside the six
    tensors, err, rc) per launch."""
    from deeprl_amd import dqn_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    net, flat, tflat, offs = _net_struct(params, target, dev, hidden, gate, padded)
    cap, b = ring["actions"].shape[0], len(idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frames, actions, rewards, masks, idx_t = t(ring["frames"]), t(ring["actions"]), t(ring["rewards"]), t(ring["masks"]), t(np.asarray(idx, dtype=np.int64))
    outs = []
    for _ in range(launches):
        grad_full, grad = _guarded((flat.numel(),), torch.float32, dev, float("nan"))
        (qt_full, qt), (td_full, td), (loss_full, loss) = (_guarded((n,), torch.float32, dev, float("nan")) for n in (b, b, 1))
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        io = dqn_mlp.UpdateIO()
        io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = frames.data_ptr(), actions.data_ptr(), rewards.data_ptr(), masks.data_ptr()
        io.idx, io.grad, io.out_q_target, io.out_td, io.out_loss = idx_t.data_ptr(), grad.data_ptr(), qt.data_ptr(), td.data_ptr(), loss.data_ptr()
        io.err, io.capacity, io.discount, io.batch, io.double_q = err.data_ptr(), cap, K.DISCOUNT, b, int(double_q)
        before = flat.cpu().numpy().copy(), tflat.cpu().numpy().copy()
        rc = lib.dra_dqn_mlp_update.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(flat.cpu().numpy()), _bits(before[0])) and np.array_equal(_bits(tflat.cpu().numpy()), _bits(before[1]))
        g = grad_full.cpu().numpy()
        covered = np.zeros(g.size, dtype=bool)
        grads = {}
        for k in R.KEYS:
            n = int(np.asarray(params[k]).size)
            grads[k] = g[offs[k]:offs[k] + n].reshape(np.asarray(params[k]).shape)
            covered[offs[k]:offs[k] + n] = True
        for full_t, n in ((qt_full, b), (td_full, b), (loss_full, 1)):
            assert torch.isnan(full_t[n:]).all()
        outs.append(dict(rc=rc, q_target=qt.cpu().numpy(), td=td.cpu().numpy(), loss=float(loss.item()), grads=grads,
                         gaps=g[~covered], err=int(err.item())))
    return outs


def _compare_update(got, want, what):
    worst = {}
    worst["q_target"] = _within(got["q_target"], want["q_target"], what + " q_target")
    worst["td"] = _within(got["td"], want["td"], what + " td")
    worst["loss"] = _within(np.asarray([got["loss"]]), np.asarray([want["loss"]]), what + " loss")
    worst["grads"] = max(_within(got["grads"][k], want["grads"][k], what + " d" + k) for k in R.KEYS)
    return worst


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_kernel_matches_restatement(dra, case):
    """dra_dqn_mlp_update against the fp64 restatement on the case's ring, indices and parameters (the target's from another
    seed): q_target, td, the loss and the six gradients within 1e-5 of scale (the module path's fp32 autograd on the same case is
    recorded next to it as the yardstick); every element of the six tensors written and nothing between or behind them (the
    parameters lie behind a leading gap with NaN between them in the cases of 65 rows); the error word 0; both parameter
    buffers unchanged; two launches give the same bits."""
    hidden, gate, batch, double_q, kind = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    padded = batch == 65
    a, b = _launch_update(dra, u["params"], u["target"], rg["ring"], u["idx"], hidden, gate, double_q, padded, launches=2)
    assert a["rc"] == 0 and a["err"] == 0
    worst = _compare_update(a, u, K.update_id(case))
    assert np.isnan(a["gaps"]).all() and a["gaps"].size == GUARD + ((3 + sum((-np.asarray(u["params"][k]).size) % 4 + 1 for k in R.KEYS)) if padded else 0)
    assert all(np.isfinite(a["grads"][k]).all() for k in R.KEYS)
    if kind == "action0":
        assert not a["grads"]["fc_head.weight"][1].any() and a["grads"]["fc_head.bias"][1] == 0
    yard = R.loss_and_grads(u["params"], u["target"], u["batch"], K.DISCOUNT, double_q, gate, dtype=torch.float32)
    yard_f = max(_fraction(yard["grads"][k], u["grads"][k], "fp32 autograd d" + k) for k in R.KEYS)
    record_parity("dqn_mlp update kernel vs restatement %s (fraction of the bar)" % K.update_id(case), **worst)
    record_parity("module path fp32 autograd vs restatement %s (fraction of the bar)" % K.update_id(case), grads=yard_f)
    for k in ("q_target", "td"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["loss"] == b["loss"] and all(np.array_equal(_bits(a["grads"][k]), _bits(b["grads"][k])) for k in R.KEYS)


def test_update_clamps_and_counts_indices_outside_the_ring(dra):
    """Staged indices outside [0, capacity - 2] are clamped into it and counted in the error word: the launch computes what it
    computes on the clamped indices, bit for bit, and reads nothing outside the ring."""
    case = (32, "relu", 10, False, "partial")
    u, rg = K.restated_update(case), K.make_ring("partial")
    cap = K.RINGS["partial"]["capacity"]
    bad = u["idx"].copy()
    bad[4], bad[5], bad[6] = -3, cap - 1, cap + 7
    clamped = np.clip(bad, 0, cap - 2)
    ring = {k: v.copy() for k, v in rg["ring"].items()}
    ring["frames"][260:], ring["rewards"][260:], ring["masks"][260:], ring["actions"][260:] = 0.25, 1.0, 1, 0     # (finite everywhere)
    got, = _launch_update(dra, u["params"], u["target"], ring, bad, 32, "relu", False)
    want, = _launch_update(dra, u["params"], u["target"], ring, clamped, 32, "relu", False)
    assert got["rc"] == want["rc"] == 0 and got["err"] == 3 and want["err"] == 0
    assert np.array_equal(_bits(got["q_target"]), _bits(want["q_target"])) and got["loss"] == want["loss"]
    assert all(np.array_equal(_bits(got["grads"][k]), _bits(want["grads"][k])) for k in R.KEYS)


@pytest.mark.parametrize("tag", [t[0] for t in K.FIXTURE_TAGS])
def test_update_kernel_matches_reference_steps(dra, tag):
    """The reference's recorded run (tests/golden/dqn_feature/): from the recorded initial parameters, every update of the run --
    dra_dqn_mlp_update on the recorded ring rows and indices, then the fused clip + RMSprop step, the target copied where the
    reference copies it -- lands on the reference's parameters after every step within rtol 2e-5 / atol 2e-6; the losses too."""
    from deeprl_amd import dqn_mlp, ops
    from deeprl_amd._lib import lib, stream_ptr
    from deeprl_amd.optim import FlatParams, FusedOptimizer
    d, dev = dra, dra.Config.DEVICE
    z = np.load(FIXTURE)
    _, _, _, double_q, freq, hidden = next(t for t in K.FIXTURE_TAGS if t[0] == tag)
    f = K.FIXTURE
    net, tgt = d.VanillaNet(2, d.FCBody(4, (hidden, hidden))), d.VanillaNet(2, d.FCBody(4, (hidden, hidden)))
    fused = FusedOptimizer.adopt(torch.optim.RMSprop(net.parameters(), K.LR))
    tflat = FlatParams(list(tgt.parameters()))
    with torch.no_grad():
        for k, p in net.state_dict().items():
            p.copy_(torch.from_numpy(z["%s_init_%s" % (tag, k)]))
        for k, p in tgt.state_dict().items():
            p.copy_(torch.from_numpy(z["%s_target0_%s" % (tag, k)]))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frames, actions, rewards, masks = (t(z["%s_ring_%s" % (tag, k)]) for k in ("frames", "actions", "rewards", "masks"))
    qt, td, loss, err = (torch.zeros(n, dtype=dt, device=dev) for n, dt in ((f["batch"], torch.float32), (f["batch"], torch.float32),
                                                                            (1, torch.float32), (1, torch.int32)))
    n = dqn_mlp.Net()
    n.param, n.target = fused.flat.flat.data_ptr(), tflat.flat.data_ptr()
    for field, p in dqn_mlp._fields(net):
        setattr(n, field, fused.flat.offset_of(p))
    n.state_dim, n.n_actions, n.hidden, n.gate = 4, 2, hidden, 1
    worst, losses = 0.0, []
    for s in range(f["steps"]):
        idx = z[tag + "_indices"][s]
        if idx[0] >= 0:
            assert idx.max() + 1 < f["k"] * (s + 1)          # (rows the run had written by then)
            idx_t = t(idx)
            io = dqn_mlp.UpdateIO()
            io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = frames.data_ptr(), actions.data_ptr(), rewards.data_ptr(), masks.data_ptr()
            io.idx, io.grad, io.out_q_target, io.out_td, io.out_loss = idx_t.data_ptr(), fused.flat.grad.data_ptr(), qt.data_ptr(), td.data_ptr(), loss.data_ptr()
            io.err, io.capacity, io.discount, io.batch, io.double_q = err.data_ptr(), f["capacity"], K.DISCOUNT, f["batch"], int(double_q)
            lib.dra_dqn_mlp_update(ctypes.byref(n), ctypes.byref(io), stream_ptr())
            fused.step(K.GRADIENT_CLIP)
            losses.append(float(loss.item()))
        if f["k"] * (s + 1) / f["k"] % freq == 0:
            ops.copy_f32(tflat.flat, fused.flat.flat)
        torch.cuda.synchronize()
        for k, p in net.state_dict().items():
            want = z["%s_params_%s" % (tag, k)][s]
            got = p.detach().cpu().numpy()
            worst = max(worst, float(np.max(np.abs(got - want) / (2e-6 + 2e-5 * np.abs(want)))))
            np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6, err_msg="%s after step %d" % (k, s))
    assert int(err.item()) == 0 and len(losses) == len(z[tag + "_losses"]) == f["steps"] - 2
    np.testing.assert_allclose(losses, z[tag + "_losses"], rtol=2e-5, atol=2e-6)
    for k, p in tgt.state_dict().items():
        np.testing.assert_allclose(p.detach().cpu().numpy(), z["%s_target_%s" % (tag, k)], rtol=2e-5, atol=2e-6, err_msg=k)
    record_parity("dqn_feature update kernel vs reference steps %s (fraction of the bar)" % tag, params=worst)


# ------------------------------------------------------------------------------------------ the agent
A = K.AGENT


def _config(d, feature, graph=True, exploration_steps=None, **extra):
    from deeprl_amd import zoo
    from deeprl_amd.replay import ReplayWrapper, UniformReplay
    kw = dict(fused_dqn_feature=True) if feature else {}
    c = zoo.config("dqn_feature", game=GAME, tag="dqn_feat%d%d" % (feature, graph), graph_update=graph,
                   overrides=dict(sgd_update_frequency=A["k"], batch_size=A["batch"], target_network_update_freq=A["target_freq"],
                                  exploration_steps=A["exploration_steps"] if exploration_steps is None else exploration_steps,
                                  double_q=A["double_q"], **extra), **kw)
    c.task_fn = lambda: d.Task(c.game, seed=A["task_seed"], synthetic_done_period=A["horizon"])
    rk = dict(memory_size=A["capacity"], batch_size=A["batch"], n_step=1, discount=A["discount"], history_length=1)
    c.replay_fn = lambda: ReplayWrapper(UniformReplay, rk, False)
    c.random_action_prob = d.LinearSchedule(*A["eps"])
    c.log_interval = 10 ** 9
    return c


def _make_agent(d, monkeypatch, feature, graph=True, **kw):
    import deeprl_amd.agents as agents_mod
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    d.random_seed(9)
    torch.manual_seed(9)
    agent = d.DQNAgent(_config(d, feature, graph, **kw))
    # the case's parameters (numpy-seeded: the same on every machine), copied into the optimiser's flat buffer through the views;
    # the target starts as their copy (DQN_agent.py:57)
    init = K.restated_agent_run()["init"]
    with torch.no_grad():
        for k, p in agent.network.state_dict().items():
            p.copy_(torch.from_numpy(init[k]))
    agent.sync_target()
    np.random.seed(A["np_seed"])        # the exploration and index stream starts here on both paths
    return agent, rec


def _ring_arrays(agent):
    torch.cuda.synchronize()
    ring = agent._inner_replay()._ring
    frames, actions, rewards, masks = ring.arrays()
    return dict(frames=frames.view(torch.float64).cpu().numpy().reshape(-1, 4), actions=actions.view(torch.int64).cpu().numpy(),
                rewards=rewards.cpu().numpy(), masks=masks.cpu().numpy())


def _snapshot(agent, rec):
    torch.cuda.synchronize()
    return dict(params={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
                target={k: v.detach().cpu().numpy().copy() for k, v in agent.target_network.state_dict().items()},
                total=agent.total_steps, actor_total=agent.actor._total_steps, ring=_ring_arrays(agent),
                pos=agent._inner_replay().pos, size=agent._inner_replay().size(),
                lines=[ln for ln in rec.lines if 'episodic_return_train' in ln],
                epsilon=agent.config.random_action_prob.current, rng=np.random.randint(0, 1 << 30, size=3))


def _run(d, monkeypatch, feature, graph=True, steps=A["steps"], **kw):
    from deeprl_amd.device_env import DeviceCartPoleVec
    agent, rec = _make_agent(d, monkeypatch, feature, graph, **kw)
    assert isinstance(agent.actor._task, DeviceCartPoleVec) == bool(feature) and (agent._feature is not None) == bool(feature)
    actions, indices = [], []
    if not feature:
        raw = agent.actor._task.step

        def step(a):
            actions.append(int(np.asarray(a).reshape(-1)[0]))
            return raw(a)
        agent.actor._task.step = step
    for _ in range(steps):
        agent.step()
        if feature:
            actions += list(agent._feature.out_action.cpu().numpy())
            indices.append(agent._feature.last_draws[3])
    events = agent.episodes()
    out = _snapshot(agent, rec)
    out.update(actions=np.asarray(actions, dtype=np.int64).reshape(steps, A["k"]), events=events, indices=indices,
               graphed={k: r.graph is not None for k, r in agent._feature.regions.items()} if feature else {},
               launches=agent._feature.launches if feature else 0)
    agent.close()
    return out


@pytest.fixture(scope="module")
def device_run(dra):
    """Eight steps of the device path with graph replay: shared by the tests below, left unchanged."""
    mp = pytest.MonkeyPatch()
    try:
        return _run(dra, mp, True, True)
    finally:
        mp.undo()


def _params_within(a, others, bar=2e-4):
    worst = 0.0
    for other in others:
        for k in a:
            scale = max(np.abs(other[k]).max(), 1e-2)
            worst = max(worst, float(np.max(np.abs(a[k] - other[k])) / (bar * scale)))
    return worst


def test_agent_device_path_equals_host_loop_and_restatement(dra, monkeypatch, device_run):
    """DQNAgent on the dqn_feature configuration (one cart-pole with episodes of at most 5 steps, 4 transitions per step,
    exploration_steps 6 crossed inside the second step, minibatches of 10 from a replay of 24 slots that wraps, a target copy every
    3 steps) with config.fused_dqn_feature -- eager steps, then graph replays -- against the same agent with the switch off (the
    parent commit's path) and against the fp64 restatement, over 8 agent steps: actions, the replay ring's four arrays, its
    cursor, the sampled indices, total_steps, the episodic-return log lines (late on the device path, otherwise the same), the
    np.random tail and the schedule's position equal; online and target parameters within 2e-4 of each tensor's largest
    magnitude (floor 1e-2), the family's bar."""
    from deeprl_amd.dqn_mlp import Step
    a, b = device_run, _run(dra, monkeypatch, False)
    want = K.restated_agent_run()
    steps = A["steps"]
    assert a['graphed'] == dict(act=False, learn=True) and a['launches'] == 1 + Step.WARMUP + 1      # eager steps and the capture pass
    assert a['total'] == b['total'] == want['total'] == a['actor_total'] == b['actor_total'] == steps * A["k"]
    assert np.array_equal(a['actions'], b['actions']) and np.array_equal(a['actions'], want['actions'])
    for k in ("frames", "rewards"):
        assert np.array_equal(_bits(a['ring'][k]), _bits(b['ring'][k])) and np.array_equal(_bits(a['ring'][k]), _bits(want['ring'][k])), k
    for k in ("actions", "masks"):
        assert np.array_equal(a['ring'][k], b['ring'][k]) and np.array_equal(a['ring'][k], want['ring'][k]), k
    assert (a['pos'], a['size']) == (b['pos'], b['size']) == (want['pos'], want['size'])
    assert all((i is None and j is None) or np.array_equal(i, j) for i, j in zip(a['indices'], want['indices']))
    assert a['lines'] == b['lines'] and len(a['lines']) >= 4
    assert a['events'] == _line_events(b['lines']) and b['events'] == []
    assert [(s, r) for s, r in a['events']] == [(s, r) for s, _, r in want['events']]
    assert np.array_equal(a['rng'], b['rng']) and np.array_equal(a['rng'], want['rng_tail'])
    assert a['epsilon'] == b['epsilon'] == want['epsilon']
    worst = _params_within(a['params'], (b['params'], want['params'][-1]))
    worst = max(worst, _params_within(a['target'], (b['target'], want['target'])))
    print("device vs host loop and restatement: worst fraction of the bar %.3f" % worst)
    record_parity("dqn_feature agent device vs host loop and restatement (fraction of the bar)", params=worst)
    assert worst <= 1.0


def test_module_update_form_matches_the_fused_one(dra, monkeypatch, device_run):
    """config.fused_dqn_update False (device acting and ring, ring.gather and the modules on the same indices) over the same
    eight steps: the same actions, ring, indices and events; parameters within the agent test's bar."""
    b = _run(dra, monkeypatch, True, fused_dqn_update=False)
    a = device_run
    assert b['graphed'] == dict(act=False, learn=True) and np.array_equal(a['actions'], b['actions'])
    assert np.array_equal(_bits(a['ring']['frames']), _bits(b['ring']['frames'])) and np.array_equal(a['ring']['masks'], b['ring']['masks'])
    assert a['events'] == b['events'] and a['lines'] == b['lines'] and a['total'] == b['total'] and np.array_equal(a['rng'], b['rng'])
    worst = _params_within(a['params'], (b['params'],))
    record_parity("dqn_feature fused update vs module update on the device (fraction of the bar)", params=worst)
    assert worst <= 1.0


def test_graph_replay_equals_eager(dra, monkeypatch):
    """exploration_steps 14: four acting-only steps (two eager, the capture, a replay), then six learning steps (two eager, the
    capture, replays) with target copies between replays.  config.graph_update False keeps every step eager: parameters, ring,
    actions and events are equal to the bit."""
    a = _run(dra, monkeypatch, True, graph=True, steps=10, exploration_steps=14)
    b = _run(dra, monkeypatch, True, graph=False, steps=10, exploration_steps=14)
    assert a['graphed'] == dict(act=True, learn=True) and b['graphed'] == dict(act=False, learn=False)
    assert a['launches'] == 3 + 3 and b['launches'] == 10
    assert a['total'] == b['total'] and a['lines'] == b['lines'] and a['events'] == b['events'] and np.array_equal(a['rng'], b['rng'])
    assert np.array_equal(a['actions'], b['actions'])
    for k in a['ring']:
        assert np.array_equal(_bits(a['ring'][k]), _bits(b['ring'][k])), k
    for k in a['params']:
        assert np.array_equal(_bits(a['params'][k]), _bits(b['params'][k])) and np.array_equal(_bits(a['target'][k]), _bits(b['target'][k])), k


def test_save_load_continues_the_run(dra, monkeypatch, device_run, tmp_path):
    """4 steps, save() + the replay's save_full(), a fresh agent, load() + load_full(), 4 more steps == 8 uninterrupted steps, bit
    for bit.  save() writes what the reference's checkpoint holds plus `<file>.envs`; the optimiser's running averages, the
    target network, the step counters, the schedule and the np.random state are no part of a checkpoint, so the test carries
    them over by hand."""
    first, rec = _make_agent(dra, monkeypatch, True)
    for _ in range(4):
        first.step()
    name = str(tmp_path / "ckpt")
    first.save(name)
    first._inner_replay().save_full(name)
    assert os.path.isfile(name + ".envs") and os.path.isfile(name + ".model") and os.path.isfile(name + ".replay")
    rng = np.random.get_state()
    second, rec2 = _make_agent(dra, monkeypatch, True)
    assert int(second._feature.step_dev.item()) == 0
    second.load(name)
    second._inner_replay().load_full(name)
    assert int(second._feature.step_dev.item()) == 4 * A["k"] == second._feature.episodes.stamp
    for key in ("env_state", "env_counter", "ep_steps", "ep_return"):
        assert torch.equal(getattr(second.actor._task, key), getattr(first.actor._task, key)), key
    second._fused.state1.copy_(first._fused.state1)
    second._fused.state2.copy_(first._fused.state2)
    second._target_flat.flat.copy_(first._target_flat.flat)
    second._fused.steps, second.total_steps, second.actor._total_steps = first._fused.steps, first.total_steps, first.actor._total_steps
    second.config.random_action_prob.current = first.config.random_action_prob.current
    np.random.set_state(rng)
    for _ in range(4):
        second.step()
    second.drain_episodes()
    got = _snapshot(second, rec2)
    first.close()
    second.close()
    assert got['total'] == device_run['total'] and got['epsilon'] == device_run['epsilon'] and got['pos'] == device_run['pos']
    assert [ln for ln in rec.lines if 'episodic_return_train' in ln] + got['lines'] == device_run['lines']
    assert np.array_equal(got['rng'], device_run['rng'])
    for k in got['ring']:
        assert np.array_equal(_bits(got['ring'][k]), _bits(device_run['ring'][k])), k
    for k in got['params']:
        assert np.array_equal(_bits(got['params'][k]), _bits(device_run['params'][k])), k


def test_default_config_stays_on_the_host(dra, monkeypatch):
    """A default-Config DQNAgent on the cart-pole Task keeps envs.Task and logs nothing (the path is opt-in); switching on with a
    network the kernels do not walk (DuelingNet) keeps the host loop and logs a warning naming the reason."""
    import deeprl_amd.agents as agents_mod
    d = dra
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    agent = d.DQNAgent(_config(d, False))
    assert agent._feature is None and type(agent.actor._task) is d.Task and rec.warnings == []
    assert agent.episodes() == [] and agent.drain_episodes() == []
    agent.step()
    assert agent.total_steps == A["k"] and agent.actor._task.env.envs[0].c == A["k"]
    agent.close()
    c = _config(d, True)
    c.network_fn = lambda: d.DuelingNet(c.action_dim, d.FCBody(c.state_dim))
    agent = d.DQNAgent(c)
    assert agent._feature is None and type(agent.actor._task) is d.Task
    assert len(rec.warnings) == 1 and "the network is not VanillaNet" in rec.warnings[0]
    agent.step()
    assert agent.total_steps == A["k"]
    agent.close()


def test_closed_loop_learns(dra, monkeypatch):
    """The dqn_feature entry itself (zoo: hidden 64, replay of 10^4, exploration_steps 1000, epsilon 1.0 -> 0.1 over 10^4, a target
    copy every 200 updates) with config.fused_dqn_feature for the number of environment steps at which the REFERENCE's own
    median over five seeds reaches 2 x the bar (tests/golden/dqn_feature/learning_reference.json: n_learn): the median over three
    seeds of the mean return of the last 100 training episodes reaches the bar, 2 x the random policy's mean (44.2)."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    from deeprl_amd.device_env import DeviceCartPoleVec
    d = dra
    ref = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))
    bar, n_learn = ref["bar"], ref["n_learn"]
    assert n_learn is not None and abs(bar - 44.2) < 0.1
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    means = []
    for seed in K.LEARN_SEEDS:
        d.random_seed(seed)
        torch.manual_seed(seed)
        c = zoo.config("dqn_feature", game=GAME, tag="dqn_feat_learn%d" % seed, fused_dqn_feature=True)
        c.task_fn = lambda seed=seed, c=c: d.Task(c.game, seed=seed)
        c.log_interval = 10 ** 9
        agent = d.DQNAgent(c)
        assert isinstance(agent.actor._task, DeviceCartPoleVec)
        returns = []
        while agent.total_steps < n_learn:
            agent.step()
            if agent.total_steps % 4096 == 0:
                returns += [r for _, r in agent.episodes()]
        returns += [r for _, r in agent.episodes()]
        agent.close()
        means.append(float(np.mean(returns[-K.LAST_EPISODES:])))
        print("seed %d: %d episodes, last-%d mean %.2f" % (seed, len(returns), K.LAST_EPISODES, means[-1]))
    median = float(np.median(means))
    record_parity("dqn_feature closed loop: last-100 mean returns per seed, median, bar", median=median, bar=bar,
                  **{"seed%d" % s: m for s, m in zip(K.LEARN_SEEDS, means)})
    assert median >= bar, (means, bar)
