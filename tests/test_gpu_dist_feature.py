"""categorical_dqn_feature / quantile_regression_dqn_feature on the device (csrc/dist_mlp.hip, deeprl_amd/dist_mlp.py, the two agents
with config.fused_dist_feature): the two kernels against the fp64 restatement (tests/dist_feature_restatement.py, pinned to the
reference's own runs by tests/test_dist_feature_host.py) and against the reference's recorded steps, the agents' device path
against the host loop (the switch off: the parent commit's path) and the restatement, save / load, and the closed loop against the
reference's learning record.  The agent tests set config.fused_dist_update True, so that the update kernel is what they run for both
head kinds (unset, the categorical head takes the module form: dist_mlp.Kind.fused_update); one test compares the two forms.

The bars.  Every tensor: the family's 1e-5 of its largest magnitude (floor 1.0).  Next to every update case the MODULE path's own
fp32 error on the same case is recorded (the modules, ops.c51_loss / ops.qr_loss and autograd against the same restatement): the
yardstick.  The quantile kernel is held to 1.0 of the bar.  For the categorical kernel's log / exp chain the bar of a quantity is
max(1.0, 2 x the module path's measured fraction of the bar for that quantity on that case) and no more."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from feature_kernel_harness import (      # noqa: F401  (dra: the fixture)
    GAME, GATE, GUARD, dra, _Rec, _fraction, _bits, _guarded, _flat, _line_events, _launch_replay_act, _check_act_case,
    _check_bad_slots)
from parity_log import record_parity

import dist_feature_cases as K
import dist_feature_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dist_feature")
FIXTURE = os.path.join(GOLDEN, "steps.npz")
ENTRY = {"c51": "categorical_dqn_feature", "qr": "quantile_regression_dqn_feature"}


def _pad_floats(params, head):
    return 3 + sum((-np.asarray(params[k]).size) % 4 + 1 for k in R.keys(head))


def _net_struct(params, target, dev, spec, hidden, gate, padded):
    from deeprl_amd import dist_mlp
    head = spec["head"]
    flat, offs = _flat(R.keys(head), params, padded)
    tflat, _ = _flat(R.keys(head), target if target is not None else params, padded)
    flat, tflat = torch.from_numpy(flat).to(dev), torch.from_numpy(tflat).to(dev)
    net = dist_mlp.Net()
    net.param, net.target = flat.data_ptr(), tflat.data_ptr()
    net.w1, net.b1, net.w2, net.b2, net.wq, net.bq = [offs[k] for k in R.keys(head)]
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, hidden, GATE[gate]
    net.head, net.n_atoms, net.v_min, net.v_max = K.HEAD_CODE[head], spec["n"], spec["v_min"], spec["v_max"]
    return net, flat, tflat, offs


# ------------------------------------------------------------------------------------------ the acting kernel
def _launch_act(dra, start, hidden, gate, k_len, cap, slot0, horizon, padded):
    """One dra_dist_mlp_act from a case's start -> dict of host arrays (guards included) and the return code."""
    from deeprl_amd._lib import lib
    net, flat, tflat, _ = _net_struct(start["params"], None, dra.Config.DEVICE, start["spec"], hidden, gate, padded)
    return _launch_replay_act(dra, lib.dra_dist_mlp_act, net, (flat, tflat), K, start, k_len, cap, slot0, horizon)


def _launch_act_case(dra, case, start, slot0=None):
    head, hidden, gate, n, k_len, cap, s0, horizon, padded, _ = case
    return _launch_act(dra, start, hidden, gate, k_len, cap, s0 if slot0 is None else slot0, horizon, padded)


@pytest.mark.parametrize("case", K.ACT_CASES, ids=K.act_id)
def test_act_kernel_matches_restatement(dra, case):
    """dra_dist_mlp_act against the restatement: the ring's four arrays (the rows written AND the rows left alone), the actions
    (the host suite asserts an action-value margin >= 1e-4 at every greedy transition of every case), the environment's arrays,
    the episode ring's rows and count and the step counter equal to the bit; q within 1e-5 of scale; the error word still 0; the
    guard elements behind every buffer and both parameter buffers untouched; a second launch from the same start gives the same
    bits everywhere."""
    head, hidden, gate, n, k_len, cap, slot0, horizon, padded, _ = case
    want, env, start = K.restated_act(case)
    _check_act_case(lambda: _launch_act_case(dra, case, start), want, env, K, k_len, slot0,
                    "dist_mlp acting kernel vs restatement %s (fraction of the bar)" % K.act_id(case))


@pytest.mark.parametrize("head", K.HEADS)
def test_act_counts_a_first_slot_outside_the_ring(dra, head):
    """A staged first slot outside [0, capacity) is taken as 0 and counted in the error word: the launch equals the launch from
    slot 0 bit for bit, and nothing outside the ring is written."""
    case = next(c for c in K.ACT_CASES if c[0] == head and c[4] == 4 and c[3] == 20)
    _, _, start = K.restated_act(case)
    _check_bad_slots(lambda slot0: _launch_act_case(dra, case, start, slot0=slot0), case[5])


# ------------------------------------------------------------------------------------------ the update kernel
def _launch_update(dra, params, target, ring, idx, spec, hidden, gate, double_q, discount, padded=False, launches=1):
    """dra_dist_mlp_update on host arrays -> per launch dict(loss, loss_vec, q_next, target, grads by name, gaps: the gradient
    buffer outside the six tensors, err, rc)."""
    from deeprl_amd import dist_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    head, n = spec["head"], spec["n"]
    net, flat, tflat, offs = _net_struct(params, target, dev, spec, hidden, gate, padded)
    cap, b = ring["actions"].shape[0], len(idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frames, actions, rewards, masks = t(ring["frames"]), t(ring["actions"]), t(ring["rewards"]), t(ring["masks"])
    idx_t = t(np.asarray(idx, dtype=np.int64)) if b else torch.zeros(1, dtype=torch.int64, device=dev)
    n_vec = max(b if head == "c51" else n, 1)
    shapes = dict(loss=(1,), loss_vec=(n_vec,), q_next=(max(b, 1), 2), target=(max(b, 1), max(n, 1)))
    outs = []
    for _ in range(launches):
        grad_full, grad = _guarded((flat.numel(),), torch.float32, dev, float("nan"))
        bufs = {k: _guarded(s, torch.float32, dev, float("nan")) for k, s in shapes.items()}
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        io = dist_mlp.UpdateIO()
        io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = frames.data_ptr(), actions.data_ptr(), rewards.data_ptr(), masks.data_ptr()
        io.idx, io.grad = idx_t.data_ptr(), grad.data_ptr()
        io.out_loss, io.out_loss_vec = bufs["loss"][1].data_ptr(), bufs["loss_vec"][1].data_ptr()
        io.out_q_next, io.out_target = bufs["q_next"][1].data_ptr(), bufs["target"][1].data_ptr()
        io.err, io.capacity, io.discount, io.batch, io.double_q = err.data_ptr(), cap, discount, b, int(double_q)
        before = flat.cpu().numpy().copy(), tflat.cpu().numpy().copy()
        rc = lib.dra_dist_mlp_update.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(flat.cpu().numpy()), _bits(before[0])) and np.array_equal(_bits(tflat.cpu().numpy()), _bits(before[1]))
        g = grad_full.cpu().numpy()
        covered = np.zeros(g.size, dtype=bool)
        grads = {}
        for k in R.keys(head):
            size = int(np.asarray(params[k]).size)
            grads[k] = g[offs[k]:offs[k] + size].reshape(np.asarray(params[k]).shape)
            covered[offs[k]:offs[k] + size] = True
        for k, s in shapes.items():
            assert torch.isnan(bufs[k][0][int(np.prod(s)):]).all(), k
        outs.append(dict(rc=rc, loss=float(bufs["loss"][1].item()), loss_vec=bufs["loss_vec"][1].cpu().numpy(),
                         q_next=bufs["q_next"][1].cpu().numpy(), target=bufs["target"][1].cpu().numpy(), grads=grads,
                         gaps=g[~covered], err=int(err.item())))
    return outs


def _module_path(dra, u, case):
    """The module path on the same case: the package's own networks, ops.c51_loss / ops.qr_loss and autograd on the device ->
    dict(loss, loss_vec, q_next, grads)."""
    from deeprl_amd import ops
    d, dev = dra, dra.Config.DEVICE
    head, n, hidden, gate, batch, double_q, kind, discount, _ = case
    spec = u["spec"]
    g = torch.relu if gate == "relu" else torch.tanh
    mk = lambda: (d.CategoricalNet if head == "c51" else d.QuantileNet)(2, n, d.FCBody(4, (hidden, hidden), gate=g))
    net, tgt = mk(), mk()
    with torch.no_grad():
        for k, p in net.state_dict().items():
            p.copy_(torch.from_numpy(u["params"][k]))
        for k, p in tgt.state_dict().items():
            p.copy_(torch.from_numpy(u["target_params"][k]))
    mb = u["batch"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    state, nxt, action, reward, mask = t(mb["state"]), t(mb["next_state"]), t(mb["action"]), t(mb["reward"]), t(mb["mask"])
    key = "logits" if head == "c51" else "quantile"
    with torch.no_grad():
        pred_t = tgt(nxt)
        out_t = pred_t[key]
        out_o = net(nxt)[key] if (head == "c51" and double_q) else None
    out = net(state)[key]
    if head == "c51":
        z = t(R.atoms(spec))
        res = ops.c51_loss(out.detach().contiguous(), out_t.contiguous(), action, reward, mask, discount, z, spec["v_min"],
                           spec["v_max"], logits_next_online=out_o)
        vec, dout, q_next = res["kl"], res["dlogits"], (pred_t["prob"] * z).sum(-1)
    else:
        res = ops.qr_loss(out.detach().contiguous(), out_t.contiguous(), action, reward, mask, discount)
        vec, dout, q_next = res["loss_vec"], res["dtheta"], out_t.mean(-1)
    out.backward(dout)
    torch.cuda.synchronize()
    return dict(loss=float(res["loss"].item()), loss_vec=vec.cpu().numpy(), q_next=q_next.cpu().numpy(),
                grads={k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()})


def _fractions(got, want, head, what):
    f = dict(loss=_fraction(np.asarray([got["loss"]]), np.asarray([want["loss"]]), what + " loss"),
             loss_vec=_fraction(got["loss_vec"], want["loss_vec"], what + " loss_vec"),
             q_next=_fraction(got["q_next"], want["q_next"], what + " q_next"),
             grads=max(_fraction(got["grads"][k], want["grads"][k], what + " d" + k) for k in R.keys(head)))
    if "target" in got:
        f["target"] = _fraction(got["target"], want["target"], what + " target")
    return f


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_kernel_matches_restatement(dra, case):
    """dra_dist_mlp_update against the fp64 restatement on the case's ring, indices and parameters (the target's from another
    seed): loss, loss_vec, q_next, target and the six gradients within the bars of the module's docstring, with the module path's
    own fp32 error on the same case recorded next to them; every element of the six tensors written and nothing between or behind
    them (the parameters lie behind a leading gap with NaN between them in the cases of 17 rows); the error word 0; both parameter
    buffers unchanged; with every sampled action 0 the other action's head rows get gradient exactly 0; two launches give the same
    bits."""
    head, n, hidden, gate, batch, double_q, kind, discount, _ = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    spec = u["spec"]
    padded = K.update_padded(case)
    a, b = _launch_update(dra, u["params"], u["target_params"], rg["ring"], u["idx"], spec, hidden, gate, double_q, discount, padded,
                          launches=2)
    assert a["rc"] == 0 and a["err"] == 0
    what = K.update_id(case)
    worst = _fractions(a, u, head, what)
    yard = _fractions(_module_path(dra, u, case), u, head, what + " [module path]")
    record_parity("dist_mlp update kernel vs restatement %s (fraction of the bar)" % what, **worst)
    record_parity("module path (modules, ops loss, autograd) vs restatement %s (fraction of the bar)" % what, **yard)
    for k, f in worst.items():
        allowed = max(1.0, 2.0 * yard[k]) if head == "c51" and k in yard else 1.0
        assert f <= allowed, (what, k, f, allowed, yard.get(k))
    assert np.isnan(a["gaps"]).all() and a["gaps"].size == GUARD + (_pad_floats(u["params"], head) if padded else 0)
    assert all(np.isfinite(a["grads"][k]).all() for k in R.keys(head))
    if kind == "action0":
        w, bias = R.keys(head)[4:]
        assert not a["grads"][w][n:].any() and not a["grads"][bias][n:].any()
    for k in ("loss_vec", "q_next", "target"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["loss"] == b["loss"] and all(np.array_equal(_bits(a["grads"][k]), _bits(b["grads"][k])) for k in R.keys(head))


@pytest.mark.parametrize("head", K.HEADS)
def test_update_clamps_and_counts_indices_outside_the_ring(dra, head):
    """Staged indices outside [0, capacity - 2] are clamped into it and counted in the error word: the launch computes what it
    computes on the clamped indices, bit for bit, and reads nothing outside the ring."""
    case = next(c for c in K.UPDATE_CASES if c[0] == head and c[1] == 20 and c[4] == 10 and c[6] == "partial")
    u, rg = K.restated_update(case), K.make_ring("partial")
    cap = K.RINGS["partial"]["capacity"]
    bad = u["idx"].copy()
    bad[4], bad[5], bad[6] = -3, cap - 1, cap + 7
    clamped = np.clip(bad, 0, cap - 2)
    ring = {k: v.copy() for k, v in rg["ring"].items()}
    ring["frames"][260:], ring["rewards"][260:], ring["masks"][260:], ring["actions"][260:] = 0.25, 1.0, 1, 0     # (finite everywhere)
    args = (u["spec"], case[2], case[3], case[5], case[7])
    got, = _launch_update(dra, u["params"], u["target_params"], ring, bad, *args)
    want, = _launch_update(dra, u["params"], u["target_params"], ring, clamped, *args)
    assert got["rc"] == want["rc"] == 0 and got["err"] == 3 and want["err"] == 0
    for k in ("loss_vec", "q_next", "target"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert got["loss"] == want["loss"]
    assert all(np.array_equal(_bits(got["grads"][k]), _bits(want["grads"][k])) for k in R.keys(head))


@pytest.mark.parametrize("head", K.HEADS)
def test_supported_agrees_with_the_launches(dra, head):
    """dra_dist_mlp_supported / dra_dist_mlp_update_supported say what the launches accept: over atoms {1, 2, 51, 52 (the first
    unsupported count)} x hidden {8, 16, 64, 128} x [batch {0, 1, 256, 257} | transitions {0, 8, 9}] the return code is 0 exactly
    where the table says yes."""
    from deeprl_amd import dist_mlp
    rg = K.make_ring("partial")
    ring = {k: v.copy() for k, v in rg["ring"].items()}
    ring["frames"][260:], ring["rewards"][260:], ring["masks"][260:], ring["actions"][260:] = 0.25, 1.0, 1, 0
    env, raw = K.make_env(K.ENV_SEED, 200)
    yes = 0
    for n in (1, 2, K.MAX_ATOMS, K.MAX_ATOMS + 1):
        spec = K.spec_of(head, n, (-10.0, 10.0))
        for hidden in (8, 16, 64, 128):
            params = R.init_params(hidden, 5, spec)
            for batch in (0, 1, 256, 257):
                idx = np.arange(batch, dtype=np.int64) % 250
                got, = _launch_update(dra, params, params, ring, idx, spec, hidden, "relu", False, K.DISCOUNT)
                want = dist_mlp.update_supported(4, 2, hidden, batch, 1, K.HEAD_CODE[head], n)
                assert (got["rc"] == 0) == want and got["rc"] in (0, -22), (n, hidden, batch, got["rc"])
                assert want == (2 <= n <= K.MAX_ATOMS and hidden in (16, 64) and 1 <= batch <= 256)
                yes += want
            for k_len in (0, 8, 9):
                start = dict(params=params, raw=raw.copy(), seed=env.seed, explore=np.ones(8, dtype=bool),
                             random_action=np.zeros(8, dtype=np.int64), spec=spec)
                got = _launch_act(dra, start, hidden, "relu", k_len, 64, 0, 200, False)
                want = dist_mlp.supported(4, 2, hidden, k_len, 1, K.HEAD_CODE[head], n)
                assert (got["rc"] == 0) == want and got["rc"] in (0, -22), (n, hidden, k_len, got["rc"])
                assert want == (2 <= n <= K.MAX_ATOMS and hidden in (16, 64) and k_len == 8)
                yes += want
    assert yes == 2 * 2 * 2 + 2 * 2


@pytest.mark.parametrize("tag", [t[0] for t in K.FIXTURE_TAGS])
def test_update_kernel_matches_reference_steps(dra, tag):
    """The reference's recorded run (tests/golden/dist_feature/): from the recorded initial parameters, every update of the run --
    dra_dist_mlp_update on the recorded ring rows and indices, then the fused clip + RMSprop step, the target copied where the
    reference copies it -- lands on the reference's parameters after every step within rtol 2e-5 / atol 2e-6; the losses too."""
    from deeprl_amd import dist_mlp, ops
    from deeprl_amd._lib import lib, stream_ptr
    from deeprl_amd.optim import FlatParams, FusedOptimizer
    d, dev = dra, dra.Config.DEVICE
    z = np.load(FIXTURE)
    _, head, _, _, double_q, freq, hidden = next(t for t in K.FIXTURE_TAGS if t[0] == tag)
    f = K.FIXTURE
    spec = K.fixture_spec(head)
    mk = lambda: (d.CategoricalNet if head == "c51" else d.QuantileNet)(2, f["n"], d.FCBody(4, (hidden, hidden)))
    net, tgt = mk(), mk()
    fused = FusedOptimizer.adopt(torch.optim.RMSprop(net.parameters(), K.LR))
    tflat = FlatParams(list(tgt.parameters()))
    with torch.no_grad():
        for k, p in net.state_dict().items():
            p.copy_(torch.from_numpy(z["%s_init_%s" % (tag, k)]))
        for k, p in tgt.state_dict().items():
            p.copy_(torch.from_numpy(z["%s_target0_%s" % (tag, k)]))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frames, actions, rewards, masks = (t(z["%s_ring_%s" % (tag, k)]) for k in ("frames", "actions", "rewards", "masks"))
    zeros = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    loss, vec, qn, tg = zeros(1), zeros(f["batch"] if head == "c51" else f["n"]), zeros(f["batch"], 2), zeros(f["batch"], f["n"])
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    n = dist_mlp.Net()
    n.param, n.target = fused.flat.flat.data_ptr(), tflat.flat.data_ptr()
    for field, p in dist_mlp._fields(net):
        setattr(n, field, fused.flat.offset_of(p))
    n.state_dim, n.n_actions, n.hidden, n.gate = 4, 2, hidden, 1
    n.head, n.n_atoms, n.v_min, n.v_max = K.HEAD_CODE[head], f["n"], spec["v_min"], spec["v_max"]
    worst, losses = 0.0, []
    for s in range(f["steps"]):
        idx = z[tag + "_indices"][s]
        if idx[0] >= 0:
            assert idx.max() + 1 < f["k"] * (s + 1)          # (rows the run had written by then)
            idx_t = t(idx)
            io = dist_mlp.UpdateIO()
            io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = frames.data_ptr(), actions.data_ptr(), rewards.data_ptr(), masks.data_ptr()
            io.idx, io.grad = idx_t.data_ptr(), fused.flat.grad.data_ptr()
            io.out_loss, io.out_loss_vec, io.out_q_next, io.out_target = loss.data_ptr(), vec.data_ptr(), qn.data_ptr(), tg.data_ptr()
            io.err, io.capacity, io.discount, io.batch, io.double_q = err.data_ptr(), f["capacity"], K.DISCOUNT, f["batch"], int(double_q)
            lib.dra_dist_mlp_update(ctypes.byref(n), ctypes.byref(io), stream_ptr())
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
    record_parity("dist_feature update kernel vs reference steps %s (fraction of the bar)" % tag, params=worst)


# ------------------------------------------------------------------------------------------ the agents
A = K.AGENT


def _config(d, head, feature, graph=True, exploration_steps=None, **extra):
    from deeprl_amd import zoo
    from deeprl_amd.replay import ReplayWrapper, UniformReplay
    kw = dict(fused_dist_feature=True) if feature else {}
    shape = (dict(categorical_n_atoms=A["n"], categorical_v_min=A["v_min"], categorical_v_max=A["v_max"]) if head == "c51"
             else dict(num_quantiles=A["n"]))
    c = zoo.config(ENTRY[head], game=GAME, tag="dist_feat_%s%d%d" % (head, feature, graph), graph_update=graph,
                   overrides=dict(sgd_update_frequency=A["k"], batch_size=A["batch"], target_network_update_freq=A["target_freq"],
                                  exploration_steps=A["exploration_steps"] if exploration_steps is None else exploration_steps,
                                  double_q=A["double_q"], **shape, **extra), **kw)
    c.task_fn = lambda: d.Task(c.game, seed=A["task_seed"], synthetic_done_period=A["horizon"])
    rk = dict(memory_size=A["capacity"], batch_size=A["batch"])
    c.replay_fn = lambda: ReplayWrapper(UniformReplay, rk, False)
    c.random_action_prob = d.LinearSchedule(*A["eps"])
    c.log_interval = 10 ** 9
    return c


def _agent_cls(d, head):
    return d.CategoricalDQNAgent if head == "c51" else d.QuantileRegressionDQNAgent


def _make_agent(d, monkeypatch, head, feature, graph=True, **kw):
    import deeprl_amd.agents as agents_mod
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    d.random_seed(9)
    torch.manual_seed(9)
    agent = _agent_cls(d, head)(_config(d, head, feature, graph, **kw))
    # the case's parameters (numpy-seeded: the same on every machine), copied into the optimiser's flat buffer through the views;
    # the target starts as their copy (DQN_agent.py:57)
    init = K.restated_agent_run(head)["init"]
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


def _run(d, monkeypatch, head, feature, graph=True, steps=A["steps"], **kw):
    from deeprl_amd.device_env import DeviceCartPoleVec
    from deeprl_amd.dist_mlp import Step
    agent, rec = _make_agent(d, monkeypatch, head, feature, graph, **kw)
    assert isinstance(agent.actor._task, DeviceCartPoleVec) == bool(feature) and (agent._feature is not None) == bool(feature), rec.warnings
    assert not feature or type(agent._feature) is Step
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


_DEVICE_RUNS = {}


@pytest.fixture
def device_run(dra, request):
    """Eight steps of a head kind's device path (the update kernel: config.fused_dist_update True) with graph replay: computed
    once per head kind, shared, left unchanged."""
    head = request.node.callspec.params["head"]
    if head not in _DEVICE_RUNS:
        mp = pytest.MonkeyPatch()
        try:
            _DEVICE_RUNS[head] = _run(dra, mp, head, True, True, fused_dist_update=True)
        finally:
            mp.undo()
    return _DEVICE_RUNS[head]


def _params_within(a, others, bar=2e-4):
    worst = 0.0
    for other in others:
        for k in a:
            scale = max(np.abs(other[k]).max(), 1e-2)
            worst = max(worst, float(np.max(np.abs(a[k] - other[k])) / (bar * scale)))
    return worst


@pytest.mark.parametrize("head", K.HEADS)
def test_agent_device_path_equals_host_loop_and_restatement(dra, monkeypatch, head, device_run):
    """The agent on its feature configuration (one cart-pole with episodes of at most 5 steps, 4 transitions per step,
    exploration_steps 6 crossed inside the second step, minibatches of 10 from a replay of 24 slots that wraps, a target copy every
    3 steps, 20 atoms) with config.fused_dist_feature -- eager steps, then graph replays -- against the same agent with the switch
    off (the parent commit's path) and against the fp64 restatement, over 8 agent steps: actions, the replay ring's four arrays,
    its cursor, the sampled indices, total_steps, the episodic-return log lines, the np.random tail and the schedule's position
    equal; online and target parameters within 2e-4 of each tensor's largest magnitude (floor 1e-2), the family's bar."""
    from deeprl_amd.dist_mlp import Step
    a, b = device_run, _run(dra, monkeypatch, head, False)
    want = K.restated_agent_run(head)
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
    record_parity("dist_feature %s agent device vs host loop and restatement (fraction of the bar)" % head, params=worst)
    assert worst <= 1.0


@pytest.mark.parametrize("head", K.HEADS)
def test_module_update_form_matches_the_fused_one(dra, monkeypatch, head, device_run):
    """config.fused_dist_update False (device acting and ring, ring.gather and the agent's own _loss_grad on the same indices) over
    the same eight steps: the same actions, ring, indices and events; parameters within the agent test's bar."""
    b = _run(dra, monkeypatch, head, True, fused_dist_update=False)
    a = device_run
    assert b['graphed'] == dict(act=False, learn=True) and np.array_equal(a['actions'], b['actions'])
    assert np.array_equal(_bits(a['ring']['frames']), _bits(b['ring']['frames'])) and np.array_equal(a['ring']['masks'], b['ring']['masks'])
    assert a['events'] == b['events'] and a['lines'] == b['lines'] and a['total'] == b['total'] and np.array_equal(a['rng'], b['rng'])
    worst = _params_within(a['params'], (b['params'],))
    record_parity("dist_feature %s fused update vs module update on the device (fraction of the bar)" % head, params=worst)
    assert worst <= 1.0


@pytest.mark.parametrize("head", K.HEADS)
def test_graph_replay_equals_eager(dra, monkeypatch, head):
    """exploration_steps 14: four acting-only steps (two eager, the capture, a replay), then six learning steps (two eager, the
    capture, replays) with target copies between replays.  config.graph_update False keeps every step eager: parameters, ring,
    actions and events are equal to the bit."""
    a = _run(dra, monkeypatch, head, True, graph=True, steps=10, exploration_steps=14, fused_dist_update=True)
    b = _run(dra, monkeypatch, head, True, graph=False, steps=10, exploration_steps=14, fused_dist_update=True)
    assert a['graphed'] == dict(act=True, learn=True) and b['graphed'] == dict(act=False, learn=False)
    assert a['launches'] == 3 + 3 and b['launches'] == 10
    assert a['total'] == b['total'] and a['lines'] == b['lines'] and a['events'] == b['events'] and np.array_equal(a['rng'], b['rng'])
    assert np.array_equal(a['actions'], b['actions'])
    for k in a['ring']:
        assert np.array_equal(_bits(a['ring'][k]), _bits(b['ring'][k])), k
    for k in a['params']:
        assert np.array_equal(_bits(a['params'][k]), _bits(b['params'][k])) and np.array_equal(_bits(a['target'][k]), _bits(b['target'][k])), k


@pytest.mark.parametrize("head", K.HEADS)
def test_save_load_continues_the_run(dra, monkeypatch, head, device_run, tmp_path):
    """4 steps, save() + the replay's save_full(), a fresh agent, load() + load_full(), 4 more steps == 8 uninterrupted steps, bit
    for bit.  The optimiser's running averages, the target network, the step counters, the schedule and the np.random state are no
    part of a checkpoint, so the test carries them over by hand."""
    first, rec = _make_agent(dra, monkeypatch, head, True, fused_dist_update=True)
    for _ in range(4):
        first.step()
    name = str(tmp_path / "ckpt")
    first.save(name)
    first._inner_replay().save_full(name)
    assert os.path.isfile(name + ".envs") and os.path.isfile(name + ".model") and os.path.isfile(name + ".replay")
    rng = np.random.get_state()
    second, rec2 = _make_agent(dra, monkeypatch, head, True, fused_dist_update=True)
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


@pytest.mark.parametrize("head", K.HEADS)
def test_default_config_stays_on_the_host(dra, monkeypatch, head):
    """A default-Config agent on the cart-pole Task keeps envs.Task and logs nothing (the path is opt-in); switching on with a
    network the kernels do not walk (VanillaNet), or on a plain DQNAgent, keeps the host path and logs a warning naming the
    reason."""
    import deeprl_amd.agents as agents_mod
    d = dra
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    agent = _agent_cls(d, head)(_config(d, head, False))
    assert agent._feature is None and type(agent.actor._task) is d.Task and rec.warnings == []
    assert agent.episodes() == [] and agent.drain_episodes() == []
    agent.step()
    assert agent.total_steps == A["k"] and agent.actor._task.env.envs[0].c == A["k"]
    agent.close()
    c = _config(d, head, True)
    c.network_fn = lambda: d.VanillaNet(c.action_dim, d.FCBody(c.state_dim))
    agent = _agent_cls(d, head)(c)
    assert agent._feature is None and type(agent.actor._task) is d.Task
    assert len(rec.warnings) == 1 and "the network is not CategoricalNet / QuantileNet" in rec.warnings[0]
    agent.close()
    agent = d.DQNAgent(c)
    assert agent._feature is None and type(agent.actor._task) is d.Task
    assert len(rec.warnings) == 2 and "not a CategoricalDQNAgent or a QuantileRegressionDQNAgent" in rec.warnings[1]
    agent.step()
    assert agent.total_steps == A["k"]
    agent.close()


@pytest.mark.parametrize("head", K.HEADS)
def test_closed_loop_learns(dra, monkeypatch, head):
    """The zoo entry itself (hidden 64, replay of 10^4, exploration_steps 100, epsilon 1.0 -> 0.1 over 10^4, a target copy every
    200 updates; 50 atoms on [-100, 100] / 20 quantiles) with config.fused_dist_feature and the update kernel for the number of environment steps at
    which the REFERENCE's own median over five seeds reaches 2 x the bar (tests/golden/dist_feature/learning_reference.json:
    n_learn): the median over three seeds of the mean return of the last 100 training episodes reaches the bar, 2 x the random
    policy's mean (44.2)."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    from deeprl_amd.device_env import DeviceCartPoleVec
    d = dra
    ref = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))[head]
    bar, n_learn = ref["bar"], ref["n_learn"]
    assert n_learn is not None and abs(bar - 44.2) < 0.1
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    means = []
    for seed in K.LEARN_SEEDS:
        d.random_seed(seed)
        torch.manual_seed(seed)
        c = zoo.config(ENTRY[head], game=GAME, tag="dist_feat_learn_%s%d" % (head, seed), fused_dist_feature=True, fused_dist_update=True)
        c.task_fn = lambda seed=seed, c=c: d.Task(c.game, seed=seed)
        c.log_interval = 10 ** 9
        agent = _agent_cls(d, head)(c)
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
    record_parity("dist_feature %s closed loop: last-100 mean returns per seed, median, bar" % head, median=median, bar=bar,
                  **{"seed%d" % s: m for s, m in zip(K.LEARN_SEEDS, means)})
    assert median >= bar, (means, bar)
