"""dra_dqn_replay_mlp_update (csrc/dqn_mlp.hip: dqn_feature's update over an n-step window with optional priorities) on the device,
against the fp64 restatement (tests/dqn_replay_feature_restatement.py, pinned to the reference's own run and replay by
tests/test_dqn_replay_feature_host.py), with the module form (ring.gather, the modules, ops.td_loss) recorded next to it, against
dra_dqn_mlp_update bit for bit where the window is 1 and there are no priorities, and at its edges: beta read from the device, the
clamp of staged indices, the supported-shape table."""
import ctypes

import numpy as np
import pytest
import torch
from feature_kernel_harness import GUARD, dra, _fraction, _bits, _guarded      # noqa: F401  (dra: the fixture)
from parity_log import record_parity

import dqn_feature_cases as K1
import dqn_replay_feature_cases as K
import dqn_replay_feature_restatement as R
from test_gpu_dqn_feature import _launch_update as _launch_one_step, _net_struct

pytestmark = pytest.mark.gpu

OUTS = ("q_target", "td", "prio", "weights")
QUANTITIES = ("q_target", "td", "loss", "prio", "weights", "grads")


def _launch(dra, params, target, ring, idx, hidden, gate, double_q, n_step, prob=None, beta=None, alpha=0.5, padded=False,
            launches=1, discount=K.DISCOUNT):
    """dra_dqn_replay_mlp_update on host arrays -> per launch dict(q_target, td, loss, prio, weights (NaN-filled where prob is
    None: the launch must leave them alone), grads by name, gaps: the gradient buffer outside the six tensors, err, rc)."""
    from deeprl_amd import dqn_replay_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    net, flat, tflat, offs = _net_struct(params, target, dev, hidden, gate, padded)
    cap, b = ring["actions"].shape[0], len(idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frames, actions, rewards, masks = t(ring["frames"]), t(ring["actions"]), t(ring["rewards"]), t(ring["masks"])
    idx_t = t(np.asarray(idx, dtype=np.int64))
    per = prob is not None
    prob_t = t(np.asarray(prob, dtype=np.float32)) if per else None
    beta_t = torch.full((1,), float(beta), dtype=torch.float32, device=dev) if per else None
    outs = []
    for _ in range(launches):
        grad_full, grad = _guarded((flat.numel(),), torch.float32, dev, float("nan"))
        full = {k: _guarded((n,), torch.float32, dev, float("nan")) for k, n in (("q_target", b), ("td", b), ("loss", 1), ("prio", b),
                                                                                ("weights", b))}
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        io = dqn_replay_mlp.UpdateIO()
        io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = frames.data_ptr(), actions.data_ptr(), rewards.data_ptr(), masks.data_ptr()
        io.idx, io.grad = idx_t.data_ptr(), grad.data_ptr()
        io.out_q_target, io.out_td, io.out_loss = (full[k][1].data_ptr() for k in ("q_target", "td", "loss"))
        # (a uniform launch is handed the priority buffers all the same: it must not write them)
        io.out_prio, io.out_weights = full["prio"][1].data_ptr(), full["weights"][1].data_ptr()
        if per:
            io.prob, io.beta = prob_t.data_ptr(), beta_t.data_ptr()
        io.err, io.capacity, io.discount, io.step_discount = err.data_ptr(), cap, float(discount) ** n_step, float(discount)
        io.replay_eps, io.replay_alpha = K.REPLAY_EPS, float(alpha)
        io.batch, io.double_q, io.n_step = b, int(double_q), n_step
        before = flat.cpu().numpy().copy(), tflat.cpu().numpy().copy()
        rc = lib.dra_dqn_replay_mlp_update.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(flat.cpu().numpy()), _bits(before[0])) and np.array_equal(_bits(tflat.cpu().numpy()), _bits(before[1]))
        g = grad_full.cpu().numpy()
        covered = np.zeros(g.size, dtype=bool)
        grads = {}
        for k in R.KEYS:
            n = int(np.asarray(params[k]).size)
            grads[k] = g[offs[k]:offs[k] + n].reshape(np.asarray(params[k]).shape)
            covered[offs[k]:offs[k] + n] = True
        for k, (full_t, body) in full.items():
            assert torch.isnan(full_t[body.numel():]).all(), k
        out = dict(rc=rc, loss=float(full["loss"][1].item()), grads=grads, gaps=g[~covered], err=int(err.item()))
        out.update({k: full[k][1].cpu().numpy() for k in OUTS})
        outs.append(out)
    return outs


def _launch_case(dra, case, launches=1, **over):
    hidden, gate, batch, double_q, n_step, kind, per, alpha, beta = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    kw = dict(prob=u["prob"], beta=beta if per else None, alpha=alpha, padded=batch == 65, launches=launches)
    kw.update(over)
    return _launch(dra, u["params"], u["target"], rg["ring"], kw.pop("idx", u["idx"]), hidden, gate, double_q, n_step, **kw)


def _fractions(got, want, what, per):
    f = dict(loss=_fraction(np.asarray([got["loss"]]), np.asarray([want["loss"]]), what + " loss"),
             grads=max(_fraction(got["grads"][k], want["grads"][k], what + " d" + k) for k in R.KEYS))
    f.update({k: _fraction(got[k], want[k], what + " " + k) for k in (OUTS if per else OUTS[:2])})
    return f


def _module_update(dra, case):
    """The module form of the update on a kernel case (what config.fused_dqn_replay_update = False runs): an ops.Ring holding the
    case's ring with the case's window, ring.gather at the data indices, VanillaNet modules holding the case's parameters,
    ops.td_loss with the device beta behind the probabilities, autograd -> dict(q_target, td, loss, prio, weights, grads)."""
    from deeprl_amd import ops
    d, dev = dra, dra.Config.DEVICE
    hidden, gate, batch, double_q, n_step, kind, per, alpha, beta = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    fn = {"relu": torch.relu, "tanh": torch.tanh}[gate]

    def make(params):
        net = d.VanillaNet(2, d.FCBody(4, hidden_units=(hidden, hidden), gate=fn))
        net.load_state_dict({k: torch.from_numpy(np.asarray(params[k])) for k in R.KEYS})
        return net
    net, tnet = make(u["params"]), make(u["target"])
    cap = rg["ring"]["actions"].shape[0]
    ring = ops.Ring(cap, 32, 8, 1, n_step, K.DISCOUNT)
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        frames, actions, rewards, masks = ring.arrays()
        frames.view(torch.float64).copy_(t(rg["ring"]["frames"]).view(-1))
        actions.view(torch.int64).copy_(t(rg["ring"]["actions"]))
        rewards.copy_(t(rg["ring"]["rewards"]))
        masks.copy_(t(rg["ring"]["masks"]))
        g = ring.gather(t(u["idx"]), (4,), torch.float64, torch.int64)
        states, nxt = g["state"].float(), g["next_state"].float()
        reward, mask = g["reward"].float(), g["mask"].float()
        with torch.no_grad():
            q_next = tnet(nxt)['q']
            q_next_online = net(nxt)['q'] if double_q else None
        q = net(states)['q']
        kw = {}
        if per:      # beta directly behind the last probability, read on the device (beta < 0)
            kw = dict(sampling_prob=t(np.concatenate([u["prob"], np.asarray([beta], dtype=np.float32)]))[:batch], beta=-1.0,
                      replay_eps=K.REPLAY_EPS, replay_alpha=alpha)
        out = ops.td_loss(q.detach(), q_next, g["action"], reward, mask, K.DISCOUNT ** n_step, q_next_online=q_next_online, **kw)
        q.backward(out['dq'])
        torch.cuda.synchronize()
        grads = {k: p.grad.cpu().numpy() for k, p in net.named_parameters()}
        td = out['delta'].cpu().numpy()
        q_a = q.detach().gather(1, g["action"].view(-1, 1)).squeeze(1).cpu().numpy()
        got = dict(td=td, q_target=td + q_a, loss=float(out['loss'].item()), grads=grads)
        if per:
            got.update(prio=out['prio'].cpu().numpy(), weights=out['weights'].cpu().numpy())
        return got
    finally:
        ring.close()


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_kernel_matches_restatement(dra, case):
    """dra_dqn_replay_mlp_update against the fp64 restatement on the case's ring, data indices, probabilities and parameters (the
    target's from another seed): q_target, td, the loss, the priorities, the weights and the six gradients within 1e-5 of scale --
    where the module form of the same case (recorded next to the kernel) itself exceeds the bar for a quantity, within max(1, twice
    the module form's fraction); every element of the six tensors written and nothing between or behind them (the parameters lie
    behind a leading gap with NaN between them in the cases of 65 rows); a uniform launch leaves the priority and weight buffers
    alone; the error word 0; both parameter buffers unchanged; two launches give the same bits."""
    hidden, gate, batch, double_q, n_step, kind, per, alpha, beta = case
    u = K.restated_update(case)
    what = K.update_id(case)
    a, b = _launch_case(dra, case, launches=2)
    assert a["rc"] == 0 and a["err"] == 0
    worst = _fractions(a, u, "kernel " + what, per)
    mod = _module_update(dra, case)
    # (the module form's q_target is td + q_a, rounded once more than the kernel's: a yardstick only for the rest)
    yard = _fractions(mod, u, "modules " + what, per)
    record_parity("dqn_replay_mlp update kernel vs restatement %s (fraction of the bar)" % what, **worst)
    record_parity("dqn_replay_mlp module form vs restatement %s (fraction of the bar)" % what, **yard)
    for k, f in worst.items():
        assert f <= max(1.0, 2.0 * yard[k] if k != "q_target" else 1.0), (what, k, f, yard[k])
    padded = batch == 65
    assert np.isnan(a["gaps"]).all() and a["gaps"].size == GUARD + ((3 + sum((-np.asarray(u["params"][k]).size) % 4 + 1 for k in R.KEYS)) if padded else 0)
    assert all(np.isfinite(a["grads"][k]).all() for k in R.KEYS)
    if per:
        assert a["weights"].max() == 1.0 and (batch < 65 or int(np.argmax(a["weights"])) == batch - 1)
    else:
        assert np.isnan(a["prio"]).all() and np.isnan(a["weights"]).all()
    for k in OUTS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["loss"] == b["loss"] and all(np.array_equal(_bits(a["grads"][k]), _bits(b["grads"][k])) for k in R.KEYS)


@pytest.mark.parametrize("case", K1.UPDATE_CASES, ids=K1.update_id)
def test_window_of_one_without_priorities_is_the_one_step_kernel(dra, case):
    """The anchor: with prob NULL and n_step 1 every output and every gradient element equals dra_dqn_mlp_update's bit for bit, on
    that kernel's own cases."""
    hidden, gate, batch, double_q, kind = case
    u, rg = K1.restated_update(case), K1.make_ring(kind)
    padded = batch == 65
    want, = _launch_one_step(dra, u["params"], u["target"], rg["ring"], u["idx"], hidden, gate, double_q, padded)
    got, = _launch(dra, u["params"], u["target"], rg["ring"], u["idx"], hidden, gate, double_q, 1, padded=padded)
    assert got["rc"] == want["rc"] == 0 and got["err"] == want["err"] == 0
    for k in ("q_target", "td"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert np.array_equal(_bits(np.float32(got["loss"])), _bits(np.float32(want["loss"])))
    for k in R.KEYS:
        assert np.array_equal(_bits(got["grads"][k]), _bits(want["grads"][k])), k
    assert np.array_equal(_bits(got["gaps"]), _bits(want["gaps"]))
    assert np.isnan(got["prio"]).all() and np.isnan(got["weights"]).all()


def test_beta_is_read_from_the_device(dra):
    """Two launches that differ in the device word beta alone: each gives that beta's weights (within the bar of the restatement's),
    and the same q_target, td and priority bits."""
    case = K.UPDATE_CASES[0]
    hidden, gate, batch, double_q, n_step, kind, per, alpha, beta = case
    u = K.restated_update(case)
    outs = {}
    for bt in (0.4, 1.0):
        outs[bt], = _launch_case(dra, case, beta=bt)
        sp = u["prob"].astype(np.float64)
        w = (sp * batch + 1e-6) ** -bt
        assert _fraction(outs[bt]["weights"], w / w.max(), "weights at beta %g" % bt) <= 1.0
    assert not np.array_equal(outs[0.4]["weights"], outs[1.0]["weights"]) and outs[0.4]["loss"] != outs[1.0]["loss"]
    for k in ("q_target", "td", "prio"):
        assert np.array_equal(_bits(outs[0.4][k]), _bits(outs[1.0][k])), k


@pytest.mark.parametrize("case", [K.UPDATE_CASES[0], K.UPDATE_CASES[8]], ids=K.update_id)
def test_update_clamps_and_counts_indices_outside_the_window_range(dra, case):
    """Staged indices outside [0, capacity - 1 - n_step] are clamped into it and counted in the error word: the launch computes
    what it computes on the clamped indices, bit for bit (the ring is full and finite: nothing outside it is read)."""
    n_step, kind = case[4], case[5]
    u = K.restated_update(case)
    cap = K.RINGS[kind]["capacity"]
    bad = u["idx"].copy()
    bad[4], bad[5], bad[6], bad[7] = -3, cap - n_step, cap - 1, cap + 7
    clamped = np.clip(bad, 0, cap - 1 - n_step)
    assert np.isfinite(K.make_ring(kind)["ring"]["frames"]).all()
    got, = _launch_case(dra, case, idx=bad)
    want, = _launch_case(dra, case, idx=clamped)
    assert got["rc"] == want["rc"] == 0 and got["err"] == 4 and want["err"] == 0
    for k in OUTS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert got["loss"] == want["loss"]
    assert all(np.array_equal(_bits(got["grads"][k]), _bits(want["grads"][k])) for k in R.KEYS)


def test_supported_table_agrees_with_the_launches(dra):
    """dra_dqn_replay_mlp_update_supported says what the launch accepts: over hidden {16, 32, 48} x gate {0, 1, 2} x batch {0, 1,
    256, 257} x n_step {0, 1, 8, 9} the return code is 0 exactly where the table says yes."""
    from deeprl_amd import dqn_replay_mlp
    rg = K.make_ring("window_full")
    seen = set()
    params = R.init_params(64, 5)
    for hidden in (16, 32, 48):
        for gate in (0, 1, 2):
            for batch in (0, 1, 256, 257):
                for n_step in (0, 1, 8, 9):
                    ok = dqn_replay_mlp.update_supported(4, 2, hidden, batch, gate, n_step)
                    idx = np.full(max(batch, 1), 30, dtype=np.int64)[:batch] if batch else np.zeros(0, dtype=np.int64)
                    name = {0: "relu", 1: "relu", 2: "tanh"}[gate]
                    got, = _launch_table(dra, params, rg["ring"], idx, hidden, gate, name, n_step)
                    assert (got == 0) == bool(ok), (hidden, gate, batch, n_step, got, ok)
                    seen.add(bool(ok))
    assert seen == {True, False}


def _launch_table(dra, params, ring, idx, hidden, gate_code, gate, n_step):
    """The return code of one launch with the net struct's hidden and gate fields set as given."""
    from deeprl_amd import dqn_replay_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    net, flat, tflat, offs = _net_struct(params, params, dev, 64, gate, False)      # (buffers of the largest width's layout)
    net.hidden, net.gate = hidden, gate_code
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frames, actions, rewards, masks = t(ring["frames"]), t(ring["actions"]), t(ring["rewards"]), t(ring["masks"])
    b = max(len(idx), 1)
    idx_t = t(np.asarray(idx if len(idx) else [0], dtype=np.int64))
    grad = torch.zeros(flat.numel(), dtype=torch.float32, device=dev)
    bufs = [torch.zeros(b, dtype=torch.float32, device=dev) for _ in range(3)]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    io = dqn_replay_mlp.UpdateIO()
    io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = frames.data_ptr(), actions.data_ptr(), rewards.data_ptr(), masks.data_ptr()
    io.idx, io.grad = idx_t.data_ptr(), grad.data_ptr()
    io.out_q_target, io.out_td, io.out_loss = (x.data_ptr() for x in bufs)
    io.err, io.capacity, io.discount, io.step_discount = err.data_ptr(), ring["actions"].shape[0], 0.99, 0.99
    io.batch, io.double_q, io.n_step = len(idx), 0, n_step
    rc = lib.dra_dqn_replay_mlp_update.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    return (rc,)
