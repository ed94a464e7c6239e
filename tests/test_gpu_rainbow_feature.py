"""rainbow_feature's two kernels on the device (csrc/rainbow_mlp.hip, deeprl_amd/rainbow_mlp.py) against the fp64 restatement
(tests/rainbow_feature_restatement.py, pinned to the reference's own RainbowNet and replay fold by
tests/test_rainbow_feature_host.py): the acting launch with one noise row per transition, and the whole update -- n-step gather,
target network under its noise, online network under one draw, double_q, projection, KL, priorities, importance weights and the
gradient of all sixteen tensors.

The bars.  Every tensor: the family's 1e-5 of its largest magnitude (floor 1.0); everything discrete equal to the bit."""
import ctypes
import os

import numpy as np
import pytest
import torch
from feature_kernel_harness import (      # noqa: F401  (dra: the fixture)
    GATE, GUARD, dra, _fraction, _bits, _guarded, _flat, _body, _launch_replay_act, _check_act, _check_act_case,
    _check_bad_slots)
from parity_log import record_parity

import rainbow_feature_cases as K
import rainbow_feature_restatement as R

pytestmark = pytest.mark.gpu

ROW_GAP = 3      # floats between two noise rows of a padded block: the stride is not the row's length


def _pad_floats(params):
    return 3 + sum((-np.asarray(params[k]).size) % 4 + 1 for k in R.KEYS)


def _noise_block(rows, hidden, n, padded, dev):
    """(device block [len(rows)][stride], offsets, stride) of raw noise dicts; padded: NaN between and behind the vectors."""
    offs, size = K.noise_layout(hidden, n, padded)
    stride = size + (ROW_GAP if padded else 0)
    block = np.full((len(rows), stride), np.nan if padded else 0.0, dtype=np.float32)
    for r, z in enumerate(rows):
        block[r, :size] = K.noise_row(z, hidden, n, padded)
    return torch.from_numpy(block).to(dev), offs, stride


def _net_struct(params, target, noise_rows, target_noise, dev, spec, hidden, gate, padded):
    """-> (net struct, the device tensors it points to -- kept alive by the caller --, parameter offsets)."""
    from deeprl_amd import rainbow_mlp
    n = spec["n"]
    flat, offs = _flat(R.KEYS, params, padded)
    tflat, _ = _flat(R.KEYS, target if target is not None else params, padded)
    flat, tflat = torch.from_numpy(flat).to(dev), torch.from_numpy(tflat).to(dev)
    noise, noffs, stride = _noise_block(noise_rows, hidden, n, padded, dev)
    tnoise, _, _ = _noise_block([target_noise if target_noise is not None else noise_rows[0]], hidden, n, padded, dev)
    net = rainbow_mlp.Net()
    net.param, net.target, net.noise, net.target_noise = flat.data_ptr(), tflat.data_ptr(), noise.data_ptr(), tnoise.data_ptr()
    for field, layer in zip(rainbow_mlp.LAYERS, R.LAYERS):
        s = getattr(net, field)
        s.w_mu, s.w_sigma, s.b_mu, s.b_sigma = [offs["%s.%s" % (layer, p)] for p in R.PARAMS]
        s.e_in, s.e_out, s.e_b = [noffs["%s.%s" % (layer, b)] for b in R.NOISE]
    net.noise_stride = stride
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, hidden, GATE[gate]
    net.n_atoms, net.v_min, net.v_max = n, spec["v_min"], spec["v_max"]
    return net, (flat, tflat, noise, tnoise), offs


# ------------------------------------------------------------------------------------------ the acting kernel
def _launch_act(dra, start, hidden, gate, k_len, cap, slot0, horizon, padded):
    """One dra_rainbow_mlp_act from a case's start -> dict of host arrays (guards included) and the return code; the parameter and
    the noise buffers are read only."""
    from deeprl_amd._lib import lib
    kk = max(k_len, 1)
    rows = (list(start["noise_rows"]) + [start["noise_rows"][-1]] * kk)[:kk]
    net, keep, _ = _net_struct(start["params"], None, rows, None, dra.Config.DEVICE, start["spec"], hidden, gate, padded)
    return _launch_replay_act(dra, lib.dra_rainbow_mlp_act, net, keep, K, start, k_len, cap, slot0, horizon)


def _launch_act_case(dra, case, start, slot0=None):
    hidden, gate, n, k_len, cap, s0, horizon, padded, _ = case
    return _launch_act(dra, start, hidden, gate, k_len, cap, s0 if slot0 is None else slot0, horizon, padded)


@pytest.mark.parametrize("case", K.ACT_CASES, ids=K.act_id)
def test_act_kernel_matches_restatement(dra, case):
    """dra_rainbow_mlp_act against the restatement, every transition under a noise row of its own: the ring's four arrays (the rows
    written AND the rows left alone), the actions (the host suite asserts an action-value margin >= 1e-4 at every transition of every
    case), the environment's arrays, the episode ring's rows and count and the step counter equal to the bit; q within 1e-5 of
    scale; the error word still 0; the guard elements behind every buffer, the parameter and the noise buffers untouched (the padded
    case has NaN between the noise vectors and between the rows); a second launch from the same start gives the same bits."""
    hidden, gate, n, k_len, cap, slot0, horizon, padded, _ = case
    want, env, start = K.restated_act(case)
    _check_act_case(lambda: _launch_act_case(dra, case, start), want, env, K, k_len, slot0,
                    "rainbow_mlp acting kernel vs restatement %s (fraction of the bar)" % K.act_id(case))


def test_act_reads_noise_row_k_at_transition_k(dra):
    """One parameter set whose greedy action alternates 0, 1, 0, 1, ... through the noise rows alone (the host suite asserts that
    under row 0 alone or row K - 1 alone the restatement chooses otherwise): the launch alternates, and with every row replaced by
    row 0 / by row K - 1 it does what the restatement does under that row alone."""
    want, env, start = K.flip_case()
    f = K.FLIP
    out = _launch_act(dra, start, f["hidden"], f["gate"], f["k"], 64, 0, 200, False)
    assert _check_act(out, want, env, K, f["k"], 0) <= 1.0
    assert list(_body(out, "action")) == [k % 2 for k in range(f["k"])]
    for fixed in (0, f["k"] - 1):
        rows = [start["noise_rows"][fixed]] * f["k"]
        e, raw = K.make_env(K.ENV_SEED, 200)
        ring = R.new_ring(64)
        alone = R.act(start["params"], rows, e, raw, f["k"], start["explore"], start["random_action"], ring, 0, start["spec"],
                      gate=f["gate"], step0=K.STEP0)
        alone["ring"] = ring
        assert alone["margin"] >= K.MARGIN and not np.array_equal(alone["action"], want["action"])
        got = _launch_act(dra, dict(start, noise_rows=rows), f["hidden"], f["gate"], f["k"], 64, 0, 200, False)
        assert _check_act(got, alone, e, K, f["k"], 0) <= 1.0


def test_act_takes_the_staged_random_action_where_told(dra):
    """The staged explore / random_action words are kept (the host stages 0 under noisy layers): where explore is set the
    transition takes random_action, as in the siblings."""
    case = next(c for c in K.ACT_CASES if c[3] == 4 and c[2] == 50 and c[0] == 64)
    hidden, gate, n, k_len, cap, slot0, horizon, padded, _ = case
    _, _, start = K.restated_act(case)
    explore = np.asarray([False, True, True, False])
    rand = np.asarray([1, 1, 0, 0], dtype=np.int64)
    env, raw = K.make_env(K.ENV_SEED, horizon)
    ring = R.new_ring(cap)
    want = R.act(start["params"], start["noise_rows"], env, raw, k_len, explore, rand, ring, slot0, start["spec"], gate=gate,
                 step0=K.STEP0)
    want["ring"] = ring
    assert want["margin"] >= 100 * K.MARGIN
    out = _launch_act_case(dra, case, dict(start, explore=explore, random_action=rand))
    assert _check_act(out, want, env, K, k_len, slot0) <= 1.0
    assert list(_body(out, "action")[1:3]) == [1, 0]


def test_act_counts_a_first_slot_outside_the_ring(dra):
    """A staged first slot outside [0, capacity) is taken as 0 and counted in the error word: the launch equals the launch from
    slot 0 bit for bit, and nothing outside the ring is written."""
    case = next(c for c in K.ACT_CASES if c[3] == 4 and c[2] == 50 and c[0] == 16)
    _, _, start = K.restated_act(case)
    _check_bad_slots(lambda slot0: _launch_act_case(dra, case, start, slot0=slot0), case[4])


# ------------------------------------------------------------------------------------------ the update kernel
OUTS = ("loss_vec", "prio", "weights", "q_next", "target")


def _launch_update(dra, u, ring, idx, hidden, gate, double_q, n_step, beta, discount, padded=False, launches=1, prob=None):
    """dra_rainbow_mlp_update on host arrays -> per launch dict(loss, loss_vec, prio, weights, q_next, target, grads by name, gaps:
    the gradient buffer outside the sixteen tensors, err, rc)."""
    from deeprl_amd import rainbow_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    spec, params = u["spec"], u["params"]
    n = spec["n"]
    net, keep, offs = _net_struct(params, u["target_params"], [u["noise"]], u["target_noise"], dev, spec, hidden, gate, padded)
    cap, b = ring["actions"].shape[0], len(idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frames, actions, rewards, masks = t(ring["frames"]), t(ring["actions"]), t(ring["rewards"]), t(ring["masks"])
    idx_t = t(np.asarray(idx, dtype=np.int64)) if b else torch.zeros(1, dtype=torch.int64, device=dev)
    prob = u["prob"] if prob is None else prob
    prob_t = t(np.asarray(prob, dtype=np.float32)) if b else torch.ones(1, dtype=torch.float32, device=dev)
    beta_t = torch.full((1,), beta, dtype=torch.float32, device=dev)
    bb = max(b, 1)
    shapes = dict(loss=(1,), loss_vec=(bb,), prio=(bb,), weights=(bb,), q_next=(bb, 2), target=(bb, max(n, 1)))
    outs = []
    for _ in range(launches):
        grad_full, grad = _guarded((keep[0].numel(),), torch.float32, dev, float("nan"))
        bufs = {k: _guarded(s, torch.float32, dev, float("nan")) for k, s in shapes.items()}
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        io = rainbow_mlp.UpdateIO()
        io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = frames.data_ptr(), actions.data_ptr(), rewards.data_ptr(), masks.data_ptr()
        io.idx, io.prob, io.beta, io.grad = idx_t.data_ptr(), prob_t.data_ptr(), beta_t.data_ptr(), grad.data_ptr()
        io.out_loss, io.out_loss_vec = bufs["loss"][1].data_ptr(), bufs["loss_vec"][1].data_ptr()
        io.out_prio, io.out_weights = bufs["prio"][1].data_ptr(), bufs["weights"][1].data_ptr()
        io.out_q_next, io.out_target = bufs["q_next"][1].data_ptr(), bufs["target"][1].data_ptr()
        io.err, io.capacity, io.discount, io.step_discount = err.data_ptr(), cap, discount ** n_step, discount
        io.replay_eps, io.replay_alpha, io.batch, io.double_q, io.n_step = K.REPLAY_EPS, K.REPLAY_ALPHA, b, int(double_q), n_step
        before = [x.cpu().numpy().copy() for x in keep]
        rc = lib.dra_rainbow_mlp_update.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(x.cpu().numpy()), _bits(y)) for x, y in zip(keep, before))
        g = grad_full.cpu().numpy()
        covered = np.zeros(g.size, dtype=bool)
        grads = {}
        for k in R.KEYS:
            size = int(np.asarray(params[k]).size)
            grads[k] = g[offs[k]:offs[k] + size].reshape(np.asarray(params[k]).shape)
            covered[offs[k]:offs[k] + size] = True
        for k, s in shapes.items():
            assert torch.isnan(bufs[k][0][int(np.prod(s)):]).all(), k
        one = dict(rc=rc, loss=float(bufs["loss"][1].item()), grads=grads, gaps=g[~covered], err=int(err.item()))
        one.update({k: bufs[k][1].cpu().numpy() for k in OUTS})
        outs.append(one)
    return outs


def _fractions(got, want, what):
    f = dict(loss=_fraction(np.asarray([got["loss"]]), np.asarray([want["loss"]]), what + " loss"),
             grads=max(_fraction(got["grads"][k], want["grads"][k], what + " d" + k) for k in R.KEYS))
    f.update({k: _fraction(got[k], want[k], what + " " + k) for k in OUTS})
    return f


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_kernel_matches_restatement(dra, case):
    """dra_rainbow_mlp_update against the fp64 restatement on the case's ring, DATA indices, sampling probabilities, parameters and
    noise (the target's of both from other seeds): loss, loss_vec, prio, weights, q_next, target and the sixteen gradients within
    1e-5 of scale; every element of the sixteen tensors written and nothing between or behind them (the parameters and the noise
    vectors lie behind gaps of NaN in the cases of 17 rows); the error word 0; the parameter and noise buffers unchanged; two
    launches give the same bits."""
    n, hidden, gate, batch, double_q, kind, n_step, beta, discount, _ = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    padded = K.update_padded(case)
    a, b = _launch_update(dra, u, rg["ring"], u["idx"], hidden, gate, double_q, n_step, beta, discount, padded, launches=2)
    assert a["rc"] == 0 and a["err"] == 0
    what = K.update_id(case)
    worst = _fractions(a, u, what)
    record_parity("rainbow_mlp update kernel vs restatement %s (fraction of the bar)" % what, **worst)
    for k, f in worst.items():
        assert f <= 1.0, (what, k, f)
    assert np.isnan(a["gaps"]).all() and a["gaps"].size == GUARD + (_pad_floats(u["params"]) if padded else 0)
    assert all(np.isfinite(a["grads"][k]).all() for k in R.KEYS)
    for k in OUTS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["loss"] == b["loss"] and all(np.array_equal(_bits(a["grads"][k]), _bits(b["grads"][k])) for k in R.KEYS)


def _module_update(dra, u, ring, idx, hidden, gate, double_q, n_step, beta, discount):
    """The module form of the update on a kernel case: RainbowNet modules holding the case's parameters and noise, the n-step
    minibatch, ops.per_weights_dev, ops.c51_loss, autograd -> dict(loss, loss_vec, prio, weights, grads by name)."""
    from deeprl_amd import ops
    d, dev = dra, dra.Config.DEVICE
    spec, n = u["spec"], u["spec"]["n"]
    fn = {"relu": torch.relu, "tanh": torch.tanh}[gate]

    def make(params, noise):
        net = d.RainbowNet(2, n, d.FCBody(4, hidden_units=(hidden, hidden), gate=fn, noisy_linear=True), noisy_linear=True)
        net.load_state_dict({k: torch.from_numpy(np.asarray(params[k])) for k in R.KEYS}, strict=False)
        block = net.noise_block()
        for (layer, name), (o, size) in block.slices.items():
            block.flat[o:o + size].copy_(torch.from_numpy(noise["%s.%s" % (layer, name)]))
        for _, m in block.layers:
            m.noise_changed()
        return net
    net = make(u["params"], u["noise"])
    tnet = make(u["target_params"] if u["target_params"] is not None else u["params"],
                u["target_noise"] if u["target_noise"] is not None else u["noise"])
    mb = R.minibatch(ring, idx, n_step, discount)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    states, nxt, action, reward, mask = t(mb["state"]), t(mb["next_state"]), t(mb["action"]), t(mb["reward"]), t(mb["mask"])
    prob, beta_t = t(np.asarray(u["prob"], dtype=np.float32)), torch.full((1,), beta, dtype=torch.float32, device=dev)
    with torch.no_grad():
        logits_t = tnet(nxt)['logits']
        logits_o = net(nxt)['logits'] if double_q else None
    logits = net(states)['logits']
    _, w = ops.per_weights_dev(None, prob, beta_t, K.REPLAY_EPS, K.REPLAY_ALPHA)
    out = ops.c51_loss(logits.detach().contiguous(), logits_t.contiguous(), action, reward, mask, discount ** n_step,
                       t(R.atoms(spec)), spec["v_min"], spec["v_max"], logits_next_online=logits_o, weights=w)
    prio, _ = ops.per_weights_dev(out['kl'], prob, beta_t, K.REPLAY_EPS, K.REPLAY_ALPHA)
    logits.backward(out['dlogits'])
    grads = {k: p.grad.cpu().numpy() for k, p in net.named_parameters() if k in R.KEYS}
    return dict(loss=float(out['loss'].item()), loss_vec=out['kl'].cpu().numpy(), prio=prio.cpu().numpy(), weights=w.cpu().numpy(),
                grads=grads)


MODULE_QUANTITIES = ("loss", "loss_vec", "prio", "weights", "grads")


def test_module_path_fractions_next_to_the_kernels(dra):
    """The module form of the update (what config.fused_rainbow_update = False runs) in fp32 against the fp64 restatement on the
    kernel's own relu cases of at most 17 rows (csrc/noisy.hip folds no tanh into a noisy layer), next to the kernel's fractions of the 1e-5-of-scale bar.  The issue's rule: where the
    module path itself exceeds the bar, a quantity's bar is twice the module path's fraction -- here the kernel stays within
    max(1, twice the module path's fraction) for every quantity, and both worst fractions are recorded."""
    worst_k, worst_m = dict.fromkeys(MODULE_QUANTITIES, 0.0), dict.fromkeys(MODULE_QUANTITIES, 0.0)
    cases = [c for c in K.UPDATE_CASES if c[3] <= 17 and c[2] == "relu" and not K.update_padded(c)]
    assert len(cases) >= 8 and {c[0] for c in cases} == {2, 50, 51} and {c[6] for c in cases} >= {1, 3}
    for case in cases:
        n, hidden, gate, batch, double_q, kind, n_step, beta, discount, _ = case
        u, rg = K.restated_update(case), K.make_ring(kind)
        what = K.update_id(case)
        got, = _launch_update(dra, u, rg["ring"], u["idx"], hidden, gate, double_q, n_step, beta, discount)
        mod = _module_update(dra, u, rg["ring"], u["idx"], hidden, gate, double_q, n_step, beta, discount)
        for name, have, worst in (("kernel", got, worst_k), ("modules", mod, worst_m)):
            f = dict(loss=_fraction(np.asarray([have["loss"]]), np.asarray([u["loss"]]), "%s %s loss" % (name, what)),
                     grads=max(_fraction(have["grads"][k], u["grads"][k], "%s %s d%s" % (name, what, k)) for k in R.KEYS))
            f.update({k: _fraction(have[k], u[k], "%s %s %s" % (name, what, k)) for k in ("loss_vec", "prio", "weights")})
            for k, v in f.items():
                worst[k] = max(worst[k], v)
    print("kernel", worst_k, "modules", worst_m)
    record_parity("rainbow_mlp update: the kernel's worst fractions of the bar", **worst_k)
    record_parity("rainbow_mlp update: the module path's worst fractions of the bar", **worst_m)
    for k in MODULE_QUANTITIES:
        assert worst_k[k] <= max(1.0, 2.0 * worst_m[k]), (k, worst_k[k], worst_m[k])


STEPS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rainbow_feature", "steps.npz")


@pytest.mark.parametrize("tag", [t[0] for t in K.FIXTURE_TAGS])
def test_update_kernel_reproduces_the_recorded_agent_steps(dra, tag):
    """dra_rainbow_mlp_update against the reference's own CategoricalDQNAgent (tests/golden/rainbow_feature/steps.npz) at every
    recorded update: launched on the parameters the reference had before the step, the target's, both recorded noise draws, the
    ring as it stood, the leaves' data indices, the sampling probabilities and beta, the KL vector and the priorities land
    within rtol 2e-5 / atol 2e-6 of the reference's, and so do the parameters behind the step -- the kernel's gradient through
    clip_grad_norm_ and RMSprop in fp64, the running averages carried from the kernel's own gradients."""
    from nstep_feature_restatement import rmsprop_step
    z = np.load(STEPS, allow_pickle=False)
    f = K.FIXTURE
    spec = next(t for t in K.FIXTURE_TAGS if t[0] == tag)
    within = lambda a, w: float((np.abs(np.asarray(a, dtype=np.float64) - w) / (2e-6 + 2e-5 * np.abs(w))).max())
    sq, worst = None, dict(kl=0.0, prio=0.0, params=0.0)
    for u in K.fixture_updates(z, tag):
        got, = _launch_update(dra, u, u["ring"], u["idx"], spec[5], "relu", spec[3], f["n_step"], u["beta"], K.DISCOUNT)
        assert got["rc"] == 0 and got["err"] == 0
        worst["kl"] = max(worst["kl"], within(got["loss_vec"], u["kl"]))
        worst["prio"] = max(worst["prio"], within(got["prio"], u["prio"]))
        grads = {k: got["grads"][k].astype(np.float64) for k in R.KEYS}
        new, sq = rmsprop_step(u["params"], grads, f["gradient_clip"], f["lr"], square_avg=sq)
        worst["params"] = max(worst["params"], max(within(new[k], u["after"][k]) for k in R.KEYS))
    print(tag, worst)
    record_parity("rainbow_mlp update kernel vs the reference's recorded steps %s (fraction of rtol 2e-5 / atol 2e-6)" % tag, **worst)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_update_reads_beta_from_the_device(dra):
    """beta is read from a device word: launches that differ in it alone give that beta's weights, and the same KL and priorities
    to the bit."""
    case = next(c for c in K.UPDATE_CASES if c[3] == 15 and c[0] == 50)
    n, hidden, gate, batch, double_q, kind, n_step, beta, discount, _ = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    a, = _launch_update(dra, u, rg["ring"], u["idx"], hidden, gate, double_q, n_step, 0.4, discount)
    b, = _launch_update(dra, u, rg["ring"], u["idx"], hidden, gate, double_q, n_step, 1.0, discount)
    w = lambda be: (u["prob"].astype(np.float64) * batch + 1e-6) ** -be
    assert _fraction(a["weights"], w(0.4) / w(0.4).max(), "weights beta 0.4") <= 1.0
    assert _fraction(b["weights"], w(1.0) / w(1.0).max(), "weights beta 1") <= 1.0
    assert np.array_equal(_bits(a["loss_vec"]), _bits(b["loss_vec"])) and np.array_equal(_bits(a["prio"]), _bits(b["prio"]))


def test_update_clamps_and_counts_indices_outside_the_ring(dra):
    """Staged indices outside [0, capacity - 1 - n_step] are clamped into it and counted in the error word: the launch computes what
    it computes on the clamped indices, bit for bit, and reads nothing outside the ring."""
    case = next(c for c in K.UPDATE_CASES if c[3] == 15 and c[0] == 50)
    n, hidden, gate, batch, double_q, kind, n_step, beta, discount, _ = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    cap = rg["ring"]["actions"].shape[0]
    bad = u["idx"].copy()
    bad[4], bad[5], bad[6], bad[7] = -3, cap - n_step, cap + 7, cap - 1 - n_step      # (the last one is the last slot allowed)
    clamped = np.clip(bad, 0, cap - 1 - n_step)
    ring = {k: v.copy() for k, v in rg["ring"].items()}
    ring["frames"][rg["size"]:], ring["rewards"][rg["size"]:], ring["masks"][rg["size"]:], ring["actions"][rg["size"]:] = 0.25, 1.0, 1, 0
    args = (hidden, gate, double_q, n_step, beta, discount)
    got, = _launch_update(dra, u, ring, bad, *args)
    want, = _launch_update(dra, u, ring, clamped, *args)
    assert got["rc"] == want["rc"] == 0 and got["err"] == 3 and want["err"] == 0
    for k in OUTS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert got["loss"] == want["loss"] and np.isfinite(got["loss"])
    assert all(np.array_equal(_bits(got["grads"][k]), _bits(want["grads"][k])) for k in R.KEYS)


def test_supported_agrees_with_the_launches(dra):
    """dra_rainbow_mlp_supported / dra_rainbow_mlp_update_supported say what the launches accept: over atoms {1, 2, 51, 52} x hidden
    {8, 16, 64, 128} x [batch {0, 1, 64, 65 (what the LDS no longer holds)} x n_step {0, 3, 8, 9} | transitions {0, 8, 9}] the
    return code is 0 exactly where the table says yes."""
    from deeprl_amd import rainbow_mlp
    rg = K.make_ring("partial")
    ring = {k: v.copy() for k, v in rg["ring"].items()}
    ring["frames"][rg["size"]:], ring["rewards"][rg["size"]:], ring["masks"][rg["size"]:], ring["actions"][rg["size"]:] = 0.25, 1.0, 1, 0
    env, raw = K.make_env(K.ENV_SEED, 200)
    yes = 0
    for n in (1, 2, K.MAX_ATOMS, K.MAX_ATOMS + 1):
        spec = K.spec_of(n, (-10.0, 10.0))
        for hidden in (8, 16, 64, 128):
            params, z = R.init_params(hidden, 5, n), R.draw_noise(hidden, n, 6)
            u = dict(spec=spec, params=params, target_params=params, noise=z, target_noise=z)
            for batch in (0, 1, K.MAX_B, K.MAX_B + 1):
                idx = np.arange(batch, dtype=np.int64) % 200
                prob = np.full(batch, 0.01, dtype=np.float32)
                for n_step in (0, 3, K.MAX_N_STEP, K.MAX_N_STEP + 1):
                    got, = _launch_update(dra, u, ring, idx, hidden, "relu", True, n_step, 0.4, K.DISCOUNT, prob=prob)
                    want = rainbow_mlp.update_supported(4, 2, hidden, batch, 1, n, n_step)
                    assert (got["rc"] == 0) == want and got["rc"] in (0, -22), (n, hidden, batch, n_step, got["rc"])
                    assert want == (2 <= n <= K.MAX_ATOMS and hidden in (16, 64) and 1 <= batch <= K.MAX_B and 1 <= n_step <= K.MAX_N_STEP)
                    yes += want
            for k_len in (0, 8, 9):
                start = dict(params=params, noise_rows=[z], raw=raw.copy(), seed=env.seed, explore=np.zeros(8, dtype=bool),
                             random_action=np.zeros(8, dtype=np.int64), spec=spec)
                got = _launch_act(dra, start, hidden, "relu", k_len, 64, 0, 200, False)
                want = rainbow_mlp.supported(4, 2, hidden, k_len, 1, n)
                assert (got["rc"] == 0) == want and got["rc"] in (0, -22), (n, hidden, k_len, got["rc"])
                assert want == (2 <= n <= K.MAX_ATOMS and hidden in (16, 64) and k_len == 8)
                yes += want
    assert yes == 2 * 2 * 2 * 2 + 2 * 2
