"""GPU tests of n_step_dqn_feature on device-resident cart-pole environments: the rollout and the update kernel of csrc/q_mlp.hip
against the restatement (tests/nstep_feature_restatement.py, pinned to the reference's own run by
tests/test_nstep_feature_host.py, which also asserts the Q margins and relu pre-activation margins these comparisons rest on),
the update kernel against the module path and against the reference's recorded NStepDQNAgent.step, NStepDQNAgent's device path
against the host-stepped path, graph replay against eager, save / load, and a closed loop that has to LEARN.
Bars: exact for everything the fp64 environment determines once the actions are equal (observations, states, counters, masks,
ring rows); 1e-5 of a tensor's largest magnitude (floor 1) for fp32 values."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from feature_kernel_harness import (      # noqa: F401  (dra: the fixture)
    GAME, GATE, GUARD, dra, _Rec, _fraction, _within, _bits, _as_int, _guarded, _flat, _tails_intact, _body, _line_events)
from parity_log import record_parity

import nstep_feature_cases as K
import nstep_feature_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nstep_feature")
FIXTURE = os.path.join(GOLDEN, "nstep_feature_step.npz")


def _net_struct(params, target, dev, hidden, gate, padded):
    from deeprl_amd import q_mlp
    flat, offs = _flat(R.KEYS, params, padded)
    tflat, _ = _flat(R.KEYS, target if target is not None else params, padded)
    flat, tflat = torch.from_numpy(flat).to(dev), torch.from_numpy(tflat).to(dev)
    net = q_mlp.Net()
    net.param, net.target = flat.data_ptr(), tflat.data_ptr()
    net.w1, net.b1, net.w2, net.b2, net.wq, net.bq = [offs[k] for k in R.KEYS]
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, hidden, GATE[gate]
    return net, flat, tflat, offs


# ------------------------------------------------------------------------------------------ rollout kernel
def _launch(dra, case, start):
    """One dra_q_mlp_rollout from the case's start -> dict of host arrays (guards included) and the return code."""
    from deeprl_amd import q_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    hidden, gate, n, t_len, horizon, padded = case[:6]
    net, flat, tflat, _ = _net_struct(start["params"], start["target"], dev, hidden, gate, padded)
    nan = float("nan")
    spec = dict(env_state=((n, 4), torch.float64, nan), env_counter=((n,), torch.int64, -7), ep_steps=((n,), torch.int32, -7),
                ep_return=((n,), torch.float64, nan), env_seed=((n,), torch.int64, -7), step=((1,), torch.int64, -7),
                ep_count=((1,), torch.int64, -7), ep_ring=((K.RING_CAP, 3), torch.float64, nan),
                explore=((t_len, n), torch.uint8, 9), random_action=((t_len, n), torch.int64, -7),
                state=((t_len, n, 4), torch.float32, nan), q=((t_len, n, 2), torch.float32, nan), action=((t_len, n), torch.int64, -7),
                reward=((t_len, n), torch.float32, nan), mask=((t_len, n), torch.float32, nan), bootstrap=((n,), torch.float32, nan))
    full, view = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], view[k] = _guarded(shape, dt, dev, fill)
    view["env_state"].copy_(torch.from_numpy(start["raw"]))
    view["env_counter"].zero_(); view["ep_steps"].zero_(); view["ep_return"].zero_()
    view["env_seed"].copy_(torch.tensor(start["seeds"], dtype=torch.int64))
    view["step"].fill_(K.STEP0); view["ep_count"].fill_(K.RING_COUNT0)
    view["explore"].copy_(torch.from_numpy(start["explore"].astype(np.uint8)))
    view["random_action"].copy_(torch.from_numpy(start["random_action"]))
    io = q_mlp.RolloutIO()
    io.env_state, io.env_counter, io.ep_steps = view["env_state"].data_ptr(), view["env_counter"].data_ptr(), view["ep_steps"].data_ptr()
    io.ep_return, io.env_seed, io.step_counter = view["ep_return"].data_ptr(), view["env_seed"].data_ptr(), view["step"].data_ptr()
    io.ep_count, io.ep_ring = view["ep_count"].data_ptr(), view["ep_ring"].data_ptr()
    io.explore, io.random_action = view["explore"].data_ptr(), view["random_action"].data_ptr()
    io.out_state, io.out_q, io.out_action = view["state"].data_ptr(), view["q"].data_ptr(), view["action"].data_ptr()
    io.out_reward, io.out_mask, io.bootstrap = view["reward"].data_ptr(), view["mask"].data_ptr(), view["bootstrap"].data_ptr()
    io.horizon, io.ring_cap, io.reward_coef, io.t_len, io.n_env = horizon, K.RING_CAP, 1.0, t_len, n
    before = flat.cpu().numpy().copy(), tflat.cpu().numpy().copy()
    rc = lib.dra_q_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in full.items()}
    out["rc"], out["spec"] = rc, spec
    # (both parameter buffers are read only)
    assert np.array_equal(_bits(flat.cpu().numpy()), _bits(before[0])) and np.array_equal(_bits(tflat.cpu().numpy()), _bits(before[1]))
    return out, (net, io, full, view, flat, tflat)


@pytest.mark.parametrize("case", K.ROLLOUT_CASES, ids=K.case_id)
def test_rollout_kernel_matches_restatement(dra, case):
    """dra_q_mlp_rollout against the restatement: actions equal (the host suite asserts a Q margin >= 1e-4 at every greedy pair of
    every case); stored observations, final environment state, counters, episode steps and returns, rewards, masks, the step
    counter and the ring's rows and count equal to the bit; q and the TARGET network's bootstrap within 1e-5 of scale; the guard
    elements behind every buffer untouched; both parameter buffers unchanged; a second launch from the same start gives the same
    bits everywhere."""
    hidden, gate, n, t_len, horizon, padded = case[:6]
    want, envs, start = K.restated_rollout(case)
    out, _ = _launch(dra, case, start)
    assert out["rc"] == 0
    assert np.array_equal(_body(out, "action"), want["action"])
    assert np.array_equal(_bits(_body(out, "state")), _bits(want["state"]))
    assert np.array_equal(_bits(_body(out, "env_state")), _bits(want["raw_states"]))
    assert np.array_equal(_body(out, "env_counter"), [e.c for e in envs])
    assert np.array_equal(_body(out, "ep_steps"), [e.steps for e in envs])
    assert np.array_equal(_bits(_body(out, "ep_return")), _bits(np.asarray([e.ret for e in envs])))
    assert np.array_equal(_bits(_body(out, "reward")), _bits(want["reward"])) and np.array_equal(_bits(_body(out, "mask")), _bits(want["mask"]))
    assert int(_body(out, "step")[0]) == K.STEP0 + t_len
    assert int(_body(out, "ep_count")[0]) == K.RING_COUNT0 + len(want["events"])
    ring = np.full((K.RING_CAP, 3), np.nan)
    for i, ev in enumerate(want["events"]):
        ring[(K.RING_COUNT0 + i) % K.RING_CAP] = ev
    assert np.array_equal(_bits(_body(out, "ep_ring")), _bits(ring))
    eq = _within(_body(out, "q"), want["q"], "q")
    eb = _within(_body(out, "bootstrap"), want["bootstrap"], "bootstrap")
    record_parity("q_mlp rollout kernel vs restatement %s (fraction of the bar)" % K.case_id(case), q=eq, bootstrap=eb)
    _tails_intact(out)
    again, _ = _launch(dra, case, start)
    for k in out["spec"]:
        assert np.array_equal(_bits(out[k]), _bits(again[k])), k


def test_rollout_refuses_unsupported_shapes_and_launches_nothing(dra):
    from deeprl_amd import q_mlp
    from deeprl_amd._lib import lib, stream_ptr
    case = K.ROLLOUT_CASES[0]
    _, _, start = K.restated_rollout(case)
    out, (net, io, full, view, flat, tflat) = _launch(dra, case, start)
    before = {k: v.clone() for k, v in full.items()}

    def refused(**change):
        n2, io2 = q_mlp.Net.from_buffer_copy(net), q_mlp.RolloutIO.from_buffer_copy(io)
        for k, v in change.items():
            setattr(n2 if hasattr(n2, k) else io2, k, v)
        rc = lib.dra_q_mlp_rollout.raw(ctypes.byref(n2), ctypes.byref(io2), stream_ptr())
        torch.cuda.synchronize()
        return rc == -22 and all(torch.equal(_as_int(before[k]), _as_int(full[k])) for k in full)

    assert refused(hidden=48) and refused(hidden=128) and refused(state_dim=5) and refused(n_actions=3) and refused(gate=3)
    assert refused(n_env=0) and refused(n_env=65) and refused(t_len=0) and refused(horizon=0) and refused(ring_cap=0)
    assert refused(w2=-1) and refused(bq=-4)
    assert refused(out_q=None) and refused(bootstrap=None) and refused(explore=None) and refused(target=None)


CORE_CASES = [      # (n_env, t_len, horizon, ring_cap)
    (1, 1, 200, 64),        # one lane, no episode end
    (64, 3, 2, 4096),       # every lane of the wave, 64 ends in one step: the ballot rank at lane 63
    (5, 6, 2, 8),           # 15 rows through an 8-row ring (5 a step: never more ends in one step than the ring has rows)
]


@pytest.mark.parametrize("gate", ["relu", "tanh"])
@pytest.mark.parametrize("n,t_len,horizon,ring_cap", CORE_CASES, ids=lambda v: str(v))
def test_rollout_cores_agree(dra, n, t_len, horizon, ring_cap, gate):
    """dra_cat_mlp_rollout and dra_q_mlp_rollout share csrc/cartpole_rollout.h: from the same environments, with the second
    launch made to take the actions the first one stored (explore all ones), everything the shared text computes is the same
    bits -- the environments' arrays, the stored observations, rewards and masks, the ring's count and columns 1 and 2 of every
    row; column 0 differs by the two starting stamps alone.  Hidden 16, both gates."""
    from deeprl_amd import cat_mlp, q_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev, hidden = dra.Config.DEVICE, 16
    rng = np.random.RandomState(1000 * n + t_len)
    shapes = dict(w1=(hidden, 4), b1=(hidden,), w2=(hidden, hidden), b2=(hidden,))
    cat_keys, q_keys = dict(shapes, wa=(2, hidden), ba=(2,), wc=(1, hidden), bc=(1,)), dict(shapes, wq=(2, hidden), bq=(2,))
    stamp_cat, stamp_q, count0 = 1000, 70, 3

    def flat_net(struct, keys):
        off, chunks = 0, []
        for k, shape in keys.items():
            setattr(struct, k, off)
            chunks.append(rng.uniform(-0.5, 0.5, size=shape).astype(np.float32).reshape(-1))
            off += chunks[-1].size
        struct.state_dim, struct.n_actions, struct.hidden, struct.gate = 4, 2, hidden, GATE[gate]
        return torch.from_numpy(np.concatenate(chunks)).to(dev)

    start = dict(env_state=torch.from_numpy(rng.uniform(-0.05, 0.05, size=(n, 4))), env_counter=torch.arange(n, dtype=torch.int64) * 3,
                 ep_steps=torch.zeros(n, dtype=torch.int32), ep_return=torch.zeros(n, dtype=torch.float64),
                 env_seed=torch.arange(n, dtype=torch.int64) + 11, ep_count=torch.full((1,), count0, dtype=torch.int64),
                 ep_ring=torch.full((ring_cap, 3), float("nan"), dtype=torch.float64))
    f32 = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)

    def side(io, stamp):
        t = {k: v.clone().to(dev) for k, v in start.items()}
        t.update(state=f32(t_len, n, 4), action=torch.full((t_len, n), -7, dtype=torch.int64, device=dev), reward=f32(t_len, n),
                 mask=f32(t_len, n), stamp=torch.full((1,), stamp, dtype=torch.int64, device=dev))
        for k in start:
            setattr(io, k, t[k].data_ptr())
        for k in ("state", "action", "reward", "mask"):
            setattr(io, "out_" + k, t[k].data_ptr())
        io.horizon, io.ring_cap, io.reward_coef, io.t_len, io.n_env = horizon, ring_cap, 1.0, t_len, n
        return t

    cnet, cio = cat_mlp.Net(), cat_mlp.RolloutIO()
    cflat = flat_net(cnet, cat_keys)
    cnet.param = cflat.data_ptr()
    c = side(cio, stamp_cat)
    c["v"] = f32(t_len + 1, n)
    cio.sampler_step, cio.out_v, cio.env0, cio.n_global, cio.noise_seed = c["stamp"].data_ptr(), c["v"].data_ptr(), 0, n, 12345
    assert lib.dra_cat_mlp_rollout.raw(ctypes.byref(cnet), ctypes.byref(cio), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(((c["action"] == 0) | (c["action"] == 1)).all())

    qnet, qio = q_mlp.Net(), q_mlp.RolloutIO()
    qflat = flat_net(qnet, q_keys)
    qnet.param = qnet.target = qflat.data_ptr()
    q = side(qio, stamp_q)
    q.update(q=f32(t_len, n, 2), bootstrap=f32(n), explore=torch.ones((t_len, n), dtype=torch.uint8, device=dev),
             random_action=c["action"].clone())
    qio.step_counter, qio.out_q, qio.bootstrap = q["stamp"].data_ptr(), q["q"].data_ptr(), q["bootstrap"].data_ptr()
    qio.explore, qio.random_action = q["explore"].data_ptr(), q["random_action"].data_ptr()
    assert lib.dra_q_mlp_rollout.raw(ctypes.byref(qnet), ctypes.byref(qio), stream_ptr()) == 0
    torch.cuda.synchronize()

    for k in ("env_state", "env_counter", "ep_steps", "ep_return", "state", "action", "reward", "mask", "ep_count"):
        assert torch.equal(_as_int(c[k]), _as_int(q[k])), k
    assert int(c["stamp"].item()) == stamp_cat + t_len + 1 and int(q["stamp"].item()) == stamp_q + t_len
    ends = sum(1 for t in range(t_len) if (t + 1) % horizon == 0) * n         # (no pole falls within `horizon` steps of such a start)
    assert int(c["ep_count"].item()) == count0 + ends and float((1 - c["mask"]).sum().item()) == ends
    cr, qr = c["ep_ring"].cpu().numpy(), q["ep_ring"].cpu().numpy()
    assert np.array_equal(_bits(cr[:, 1:]), _bits(qr[:, 1:]))
    written = ~np.isnan(cr[:, 0])
    assert written.sum() == min(ends, ring_cap) and np.array_equal(written, ~np.isnan(qr[:, 0]))
    assert np.array_equal(cr[written, 0] - stamp_cat, qr[written, 0] - stamp_q)
    assert np.array_equal(np.isnan(cr[:, 1]), ~written) and (cr[written, 2] == horizon).all()


# ------------------------------------------------------------------------------------------ update kernel
SENTINEL = 123.25       # what the gaps of the gradient buffer hold before a launch


def _launch_update(dra, case, padded, rows_override=None):
    """One dra_q_mlp_update on the case's inputs -> (dict of host arrays, rc, handles)."""
    from deeprl_amd import q_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    hidden, gate, n, t_len = case[:4]
    u = K.restated_update(case)
    net, flat, _, offs = _net_struct(u["params"], None, dev, hidden, gate, padded)
    net.target = None          # (the update does not read it)
    grad_full, grad = _guarded((flat.numel(),), torch.float32, dev, SENTINEL)
    grad.fill_(SENTINEL)
    nan = float("nan")
    spec = dict(ret=((t_len, n), torch.float32, nan), loss=((1,), torch.float32, nan))
    full, view = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], view[k] = _guarded(shape, dt, dev, fill)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    inp = {k: up(v) for k, v in u["inputs"].items()}
    io = q_mlp.UpdateIO()
    io.state, io.action, io.reward, io.mask = [inp[k].data_ptr() for k in ("state", "action", "reward", "mask")]
    io.bootstrap, io.grad, io.out_ret, io.out_loss = inp["bootstrap"].data_ptr(), grad.data_ptr(), view["ret"].data_ptr(), view["loss"].data_ptr()
    io.discount, io.t_len, io.n_env = K.DISCOUNT, t_len if rows_override is None else rows_override, n
    flat_before = flat.cpu().numpy().copy()
    rc = lib.dra_q_mlp_update.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(flat.cpu().numpy()), _bits(flat_before))        # NaN gaps included: the parameters are read only
    out = {k: v.cpu().numpy() for k, v in full.items()}
    out["spec"], out["grad_full"] = spec, grad_full.cpu().numpy()
    return out, rc, (offs, inp, flat)


def _module_grads(dra, case):
    """The module path's fp32 autograd on the same inputs -> {key: gradient} (what fused_nstep_update=False computes)."""
    import torch.nn.functional as F
    d = dra
    hidden, gate, n, t_len = case[:4]
    u = K.restated_update(case)
    net = d.VanillaNet(2, d.FCBody(4, (hidden, hidden), gate=F.relu if gate == "relu" else torch.tanh))
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in u["params"].items()})
    dev = d.Config.DEVICE
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ret = up(R.returns(u["inputs"]["reward"], u["inputs"]["mask"], u["inputs"]["bootstrap"], K.DISCOUNT, dtype=np.float32))
    q_a = net(up(u["inputs"]["state"]).view(t_len * n, 4))['q'].gather(1, up(u["inputs"]["action"]).view(-1, 1))
    for p in net.parameters():
        p.grad = None
    q_a.backward((q_a.detach() - ret.view(-1, 1)) / (t_len * n))
    torch.cuda.synchronize()
    return {k: p.grad.cpu().numpy() for k, p in net.named_parameters()}


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_kernel_matches_restatement(dra, case, padded):
    """dra_q_mlp_update against the fp64 restatement: ret, loss and each of the six gradient tensors within 1e-5 of its fp64
    counterpart's largest magnitude (floor 1); the measured fraction of that bar is recorded next to the fraction the module
    path's fp32 autograd reaches on the same case.  In the one-action case the head's other row and bias entry are exactly 0.0.
    Padded layout: the NaN gaps of the parameter buffer and the sentinel in the gaps of the gradient buffer survive.  Two
    launches give the same bits."""
    hidden, gate, n, t_len, horizon, force_zero = case[:6]
    u = K.restated_update(case)
    out, rc, (offs, _, flat) = _launch_update(dra, case, padded)
    assert rc == 0
    fr = dict(ret=_within(_body(out, "ret"), u["ret"], "ret"), loss=_within(_body(out, "loss"), np.asarray([u["loss"]]), "loss"))
    # the returns are the reference's fp32 scan, bit for bit
    ret32 = R.returns(u["inputs"]["reward"], u["inputs"]["mask"], u["inputs"]["bootstrap"], K.DISCOUNT, dtype=np.float32)
    assert np.array_equal(_bits(_body(out, "ret")), _bits(ret32))
    g = out["grad_full"]
    covered = np.zeros(g.size, dtype=bool)
    covered[-GUARD:] = False
    module = _module_grads(dra, case)
    mod_fr = {}
    for k in R.KEYS:
        want = u["grads"][k]
        got = g[offs[k]:offs[k] + want.size].reshape(want.shape)
        covered[offs[k]:offs[k] + want.size] = True
        fr[k] = _fraction(got, want, k)
        mod_fr[k] = _fraction(module[k], want, "module path " + k)
    record_parity("q_mlp update kernel vs restatement %s %s (fraction of the bar)" % (K.update_id(case), "padded" if padded else "packed"),
                  **{k.replace(".", "_"): v for k, v in fr.items()})
    record_parity("module path fp32 autograd vs restatement %s (fraction of the bar)" % K.update_id(case),
                  **{k.replace(".", "_"): v for k, v in mod_fr.items()})
    for k in R.KEYS:
        assert fr[k] <= 1.0, (k, fr[k])
    # everything that is not one of the six tensors keeps the sentinel: the gaps (padded) and the guard behind the buffer
    assert (g[~covered] == SENTINEL).all() and (~covered).sum() == GUARD + (flat.numel() - sum(u["grads"][k].size for k in R.KEYS))
    if padded:
        assert np.isnan(flat.cpu().numpy()).sum() == flat.numel() - sum(u["grads"][k].size for k in R.KEYS) > 0
    if force_zero:
        wq = g[offs["fc_head.weight"]:offs["fc_head.weight"] + 2 * hidden].reshape(2, hidden)
        assert (wq[1] == 0.0).all() and g[offs["fc_head.bias"] + 1] == 0.0 and np.abs(wq[0]).max() > 1e-3
    _tails_intact(out)
    again, rc2, _ = _launch_update(dra, case, padded)
    assert rc2 == 0 and np.array_equal(_bits(again["grad_full"]), _bits(g))
    for k in out["spec"]:
        assert np.array_equal(_bits(out[k]), _bits(again[k])), k


def test_update_refuses_rows_above_the_cap_and_writes_nothing(dra):
    """64 environments x 17 steps = 1088 rows: DRA_EINVAL, the gradient buffer and the outputs keep their sentinels.  (The kernel
    would read 17 steps of inputs: the refusal comes before any launch, so the case's 16 are never overrun.)"""
    case = K.UPDATE_CASES[4]
    assert case[2] * case[3] == K.UPDATE_CAP
    out, rc, _ = _launch_update(dra, case, False, rows_override=case[3] + 1)
    assert rc == -22
    assert (out["grad_full"] == SENTINEL).all() and np.isnan(out["ret"]).all() and np.isnan(out["loss"]).all()


# ------------------------------------------------------------------------------------------ update against module path / reference
def _bare_agent(d, params, target, t_len, n, fused_update, discount=K.DISCOUNT, clip=5, lr=0.001, gate="relu", hidden=64):
    """An NStepDQNAgent with everything _feature_learn's update half reads and nothing else (no task: the rollout is given)."""
    import torch.nn.functional as F
    from deeprl_amd import q_mlp
    from deeprl_amd.optim import FlatParams, FusedOptimizer
    cfg = d.Config()
    cfg.discount, cfg.gradient_clip, cfg.rollout_length, cfg.num_workers = discount, clip, int(t_len), int(n)
    cfg.fused_nstep_feature, cfg.fused_nstep_update = True, fused_update
    agent = d.NStepDQNAgent.__new__(d.NStepDQNAgent)
    agent.config, agent.grad_hook = cfg, None
    mk = lambda: d.VanillaNet(2, d.FCBody(4, (hidden, hidden), gate=F.relu if gate == "relu" else torch.tanh))
    agent.network, agent.target_network = mk(), mk()
    agent.network.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in params.items()})
    agent.target_network.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in target.items()})
    agent.optimizer = torch.optim.RMSprop(agent.network.parameters(), lr)
    agent._fused = FusedOptimizer.adopt(agent.optimizer)
    agent._target_flat = FlatParams(list(agent.target_network.parameters()))
    assert q_mlp.why_not(agent) is None
    agent._feature = q_mlp.Rollout(agent, q_mlp.shape(agent.network))
    return agent


def _apply_update(d, agent, inputs):
    """The update half of NStepDQNAgent._feature_learn on given rollout buffers."""
    dev = d.Config.DEVICE
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_len, n = inputs["action"].shape
    b = dict(state=up(inputs["state"].astype(np.float32)), action=up(inputs["action"].astype(np.int64)),
             reward=up(inputs["reward"].astype(np.float32)), mask=up(inputs["mask"].astype(np.float32)),
             bootstrap=up(np.asarray(inputs["bootstrap"], dtype=np.float32)),
             ret=torch.zeros((t_len, n), dtype=torch.float32, device=dev), loss=torch.zeros(1, dtype=torch.float32, device=dev))
    agent._feature.run = lambda t: b        # (the rollout is given)
    agent._rollout_step = 0
    from deeprl_amd.mlp_rollout import Plan
    loss = agent._feature_learn(Plan(None, t_len))
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()}, float(loss)


@pytest.mark.parametrize("case", [K.UPDATE_CASES[1], K.UPDATE_CASES[2], K.UPDATE_CASES[3]], ids=K.update_id)
def test_fused_update_matches_module_path_on_the_device(dra, case):
    """The same rollout buffers through config.fused_nstep_update True (dra_q_mlp_update) and False (the scan kernel, one module
    forward, autograd): the parameters after _fused.step agree within rtol 2e-5 / atol 2e-6, and so do the two losses."""
    hidden, gate, n, t_len = case[:4]
    u = K.restated_update(case)
    got = {}
    for fused in (True, False):
        agent = _bare_agent(dra, u["params"], u["params"], t_len, n, fused, gate=gate, hidden=hidden)
        got[fused] = _apply_update(dra, agent, u["inputs"])
    worst = 0.0
    for k in got[True][0]:
        a, b = got[True][0][k], got[False][0][k]
        worst = max(worst, float(np.max(np.abs(a - b) / (2e-6 + 2e-5 * np.abs(b)))))
        assert (a != np.asarray(u["params"][k], dtype=np.float32)).any(), k
    record_parity("q_mlp fused update vs module path %s (fraction of the bar)" % K.update_id(case), params=worst)
    for k in got[True][0]:
        np.testing.assert_allclose(got[True][0][k], got[False][0][k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(got[True][1], got[False][1], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(got[True][1], u["loss"], rtol=2e-5, atol=2e-6)


def _fixture_params(g, tag, which):
    pre = "%s_%s_" % (tag, which)
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


@pytest.mark.parametrize("tag", ["t5n5", "t3n2", "t3n2_sync"])
def test_update_kernel_matches_reference_step(dra, tag):
    """The fixture's stored rollout, laid out as the rollout kernel leaves it, with the bootstrap computed by the test from the
    fixture's target parameters (sync tag: the online ones, the copy fell inside the rollout): the parameters after
    dra_q_mlp_update + _fused.step(5) against the reference's own NStepDQNAgent.step (rtol 2e-5 / atol 2e-6)."""
    g = np.load(FIXTURE)
    discount, clip, lr = [float(x) for x in g[tag + "_cfg"][:3]]
    t_len, n, horizon, freq = [int(x) for x in g[tag + "_cfg"][3:7]]
    init, target = _fixture_params(g, tag, "init"), _fixture_params(g, tag, "target")
    boot_params = init if freq <= t_len else target
    with torch.no_grad():
        boot = R.forward(R.to_t(boot_params), g[tag + "_states"][t_len]).max(dim=1)[0].numpy()
    _within(boot, g[tag + "_bootstrap"], "bootstrap")
    agent = _bare_agent(dra, init, target, t_len, n, True, discount=discount, clip=clip, lr=lr)
    inputs = dict(state=g[tag + "_states"][:t_len], action=g[tag + "_action"].reshape(t_len, n), reward=g[tag + "_reward"].reshape(t_len, n),
                  mask=g[tag + "_mask"].reshape(t_len, n), bootstrap=boot)
    params, loss = _apply_update(dra, agent, inputs)
    np.testing.assert_allclose(loss, float(g[tag + "_loss"]), rtol=2e-5, atol=2e-6)
    worst = 0.0
    for k, got in params.items():
        want = g["%s_final_%s" % (tag, k)]
        worst = max(worst, float(np.max(np.abs(got - want) / (2e-6 + 2e-5 * np.abs(want)))))
    print("%s: worst parameter error as a fraction of atol + rtol |want|: %.3f" % (tag, worst))
    record_parity("n_step_dqn_feature update kernel vs reference step %s (fraction of the bar)" % tag, params=worst)
    for k, got in params.items():
        np.testing.assert_allclose(got, g["%s_final_%s" % (tag, k)], rtol=2e-5, atol=2e-6, err_msg=k)


# ------------------------------------------------------------------------------------------ the agent
A = K.AGENT


def _config(d, feature, graph=True, horizon=A["horizon"], n_env=A["n_env"], **extra):
    from deeprl_amd import zoo
    kw = dict(fused_nstep_feature=True) if feature else {}
    c = zoo.config("n_step_dqn_feature", game=GAME, tag="nstep_feat%d%d" % (feature, graph), graph_update=graph,
                   overrides=dict(num_workers=n_env, rollout_length=A["t_len"], target_network_update_freq=A["target_freq"], **extra),
                   **kw)
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=A["task_seed"], synthetic_done_period=horizon)
    c.random_action_prob = d.LinearSchedule(*A["eps"])
    c.log_interval = 10 ** 9
    return c


def _make_agent(d, monkeypatch, feature, graph=True, **kw):
    import deeprl_amd.agents as agents_mod
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    d.random_seed(9)
    torch.manual_seed(9)
    agent = d.NStepDQNAgent(_config(d, feature, graph, **kw))
    # the case's parameters (numpy-seeded: the same on every machine), copied into the optimiser's flat buffer through the views;
    # the target starts as their copy (NStepDQN_agent.py:21)
    init = K.restated_agent_run()["init"]
    with torch.no_grad():
        for k, p in agent.network.state_dict().items():
            p.copy_(torch.from_numpy(init[k]))
    agent._sync_target()
    np.random.seed(A["np_seed"])        # the exploration stream starts here on both paths
    return agent, rec


def _watch_host(agent, log):
    raw = agent.task.step

    def step(actions):
        o = raw(actions)
        log['actions'].append(np.asarray(actions).copy())
        log['masks'].append(1.0 - np.asarray(o[2], dtype=np.float32))
        return o
    agent.task.step = step


def _snapshot(agent, rec):
    torch.cuda.synchronize()
    return dict(params={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
                total=agent.total_steps, lines=[ln for ln in rec.lines if 'episodic_return_train' in ln],
                epsilon=agent.config.random_action_prob.current, rng=np.random.randint(0, 1 << 30, size=3))


def _run(d, monkeypatch, feature, graph=True, steps=A["steps"], **kw):
    from deeprl_amd.device_env import DeviceCartPoleVec
    agent, rec = _make_agent(d, monkeypatch, feature, graph, **kw)
    assert isinstance(agent.task, DeviceCartPoleVec) == bool(feature) and (agent._feature is not None) == bool(feature)
    log = dict(actions=[], masks=[])
    if not feature:
        _watch_host(agent, log)
    for _ in range(steps):
        agent.step()
        if feature:
            b = agent._feature.buffers(A["t_len"])
            log['actions'] += list(b['action'].cpu().numpy())
            log['masks'] += list(b['mask'].cpu().numpy())
    events = agent.episodes()
    out = _snapshot(agent, rec)
    out.update(actions=np.stack(log['actions']), masks=np.stack(log['masks']), events=events,
               graphed=agent._dev_graph.graph is not None, launches=agent._feature.launches if feature else 0)
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


def test_agent_device_path_equals_host_path(dra, monkeypatch, device_run):
    """NStepDQNAgent on the n_step_dqn_feature configuration (4 environments, rollout length 5, episodes of at most 7 steps,
    epsilon from 1.0 to 0.1 over 100 steps, a target copy every 3 steps) with config.fused_nstep_feature -- one rollout and one
    update launch, graph replay from the third step -- against the same agent with the switch off (the parent commit's path), and
    against the fp64 restatement: actions, masks, total_steps, the episodic-return log lines (late on the device path, otherwise
    the same), the np.random tail and the schedule's position equal; parameters within 2e-4 of each tensor's largest magnitude
    (floor 1e-2)."""
    from deeprl_amd.agents import _OnPolicyGraph
    a, b = device_run, _run(dra, monkeypatch, False)
    want = K.restated_agent_run()
    steps, t_len, n = A["steps"], A["t_len"], A["n_env"]
    assert a['graphed'] and not b['graphed'] and b['launches'] == 0
    assert a['launches'] == _OnPolicyGraph.WARMUP + 1          # the eager rollouts and the capture pass; the replays launch from the graph
    assert a['total'] == b['total'] == want['total'] == steps * t_len * n
    assert np.array_equal(a['actions'], b['actions']) and np.array_equal(a['masks'], b['masks'])
    assert np.array_equal(a['actions'], want['actions'].reshape(steps * t_len, n))
    assert np.array_equal(a['masks'], want['masks'].reshape(steps * t_len, n))
    assert a['lines'] == b['lines'] and len(a['lines']) >= 8
    assert a['events'] == _line_events(b['lines']) and b['events'] == []
    assert [r for _, r in a['events']] == [r for _, _, r in want['events']]
    assert np.array_equal(a['rng'], b['rng']) and np.array_equal(a['rng'], want['rng_tail'])
    assert a['epsilon'] == b['epsilon'] == want['epsilon']
    worst = 0.0
    for other, name in ((b['params'], "host path"), (want['params'], "restatement")):
        for k in a['params']:
            scale = max(np.abs(other[k]).max(), 1e-2)
            worst = max(worst, float(np.max(np.abs(a['params'][k] - other[k])) / (2e-4 * scale)))
        print("device vs %s parameters: worst fraction of the bar so far %.3f" % (name, worst))
    record_parity("n_step_dqn_feature agent device vs host path and restatement (fraction of the bar)", params=worst)
    for other in (b['params'], want['params']):
        for k in a['params']:
            scale = max(np.abs(other[k]).max(), 1e-2)
            assert np.max(np.abs(a['params'][k] - other[k])) <= 2e-4 * scale, k


def test_module_update_form_matches_the_fused_one(dra, monkeypatch, device_run):
    """config.fused_nstep_update False (device rollout, module-path update) over the same six steps: the same actions, masks and
    events; parameters within the agent test's bar."""
    b = _run(dra, monkeypatch, True, fused_nstep_update=False)
    a = device_run
    assert b['graphed'] and np.array_equal(a['actions'], b['actions']) and np.array_equal(a['masks'], b['masks'])
    assert a['events'] == b['events'] and a['lines'] == b['lines'] and a['total'] == b['total']
    for k in a['params']:
        scale = max(np.abs(b['params'][k]).max(), 1e-2)
        assert np.max(np.abs(a['params'][k] - b['params'][k])) <= 2e-4 * scale, k


def test_graph_replay_equals_eager(dra, monkeypatch):
    """config.graph_update = False keeps every step eager: after 8 steps parameters, actions and events are equal to the bit."""
    a = _run(dra, monkeypatch, True, graph=True, steps=8)
    b = _run(dra, monkeypatch, True, graph=False, steps=8)
    assert a['graphed'] and not b['graphed'] and a['launches'] == 3 and b['launches'] == 8
    assert a['total'] == b['total'] and a['lines'] == b['lines'] and a['events'] == b['events']
    assert np.array_equal(a['actions'], b['actions']) and np.array_equal(a['masks'], b['masks'])
    for k in a['params']:
        assert np.array_equal(_bits(a['params'][k]), _bits(b['params'][k])), k


def test_save_load_continues_the_run(dra, monkeypatch, device_run, tmp_path):
    """3 steps, save, load into a fresh agent, 3 more steps == 6 uninterrupted steps, bit for bit.  save() writes what the
    reference's checkpoint holds plus the environments' arrays and the device step counter; the optimiser's running averages,
    total_steps, the schedule and the np.random state are no part of a checkpoint, so the test carries them over by hand."""
    first, rec = _make_agent(dra, monkeypatch, True)
    for _ in range(3):
        first.step()
    name = str(tmp_path / "ckpt")
    first.save(name)
    assert os.path.isfile(name + ".envs") and os.path.isfile(name + ".model")
    rng = np.random.get_state()
    second, rec2 = _make_agent(dra, monkeypatch, True)
    assert int(second._feature.step_dev.item()) == 0
    second.load(name)
    assert int(second._feature.step_dev.item()) == 3 * A["t_len"] == second._step_host
    for key in ("env_state", "env_counter", "ep_steps", "ep_return"):
        assert torch.equal(getattr(second.task, key), getattr(first.task, key)), key
    second._fused.state1.copy_(first._fused.state1)
    second._fused.state2.copy_(first._fused.state2)
    second._fused.steps, second.total_steps = first._fused.steps, first.total_steps
    second.config.random_action_prob.current = first.config.random_action_prob.current
    np.random.set_state(rng)
    for _ in range(3):
        second.step()
    second.drain_episodes()
    got = _snapshot(second, rec2)
    first.close()
    second.close()
    assert got['total'] == device_run['total'] and got['epsilon'] == device_run['epsilon']
    assert [ln for ln in rec.lines if 'episodic_return_train' in ln] + got['lines'] == device_run['lines']
    assert np.array_equal(got['rng'], device_run['rng'])
    for k in got['params']:
        assert np.array_equal(_bits(got['params'][k]), _bits(device_run['params'][k])), k


def test_default_config_stays_on_the_host(dra, monkeypatch):
    """A default-Config NStepDQNAgent on the cart-pole Task keeps envs.Task (the path is opt-in); switching on with a network the
    kernels do not walk (a three-layer FCBody) keeps the host path and logs a warning naming the reason."""
    import deeprl_amd.agents as agents_mod
    d = dra
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)

    def make(**kw):
        c = d.Config()
        c.merge(dict(game=GAME, log_level=0, tag="nstep_feat_guard", **kw))
        c.num_workers = 4
        c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=3, synthetic_done_period=7)
        c.eval_env = d.Task(c.game, seed=4)
        c.optimizer_fn = lambda p: torch.optim.RMSprop(p, 0.001)
        c.random_action_prob = d.LinearSchedule(1.0, 0.05, 1e4)
        c.discount, c.gradient_clip, c.rollout_length, c.target_network_update_freq = 0.99, 5, 5, 200
        c.log_interval = 10 ** 9
        return c

    c = make()
    c.network_fn = lambda: d.VanillaNet(c.action_dim, d.FCBody(c.state_dim))
    d.random_seed(9)
    agent = d.NStepDQNAgent(c)
    assert type(agent.task) is d.Task and agent._feature is None and not rec.warnings
    agent.step()
    torch.cuda.synchronize()
    assert agent.total_steps == 5 * 4 and [e.c for e in agent.task.env.envs] == [5] * 4 and agent.episodes() == []
    agent.close()

    c = make(fused_nstep_feature=True)
    c.network_fn = lambda: d.VanillaNet(c.action_dim, d.FCBody(c.state_dim, (64, 64, 64)))
    agent = d.NStepDQNAgent(c)
    assert type(agent.task) is d.Task and agent._feature is None
    assert len(rec.warnings) == 1 and "the network is not VanillaNet over a two-layer" in rec.warnings[0]
    agent.step()
    torch.cuda.synchronize()
    assert agent.total_steps == 5 * 4 and [e.c for e in agent.task.env.envs] == [5] * 4
    agent.close()


# ------------------------------------------------------------------------------------------ the closed loop
def test_closed_loop_learns(dra, monkeypatch):
    """zoo.agent('n_step_dqn_feature', fused_nstep_feature=True) for n_learn environment steps and three fixed seeds: the median
    over the seeds of the mean return of the last 100 drained episodes must reach 2 x the random policy's mean return.  n_learn is
    the length at which the REFERENCE's own NStepDQNAgent over envs.CartPole reaches twice that bar in the median of 5 seeds
    (tests/golden/nstep_feature/learning_reference.json)."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    from deeprl_amd.device_env import DeviceCartPoleVec
    rec = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))
    bar = 2.0 * json.load(open(os.path.join(GOLDEN, "random_policy.json")))["mean"]
    n_learn = int(rec["n_learn"])
    assert rec["bar"] == bar and rec["medians"][str(n_learn)] >= 2.0 * bar
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    means = []
    for seed in K.LEARN_SEEDS:
        dra.random_seed(seed)
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        agent = zoo.agent("n_step_dqn_feature", game=GAME, tag="nstep_feat_learn%d" % seed, fused_nstep_feature=True)
        assert isinstance(agent.task, DeviceCartPoleVec)
        returns = []
        while agent.total_steps < n_learn:
            agent.step()
            if agent._dev_steps % 512 == 0:
                returns += [r for _, r in agent.episodes()]
        returns += [r for _, r in agent.episodes()]
        assert agent._dev_graph.graph is not None
        agent.close()
        means.append(float(np.mean(returns[-K.LAST_EPISODES:])))
        print("seed %d: %d episodes, mean return of the last %d: %.1f" % (seed, len(returns), K.LAST_EPISODES, means[-1]))
    median = float(np.median(means))
    print("median %.1f, bar %.1f (random policy x 2), reference median at %d steps %.1f" % (median, bar, n_learn, rec["medians"][str(n_learn)]))
    record_parity("n_step_dqn_feature closed loop: last-100 mean returns per seed, median, bar", median=median, bar=bar,
                  **{"seed_%d" % s: m for s, m in zip(K.LEARN_SEEDS, means)})
    assert median >= bar
