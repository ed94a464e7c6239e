"""GPU tests of option_critic_feature on device-resident cart-pole environments: the rollout and the update kernel of
csrc/oc_mlp.hip against the restatement (tests/option_critic_feature_restatement.py, pinned to the reference's own run by
tests/test_option_critic_feature_host.py, which also asserts the decision margins and relu pre-activation margins these
comparisons rest on), the update kernel against the module path and against the reference's recorded OptionCriticAgent.step,
OptionCriticAgent's device path against the restatement and the host-stepped path, graph replay against eager, save / load, and a
closed loop that has to LEARN.
Bars: exact for everything the fp64 environment determines once the decisions are equal (options, actions, observations, states,
counters, masks, ring rows, the carried option state); 1e-5 of a tensor's largest magnitude (floor 1) for fp32 values."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from feature_kernel_harness import (      # noqa: F401  (dra: the fixture)
    GAME, GATE, GUARD, dra, _Rec, _fraction, _within, _bits, _as_int, _guarded, _flat, _tails_intact, _body, _line_events)
from parity_log import record_parity

import option_critic_feature_cases as K
import option_critic_feature_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "option_critic_feature")
FIXTURE = os.path.join(GOLDEN, "option_critic_feature_step.npz")


def _net_struct(params, target, dev, hidden, gate, n_opt, padded):
    from deeprl_amd import oc_mlp
    flat, offs = _flat(R.KEYS, params, padded)
    tflat, _ = _flat(R.KEYS, target if target is not None else params, padded)
    flat, tflat = torch.from_numpy(flat).to(dev), torch.from_numpy(tflat).to(dev)
    net = oc_mlp.Net()
    net.param, net.target = flat.data_ptr(), tflat.data_ptr()
    for field, k in zip(oc_mlp._OFFSETS, R.KEYS):
        setattr(net, field, offs[k])
    net.state_dim, net.n_actions, net.hidden, net.gate, net.n_options = 4, 2, hidden, GATE[gate], n_opt
    return net, flat, tflat, offs


# ------------------------------------------------------------------------------------------ rollout kernel
ROLLOUT_OUT = ("state", "q", "beta", "logits", "option", "prev_option", "action", "init", "log_pi_a", "entropy", "reward", "mask")


def _launch(dra, case, start):
    """One dra_oc_mlp_rollout from the case's start -> dict of host arrays (guards included) and the return code."""
    from deeprl_amd import oc_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    hidden, gate, n, t_len, horizon, n_opt, padded = case[:7]
    net, flat, tflat, _ = _net_struct(start["params"], start["target"], dev, hidden, gate, n_opt, padded)
    nan = float("nan")
    f, i64 = torch.float32, torch.int64
    spec = dict(env_state=((n, 4), torch.float64, nan), env_counter=((n,), i64, -7), ep_steps=((n,), torch.int32, -7),
                ep_return=((n,), torch.float64, nan), env_seed=((n,), i64, -7), step=((1,), i64, -7),
                ep_count=((1,), i64, -7), ep_ring=((K.RING_CAP, 3), torch.float64, nan),
                eps=((t_len,), f, nan), uniform=((t_len, n, 3), f, nan), carried_option=((n,), i64, -7),
                carried_init=((n,), torch.uint8, 9),
                state=((t_len, n, 4), f, nan), q=((t_len, n, n_opt), f, nan), beta=((t_len, n, n_opt), f, nan),
                logits=((t_len, n, 2), f, nan), option=((t_len, n), i64, -7), prev_option=((t_len, n), i64, -7),
                action=((t_len, n), i64, -7), init=((t_len, n), f, nan), log_pi_a=((t_len, n), f, nan), entropy=((t_len, n), f, nan),
                reward=((t_len, n), f, nan), mask=((t_len, n), f, nan), bootstrap=((n,), f, nan))
    full, view = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], view[k] = _guarded(shape, dt, dev, fill)
    view["env_state"].copy_(torch.from_numpy(start["raw"]))
    view["env_counter"].zero_(); view["ep_steps"].zero_(); view["ep_return"].zero_()
    view["env_seed"].copy_(torch.tensor(start["seeds"], dtype=torch.int64))
    view["step"].fill_(K.STEP0); view["ep_count"].fill_(K.RING_COUNT0)
    view["eps"].copy_(torch.from_numpy(start["eps"])); view["uniform"].copy_(torch.from_numpy(start["uniform"]))
    view["carried_option"].copy_(torch.from_numpy(start["prev_option"]))
    view["carried_init"].copy_(torch.from_numpy(start["is_initial"].astype(np.uint8)))
    io = oc_mlp.RolloutIO()
    for k in ("env_state", "env_counter", "ep_steps", "ep_return", "env_seed", "ep_count", "ep_ring", "eps", "uniform", "bootstrap"):
        setattr(io, k, view[k].data_ptr())
    io.step_counter, io.prev_option, io.is_initial = view["step"].data_ptr(), view["carried_option"].data_ptr(), view["carried_init"].data_ptr()
    for k in ROLLOUT_OUT:
        setattr(io, "out_" + k, view[k].data_ptr())
    io.horizon, io.ring_cap, io.reward_coef, io.t_len, io.n_env = horizon, K.RING_CAP, 1.0, t_len, n
    before = flat.cpu().numpy().copy(), tflat.cpu().numpy().copy()
    rc = lib.dra_oc_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in full.items()}
    out["rc"], out["spec"] = rc, spec
    # (both parameter buffers are read only)
    assert np.array_equal(_bits(flat.cpu().numpy()), _bits(before[0])) and np.array_equal(_bits(tflat.cpu().numpy()), _bits(before[1]))
    return out, (net, io, full, view, flat, tflat)


@pytest.mark.parametrize("case", K.ROLLOUT_CASES, ids=K.case_id)
def test_rollout_kernel_matches_restatement(dra, case):
    """dra_oc_mlp_rollout against the restatement from a mixed prev_option / is_initial, a non-zero step counter and a short ring
    near its end: options, actions, the prev_option / init each step read, the carried state after the launch equal (the host
    suite asserts a decision margin >= 1e-4 at every (step, environment) of every case, no row excluded); stored observations,
    final environment state, counters, episode steps and returns, rewards, masks, the step counter and the ring's rows and count
    equal to the bit; q, beta, the chosen option's logits, log pi(a), entropy and the TARGET network's bootstrap within 1e-5 of
    scale; the guard elements behind every buffer untouched; both parameter buffers unchanged; a second launch from the same start
    gives the same bits everywhere."""
    hidden, gate, n, t_len, horizon, n_opt, padded = case[:7]
    want, envs, start = K.restated_rollout(case)
    out, _ = _launch(dra, case, start)
    assert out["rc"] == 0
    for k in ("option", "action", "prev_option"):
        assert np.array_equal(_body(out, k), want[k]), k
    assert np.array_equal(_bits(_body(out, "init")), _bits(want["init"]))
    assert np.array_equal(_body(out, "carried_option"), want["prev_option_out"])
    assert np.array_equal(_body(out, "carried_init"), want["is_initial_out"].astype(np.uint8))
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
    assert np.array_equal(_bits(_body(out, "eps")), _bits(start["eps"])) and np.array_equal(_bits(_body(out, "uniform")), _bits(start["uniform"]))
    fr = {k: _within(_body(out, k), want[k], k) for k in ("q", "beta", "logits", "log_pi_a", "entropy", "bootstrap")}
    record_parity("oc_mlp rollout kernel vs restatement %s (fraction of the bar)" % K.case_id(case), **fr)
    _tails_intact(out)
    again, _ = _launch(dra, case, start)
    for k in out["spec"]:
        assert np.array_equal(_bits(out[k]), _bits(again[k])), k


def test_rollout_refuses_unsupported_shapes_and_launches_nothing(dra):
    """One option (the reference's initial prev_options = ones is out of range there), nine options, 65 environments, hidden 48, a
    null pointer, a negative offset and the other shapes outside the table: -22, and nothing is written."""
    from deeprl_amd import oc_mlp
    from deeprl_amd._lib import lib, stream_ptr
    case = K.ROLLOUT_CASES[1]
    _, _, start = K.restated_rollout(case)
    out, (net, io, full, view, flat, tflat) = _launch(dra, case, start)
    before = {k: v.clone() for k, v in full.items()}

    def refused(**change):
        n2, io2 = oc_mlp.Net.from_buffer_copy(net), oc_mlp.RolloutIO.from_buffer_copy(io)
        for k, v in change.items():
            setattr(n2 if hasattr(n2, k) else io2, k, v)
        rc = lib.dra_oc_mlp_rollout.raw(ctypes.byref(n2), ctypes.byref(io2), stream_ptr())
        torch.cuda.synchronize()
        return rc == -22 and all(torch.equal(_as_int(before[k]), _as_int(full[k])) for k in full)

    assert refused(n_options=1) and refused(n_options=9) and refused(n_options=0)
    assert refused(n_env=65) and refused(n_env=0) and refused(hidden=48) and refused(hidden=128)
    assert refused(state_dim=5) and refused(n_actions=3) and refused(gate=3)
    assert refused(t_len=0) and refused(horizon=0) and refused(ring_cap=0)
    assert refused(w2=-1) and refused(bq=-4) and refused(wp=-1) and refused(bb=-2)
    assert refused(out_q=None) and refused(out_beta=None) and refused(bootstrap=None) and refused(eps=None) and refused(uniform=None)
    assert refused(prev_option=None) and refused(is_initial=None) and refused(out_option=None) and refused(target=None)
    assert lib.dra_oc_mlp_rollout.raw(None, ctypes.byref(io), stream_ptr()) == -22
    assert lib.dra_oc_mlp_rollout.raw(ctypes.byref(net), None, stream_ptr()) == -22


# ------------------------------------------------------------------------------------------ update kernel
SENTINEL = 123.25       # what the gaps of the gradient buffer hold before a launch


def _launch_update(dra, case, padded, rows_override=None):
    """One dra_oc_mlp_update on the case's inputs -> (dict of host arrays, rc, handles)."""
    from deeprl_amd import oc_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    hidden, gate, n, t_len, _, n_opt = case[:6]
    u = K.restated_update(case)
    net, flat, _, offs = _net_struct(u["params"], None, dev, hidden, gate, n_opt, padded)
    net.target = None          # (the update does not read it)
    grad_full, grad = _guarded((flat.numel(),), torch.float32, dev, SENTINEL)
    nan = float("nan")
    spec = dict(ret=((t_len, n), torch.float32, nan), adv=((t_len, n), torch.float32, nan),
                beta_adv=((t_len, n), torch.float32, nan), loss=((4,), torch.float32, nan))
    full, view = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], view[k] = _guarded(shape, dt, dev, fill)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    inp = {k: up(v) for k, v in u["inputs"].items()}
    inp["eps"] = up(u["eps"])
    io = oc_mlp.UpdateIO()
    for k in K.UPDATE_INPUTS + ("eps",):
        setattr(io, k, inp[k].data_ptr())
    io.grad = grad.data_ptr()
    io.out_ret, io.out_adv, io.out_beta_adv, io.out_loss = [view[k].data_ptr() for k in ("ret", "adv", "beta_adv", "loss")]
    io.discount, io.termination_regularizer, io.entropy_weight = K.DISCOUNT, K.TERM_REG, K.ENT_W
    io.t_len, io.n_env = t_len if rows_override is None else rows_override, n
    flat_before = flat.cpu().numpy().copy()
    rc = lib.dra_oc_mlp_update.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(flat.cpu().numpy()), _bits(flat_before))        # NaN gaps included: the parameters are read only
    out = {k: v.cpu().numpy() for k, v in full.items()}
    out["spec"], out["grad_full"] = spec, grad_full.cpu().numpy()
    return out, rc, (offs, inp, flat)


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_kernel_matches_restatement(dra, case, padded):
    """dra_oc_mlp_update against the fp64 restatement: ret equal to the fp32 scan bit for bit; adv, beta_adv, the four losses and
    each of the ten gradient tensors within 1e-5 of its fp64 counterpart's largest magnitude (floor 1); the measured fraction of
    that bar is recorded next to the fraction the module path's fp32 autograd reaches on the same case.  In the one-option case the
    other options' rows of fc_q / fc_pi / fc_beta and their bias entries are exactly 0.0.  Padded layout: the NaN gaps of the
    parameter buffer and the sentinel in the gaps of the gradient buffer survive.  Two launches give the same bits."""
    hidden, gate, n, t_len, horizon, n_opt, one_option = case[:7]
    u = K.restated_update(case)
    out, rc, (offs, _, flat) = _launch_update(dra, case, padded)
    assert rc == 0
    ret32 = R.returns(u["inputs"]["reward"], u["inputs"]["mask"], u["inputs"]["bootstrap"], K.DISCOUNT, dtype=np.float32)
    assert np.array_equal(_bits(_body(out, "ret")), _bits(ret32))
    fr = dict(ret=_within(_body(out, "ret"), u["ret"], "ret"), adv=_within(_body(out, "adv"), u["adv"], "adv"),
              beta_adv=_within(_body(out, "beta_adv"), u["beta_adv"], "beta_adv"))
    for i, name in enumerate(("loss", "q_loss", "pi_loss", "beta_loss")):
        fr[name] = _within(_body(out, "loss")[i:i + 1], u["loss"][i:i + 1], name)
    g = out["grad_full"]
    covered = np.zeros(g.size, dtype=bool)
    module = _module_grads(dra, case)
    mod_fr = {}
    for k in R.KEYS:
        want = u["grads"][k]
        got = g[offs[k]:offs[k] + want.size].reshape(want.shape)
        covered[offs[k]:offs[k] + want.size] = True
        fr[k] = _fraction(got, want, k)
        mod_fr[k] = _fraction(module[k], want, "module path " + k)
    record_parity("oc_mlp update kernel vs restatement %s %s (fraction of the bar)" % (K.update_id(case), "padded" if padded else "packed"),
                  **{k.replace(".", "_"): v for k, v in fr.items()})
    record_parity("option_critic_feature module path fp32 autograd vs restatement %s (fraction of the bar)" % K.update_id(case),
                  **{k.replace(".", "_"): v for k, v in mod_fr.items()})
    for k in R.KEYS:
        assert fr[k] <= 1.0, (k, fr[k])
    # everything that is not one of the ten tensors keeps the sentinel: the gaps (padded) and the guard behind the buffer
    n_param = sum(u["grads"][k].size for k in R.KEYS)
    assert (g[~covered] == SENTINEL).all() and (~covered).sum() == GUARD + (flat.numel() - n_param)
    assert not (g[covered] == SENTINEL).any()
    if padded:
        assert np.isnan(flat.cpu().numpy()).sum() == flat.numel() - n_param > 0
    if one_option:
        o = K.FORCED_OPTION
        others = [j for j in range(n_opt) if j != o]
        part = lambda k, shape: g[offs[k]:offs[k] + int(np.prod(shape))].reshape(shape)
        wq, wb, wp = part("fc_q.weight", (n_opt, hidden)), part("fc_beta.weight", (n_opt, hidden)), part("fc_pi.weight", (n_opt, 2, hidden))
        bq, bb, bp = part("fc_q.bias", (n_opt,)), part("fc_beta.bias", (n_opt,)), part("fc_pi.bias", (n_opt, 2))
        for t in (wq, wb, wp, bq, bb, bp):
            assert (t[others] == 0.0).all()
        assert np.abs(wq[o]).max() > 1e-3 and np.abs(wp[o]).max() > 1e-4 and np.abs(wb[o]).max() > 1e-5
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
    assert (out["grad_full"] == SENTINEL).all() and all(np.isnan(out[k]).all() for k in ("ret", "adv", "beta_adv", "loss"))


# ------------------------------------------------------------------------------------------ update against module path / reference
def _bare_agent(d, params, target, t_len, n, fused_update, n_opt=2, discount=K.DISCOUNT, clip=5, lr=0.001, gate="relu", hidden=64,
                term_reg=K.TERM_REG, ent_w=K.ENT_W):
    """An OptionCriticAgent with everything _feature_learn's update half reads and nothing else (no task: the rollout is given)."""
    import torch.nn.functional as F
    from deeprl_amd import oc_mlp
    from deeprl_amd.optim import FlatParams, FusedOptimizer
    cfg = d.Config()
    cfg.discount, cfg.gradient_clip, cfg.rollout_length, cfg.num_workers = discount, clip, int(t_len), int(n)
    cfg.termination_regularizer, cfg.entropy_weight = term_reg, ent_w
    cfg.fused_oc_feature, cfg.fused_oc_update = True, fused_update
    agent = d.OptionCriticAgent.__new__(d.OptionCriticAgent)
    agent.config, agent.grad_hook = cfg, None
    mk = lambda: d.OptionCriticNet(d.FCBody(4, (hidden, hidden), gate=F.relu if gate == "relu" else torch.tanh), 2, n_opt)
    agent.network, agent.target_network = mk(), mk()
    agent.network.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in params.items()})
    agent.target_network.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in target.items()})
    agent.optimizer = torch.optim.RMSprop(agent.network.parameters(), lr)
    agent._fused = FusedOptimizer.adopt(agent.optimizer)
    agent._target_flat = FlatParams(list(agent.target_network.parameters()))
    assert oc_mlp.why_not(agent) is None
    agent._feature = oc_mlp.Rollout(agent, oc_mlp.shape(agent.network))
    return agent


def _apply_update(d, agent, inputs, eps, step=True):
    """The update half of OptionCriticAgent._feature_learn on given rollout buffers -> (parameters after it, the four losses)."""
    dev = d.Config.DEVICE
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_len, n = inputs["action"].shape
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    b = {k: up(np.asarray(inputs[k], dtype=np.int64 if k in ("option", "prev_option", "action") else np.float32)) for k in K.UPDATE_INPUTS}
    b.update(ret=z(t_len, n), adv=z(t_len, n), beta_adv=z(t_len, n), loss=z(4))
    agent._feature.run = lambda t: b        # (the rollout is given)
    agent._feature.eps = up(np.asarray(eps, dtype=np.float32))
    agent._rollout_step = 0
    if not step:
        agent._fused.step = lambda clip: None
    from deeprl_amd.mlp_rollout import Plan
    agent._feature_learn(Plan(None, t_len))
    torch.cuda.synchronize()
    return ({k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
            agent.last_losses.detach().cpu().numpy().astype(np.float64), b)


def _module_grads(dra, case):
    """The module path's fp32 autograd on the same inputs -> {key: gradient} (what fused_oc_update=False computes)."""
    hidden, gate, n, t_len, _, n_opt = case[:6]
    u = K.restated_update(case)
    agent = _bare_agent(dra, u["params"], u["params"], t_len, n, False, n_opt=n_opt, gate=gate, hidden=hidden)
    _apply_update(dra, agent, u["inputs"], u["eps"], step=False)
    return {k: p.grad.detach().cpu().numpy().copy() for k, p in agent.network.named_parameters()}


@pytest.mark.parametrize("case", [K.UPDATE_CASES[1], K.UPDATE_CASES[2], K.UPDATE_CASES[3]], ids=K.update_id)
def test_fused_update_matches_module_path_on_the_device(dra, case):
    """The same rollout buffers through config.fused_oc_update True (dra_oc_mlp_update) and False (the scan kernel, one module
    forward, the three losses in torch, autograd): the parameters after _fused.step agree within rtol 2e-5 / atol 2e-6, and so do
    the losses and ret / adv / beta_adv."""
    hidden, gate, n, t_len, _, n_opt = case[:6]
    u = K.restated_update(case)
    got = {}
    for fused in (True, False):
        agent = _bare_agent(dra, u["params"], u["params"], t_len, n, fused, n_opt=n_opt, gate=gate, hidden=hidden)
        got[fused] = _apply_update(dra, agent, u["inputs"], u["eps"])
    worst = 0.0
    for k in got[True][0]:
        a, b = got[True][0][k], got[False][0][k]
        worst = max(worst, float(np.max(np.abs(a - b) / (2e-6 + 2e-5 * np.abs(b)))))
        assert (a != np.asarray(u["params"][k], dtype=np.float32)).any(), k
    record_parity("oc_mlp fused update vs module path %s (fraction of the bar)" % K.update_id(case), params=worst)
    for k in got[True][0]:
        np.testing.assert_allclose(got[True][0][k], got[False][0][k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(got[True][1], got[False][1], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(got[True][1], u["loss"], rtol=2e-5, atol=2e-6)
    for k in ("ret", "adv", "beta_adv"):
        np.testing.assert_allclose(got[True][2][k].cpu().numpy(), got[False][2][k].cpu().numpy(), rtol=2e-5, atol=2e-6, err_msg=k)


def _fixture_params(g, tag, which):
    pre = "%s_%s_" % (tag, which)
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


@pytest.mark.parametrize("tag", ["t5n5", "t3n2", "t3n2_o3"])
def test_update_kernel_matches_reference_step(dra, tag):
    """The fixture's stored rollout, laid out as the rollout kernel leaves it (the chosen option's log pi row stands for its
    logits: a softmax is invariant under the shift between them), with the reference's recorded bootstrap: the parameters after
    dra_oc_mlp_update + _fused.step(5) against the reference's own OptionCriticAgent.step (rtol 2e-5 / atol 2e-6, the bar of
    test_gpu_nstep_feature.py::test_update_kernel_matches_reference_step), the four losses, ret, advantage and beta_advantage
    within 1e-5 of scale."""
    g = np.load(FIXTURE)
    c = g[tag + "_cfg"]
    discount, clip, lr, term_reg, ent_w = float(c[0]), float(c[1]), float(c[2]), float(c[9]), float(c[10])
    t_len, n, n_opt = int(c[3]), int(c[4]), int(c[8])
    init, target = _fixture_params(g, tag, "init"), _fixture_params(g, tag, "target")
    agent = _bare_agent(dra, init, target, t_len, n, True, n_opt=n_opt, discount=discount, clip=clip, lr=lr, term_reg=term_reg, ent_w=ent_w)
    log_pi = g[tag + "_log_pi"]
    inputs = dict(state=g[tag + "_states"][:t_len], q=g[tag + "_q"], beta=g[tag + "_beta"], logits=log_pi, option=g[tag + "_option"],
                  prev_option=g[tag + "_prev_option"], action=g[tag + "_action"], init=g[tag + "_init"],
                  log_pi_a=np.take_along_axis(log_pi, g[tag + "_action"][..., None], axis=-1)[..., 0], entropy=g[tag + "_entropy"],
                  reward=g[tag + "_reward"], mask=g[tag + "_mask"], bootstrap=g[tag + "_bootstrap"])
    params, losses, b = _apply_update(dra, agent, inputs, g[tag + "_eps"])
    fr = dict(loss=_within(losses, g[tag + "_loss"], "losses"), ret=_within(b["ret"].cpu().numpy(), g[tag + "_ret"], "ret"),
              adv=_within(b["adv"].cpu().numpy(), g[tag + "_advantage"], "advantage"),
              beta_adv=_within(b["beta_adv"].cpu().numpy(), g[tag + "_beta_advantage"], "beta_advantage"))
    worst = 0.0
    for k, got in params.items():
        want = g["%s_final_%s" % (tag, k)]
        worst = max(worst, float(np.max(np.abs(got - want) / (2e-6 + 2e-5 * np.abs(want)))))
    print("%s: worst parameter error as a fraction of atol + rtol |want|: %.3f" % (tag, worst))
    record_parity("option_critic_feature update kernel vs reference step %s (fraction of the bar)" % tag, params=worst, **fr)
    for k, got in params.items():
        np.testing.assert_allclose(got, g["%s_final_%s" % (tag, k)], rtol=2e-5, atol=2e-6, err_msg=k)


# ------------------------------------------------------------------------------------------ the agent
A = K.AGENT


def _config(d, feature, graph=True, horizon=A["horizon"], n_env=A["n_env"], **extra):
    from deeprl_amd import zoo
    kw = dict(fused_oc_feature=True) if feature else {}
    kw.update({k: extra.pop(k) for k in list(extra) if k.startswith("fused_")})
    c = zoo.config("option_critic_feature", game=GAME, tag="oc_feat%d%d" % (feature, graph), graph_update=graph,
                   overrides=dict(num_workers=n_env, rollout_length=A["t_len"], target_network_update_freq=A["target_freq"], **extra),
                   **kw)
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=A["task_seed"], synthetic_done_period=horizon)
    c.random_option_prob = d.LinearSchedule(*A["eps"])
    c.log_interval = 10 ** 9
    return c


def _make_agent(d, monkeypatch, feature, graph=True, **kw):
    import deeprl_amd.agents as agents_mod
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    d.random_seed(9)
    agent = d.OptionCriticAgent(_config(d, feature, graph, **kw))
    # the case's parameters (numpy-seeded: the same on every machine), copied into the optimiser's flat buffer through the views;
    # the target starts as their copy (OptionCritic_agent.py:20)
    init = K.agent_init_params()
    with torch.no_grad():
        for k, p in agent.network.state_dict().items():
            p.copy_(torch.from_numpy(init[k]))
    agent._sync_target()
    torch.manual_seed(A["torch_seed"])      # the device generator's uniforms start here
    return agent, rec


def _snapshot(agent, rec):
    torch.cuda.synchronize()
    return dict(params={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
                total=agent.total_steps, lines=[ln for ln in rec.lines if 'episodic_return_train' in ln],
                epsilon=agent.config.random_option_prob.current, prev_option=agent.prev_options.cpu().numpy().copy(),
                is_initial=agent.is_initial_states.cpu().numpy().astype(bool))


def _run(d, monkeypatch, feature=True, graph=True, steps=A["steps"], decisions=None, **kw):
    """`steps` agent steps.  feature: the device path (options, actions, masks and the uniforms read back from its buffers); else
    the host path, its Categorical.sample made to return `decisions` -- per rollout step the option (both option draws), then the
    action -- as tests/test_gpu_option_critic_pixel.py::test_device_path_equals_host_path does."""
    from deeprl_amd.device_env import DeviceCartPoleVec
    agent, rec = _make_agent(d, monkeypatch, feature, graph, **kw)
    assert isinstance(agent.task, DeviceCartPoleVec) == bool(feature) and (agent._feature is not None) == bool(feature)
    log = dict(options=[], actions=[], masks=[], uniforms=[])
    if not feature:
        queue = []
        for o, a in zip(decisions[0], decisions[1]):
            queue += [o, o, a]
        queue.reverse()
        monkeypatch.setattr(torch.distributions.Categorical, "sample",
                            lambda self, sample_shape=torch.Size(): torch.as_tensor(queue.pop(), device=self.probs.device))
        raw = agent.task.step

        def step(actions):
            o = raw(actions)
            log['actions'].append(np.asarray(actions).copy())
            log['masks'].append(1.0 - np.asarray(o[2], dtype=np.float32))
            return o
        agent.task.step = step
    for _ in range(steps):
        agent.step()
        if feature:
            b = agent._feature.buffers(A["t_len"])
            log['options'] += list(b['option'].cpu().numpy())
            log['actions'] += list(b['action'].cpu().numpy())
            log['masks'] += list(b['mask'].cpu().numpy())
            log['uniforms'].append(agent._feature.uniform.cpu().numpy().copy())
    events = agent.episodes()
    out = _snapshot(agent, rec)
    out.update(actions=np.stack(log['actions']), masks=np.stack(log['masks']), events=events,
               graphed=agent._dev_graph.graph is not None, launches=agent._feature.launches if feature else 0)
    if feature:
        out.update(options=np.stack(log['options']), uniforms=np.stack(log['uniforms']))
    else:
        assert not queue
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


def test_agent_device_path_equals_restatement_and_host_path(dra, monkeypatch, device_run):
    """OptionCriticAgent on the option_critic_feature configuration (4 environments, rollout length 5, episodes of at most 7
    steps, 2 options, option epsilon from 1.0 to 0.1 over 100 steps, a target copy every 3 steps) with config.fused_oc_feature --
    one rollout and one update launch, graph replay from the third step -- against the fp64 restatement fed the uniforms the
    device run drew, and against the same agent with the switch off (the parent commit's path) made to take the device run's
    decisions: options, actions, masks, total_steps, the episodic-return log lines (late on the device path, otherwise the same)
    and the schedule's position equal; parameters within 2e-4 of each tensor's largest magnitude (floor 1e-2)."""
    from deeprl_amd.agents import _OnPolicyGraph
    a = device_run
    steps, t_len, n = A["steps"], A["t_len"], A["n_env"]
    assert a['uniforms'].shape == (steps, t_len, n, 3) and len(np.unique(a['uniforms'])) > steps * t_len * n      # a new draw per rollout
    want = K.restated_agent_run(a['uniforms'])
    print("agent case: decision margin %.3e, fp32 restatement makes the same decisions: %s, %d episodes"
          % (want["margin"], want["fp32_same_decisions"], len(want["events"])))
    assert want["fp32_same_decisions"]
    b = _run(dra, monkeypatch, False, decisions=(a['options'], a['actions']))
    assert a['graphed'] and not b['graphed'] and b['launches'] == 0
    assert a['launches'] == _OnPolicyGraph.WARMUP + 1          # the eager rollouts and the capture pass; the replays launch from the graph
    assert a['total'] == b['total'] == want['total'] == steps * t_len * n
    assert np.array_equal(a['options'], want['options'].reshape(steps * t_len, n))
    assert np.array_equal(a['actions'], want['actions'].reshape(steps * t_len, n)) and np.array_equal(a['actions'], b['actions'])
    assert np.array_equal(a['masks'], want['masks'].reshape(steps * t_len, n)) and np.array_equal(a['masks'], b['masks'])
    assert np.array_equal(a['prev_option'], want['prev_option']) and np.array_equal(a['is_initial'], want['is_initial'])
    assert np.array_equal(a['prev_option'], b['prev_option']) and np.array_equal(a['is_initial'], b['is_initial'])
    assert a['lines'] == b['lines'] and len(a['lines']) >= 8
    assert a['events'] == _line_events(b['lines']) and b['events'] == []
    assert [r for _, r in a['events']] == [r for _, _, r in want['events']]
    assert a['epsilon'] == b['epsilon'] == want['epsilon']
    worst = 0.0
    for other, name in ((b['params'], "host path"), (want['params'], "restatement")):
        for k in a['params']:
            scale = max(np.abs(other[k]).max(), 1e-2)
            worst = max(worst, float(np.max(np.abs(a['params'][k] - other[k])) / (2e-4 * scale)))
        print("device vs %s parameters: worst fraction of the bar so far %.3f" % (name, worst))
    record_parity("option_critic_feature agent device vs host path and restatement (fraction of the bar)", params=worst)
    init = K.agent_init_params()
    for other in (b['params'], want['params']):
        for k in a['params']:
            scale = max(np.abs(other[k]).max(), 1e-2)
            assert np.max(np.abs(a['params'][k] - other[k])) <= 2e-4 * scale, k
    assert sum(int((a['params'][k] != init[k]).sum()) for k in init) > 100


def test_module_update_form_matches_the_fused_one(dra, monkeypatch, device_run):
    """config.fused_oc_update False (device rollout, module-path update) over the same six steps: the same options, actions, masks
    and events; parameters within the agent test's bar."""
    b = _run(dra, monkeypatch, True, fused_oc_update=False)
    a = device_run
    assert b['graphed'] and np.array_equal(a['uniforms'], b['uniforms'])
    assert np.array_equal(a['options'], b['options']) and np.array_equal(a['actions'], b['actions']) and np.array_equal(a['masks'], b['masks'])
    assert a['events'] == b['events'] and a['lines'] == b['lines'] and a['total'] == b['total']
    for k in a['params']:
        scale = max(np.abs(b['params'][k]).max(), 1e-2)
        assert np.max(np.abs(a['params'][k] - b['params'][k])) <= 2e-4 * scale, k


def test_graph_replay_equals_eager(dra, monkeypatch):
    """config.graph_update = False keeps every step eager: after 8 steps parameters, options, actions and events are equal to the
    bit."""
    a = _run(dra, monkeypatch, True, graph=True, steps=8)
    b = _run(dra, monkeypatch, True, graph=False, steps=8)
    assert a['graphed'] and not b['graphed'] and a['launches'] == 3 and b['launches'] == 8
    assert a['total'] == b['total'] and a['lines'] == b['lines'] and a['events'] == b['events']
    assert np.array_equal(a['options'], b['options']) and np.array_equal(a['actions'], b['actions']) and np.array_equal(a['masks'], b['masks'])
    assert np.array_equal(a['prev_option'], b['prev_option']) and np.array_equal(a['is_initial'], b['is_initial'])
    for k in a['params']:
        assert np.array_equal(_bits(a['params'][k]), _bits(b['params'][k])), k


def test_save_load_continues_the_run(dra, monkeypatch, device_run, tmp_path):
    """3 steps, save, load into a fresh agent, 3 more steps == 6 uninterrupted steps, bit for bit, prev_option / is_initial
    included.  save() writes what the reference's checkpoint holds plus the environments' arrays, the device step counter and the
    carried option state; the optimiser's running averages, total_steps, the schedule and the device generator's state are no part
    of a checkpoint, so the test carries them over by hand."""
    first, rec = _make_agent(dra, monkeypatch, True)
    for _ in range(3):
        first.step()
    name = str(tmp_path / "ckpt")
    first.save(name)
    assert os.path.isfile(name + ".envs") and os.path.isfile(name + ".model")
    rng = torch.cuda.get_rng_state()
    second, rec2 = _make_agent(dra, monkeypatch, True)
    assert int(second._feature.step_dev.item()) == 0 and bool(second.is_initial_states.all()) and bool((second.prev_options == 1).all())
    second.load(name)
    assert int(second._feature.step_dev.item()) == 3 * A["t_len"] == second._step_host
    for key in ("env_state", "env_counter", "ep_steps", "ep_return"):
        assert torch.equal(getattr(second.task, key), getattr(first.task, key)), key
    assert torch.equal(second.prev_options, first.prev_options) and torch.equal(second.is_initial_states, first.is_initial_states)
    assert second.prev_options.data_ptr() == second._feature.prev_option.data_ptr()      # (loaded in place: the kernel reads them)
    second._fused.state1.copy_(first._fused.state1)
    second._fused.state2.copy_(first._fused.state2)
    second._fused.steps, second.total_steps = first._fused.steps, first.total_steps
    second.config.random_option_prob.current = first.config.random_option_prob.current
    torch.cuda.set_rng_state(rng)
    for _ in range(3):
        second.step()
    second.drain_episodes()
    got = _snapshot(second, rec2)
    first.close()
    second.close()
    assert got['total'] == device_run['total'] and got['epsilon'] == device_run['epsilon']
    assert [ln for ln in rec.lines if 'episodic_return_train' in ln] + got['lines'] == device_run['lines']
    assert np.array_equal(got['prev_option'], device_run['prev_option']) and np.array_equal(got['is_initial'], device_run['is_initial'])
    for k in got['params']:
        assert np.array_equal(_bits(got['params'][k]), _bits(device_run['params'][k])), k


def test_default_config_stays_on_the_host(dra, monkeypatch):
    """A default-Config OptionCriticAgent on the cart-pole Task keeps envs.Task (the path is opt-in) and logs no warning;
    switching on with a network the kernels do not walk (a three-layer FCBody) or with one option keeps the host path and logs one
    warning naming the reason."""
    import deeprl_amd.agents as agents_mod
    d = dra
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)

    def make(**kw):
        c = d.Config()
        c.merge(dict(game=GAME, log_level=0, tag="oc_feat_guard", **kw))
        c.num_workers = 4
        c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=3, synthetic_done_period=7)
        c.eval_env = d.Task(c.game, seed=4)
        c.optimizer_fn = lambda p: torch.optim.RMSprop(p, 0.001)
        c.random_option_prob = d.LinearSchedule(1.0, 0.1, 1e4)
        c.discount, c.gradient_clip, c.rollout_length, c.target_network_update_freq = 0.99, 5, 5, 200
        c.termination_regularizer, c.entropy_weight = 0.01, 0.01
        c.log_interval = 10 ** 9
        return c

    c = make()
    c.network_fn = lambda: d.OptionCriticNet(d.FCBody(c.state_dim), c.action_dim, num_options=2)
    d.random_seed(9)
    agent = d.OptionCriticAgent(c)
    assert type(agent.task) is d.Task and agent._feature is None and not rec.warnings
    agent.step()
    torch.cuda.synchronize()
    assert agent.total_steps == 5 * 4 and [e.c for e in agent.task.env.envs] == [5] * 4 and agent.episodes() == []
    agent.close()

    c = make(fused_oc_feature=True)
    c.network_fn = lambda: d.OptionCriticNet(d.FCBody(c.state_dim, (64, 64, 64)), c.action_dim, num_options=2)
    agent = d.OptionCriticAgent(c)
    assert type(agent.task) is d.Task and agent._feature is None
    assert len(rec.warnings) == 1 and "the network is not OptionCriticNet over a two-layer" in rec.warnings[0]
    agent.step()
    torch.cuda.synchronize()
    assert agent.total_steps == 5 * 4 and [e.c for e in agent.task.env.envs] == [5] * 4
    agent.close()

    c = make(fused_oc_feature=True)
    c.network_fn = lambda: d.OptionCriticNet(d.FCBody(c.state_dim), c.action_dim, num_options=1)
    agent = d.OptionCriticAgent(c)      # (not stepped: with one option the reference's initial prev_options = ones is out of range)
    assert type(agent.task) is d.Task and agent._feature is None
    assert len(rec.warnings) == 2 and "not built for 1 option" in rec.warnings[1]
    agent.close()


# ------------------------------------------------------------------------------------------ the closed loop
LEARNING = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))


def test_closed_loop_learns(dra, monkeypatch):
    """zoo.agent('option_critic_feature', fused_oc_feature=True) for n_learn environment steps and three fixed seeds: the median
    over the seeds of the mean return of the last 100 drained episodes must reach the bar of
    tests/golden/option_critic_feature/learning_reference.json (2 x the random policy's mean return; n_learn is the length at
    which the REFERENCE's own OptionCriticAgent over envs.CartPole reaches twice that bar in the median of 5 seeds)."""
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    from deeprl_amd.device_env import DeviceCartPoleVec
    rec = LEARNING
    assert rec["learns"] is True      # (the record of a reference that does not learn has no closed-loop test: DESIGN.md 4.14)
    bar, n_learn = float(rec["bar"]), int(rec["n_learn"])
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    means = []
    for seed in K.LEARN_SEEDS:
        dra.random_seed(seed)
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        agent = zoo.agent("option_critic_feature", game=GAME, tag="oc_feat_learn%d" % seed, fused_oc_feature=True)
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
    print("median %.1f, bar %.1f, reference median at %d steps %.1f" % (median, bar, n_learn, rec["medians"][str(n_learn)]))
    record_parity("option_critic_feature closed loop: last-100 mean returns per seed, median, bar", median=median, bar=bar,
                  **{"seed_%d" % s: m for s, m in zip(K.LEARN_SEEDS, means)})
    assert median >= bar
