"""Edge-shape parity of the loss, scan and sampling kernels (csrc/losses.hip, csrc/scan.hip, dra_soft_update / dra_copy_f32)
against float64 references, at the shapes where their code paths change: one wave / many waves in block_sum and block_max,
second trips of grid-stride loops, the three dra_gae instantiations, the device-beta and powf PER branches, prefetch tails,
A = 1, out-of-range actions, and exact ties / boundary hits of every discrete decision.

Cases, references and bars live in tests/loss_edge_cases.py; tests/test_loss_edge_cases_host.py proves on the CPU that the
inputs carry the bars.  Rules:
  continuous  max |got - want64| <= 1e-5 * max |want64| per output tensor (the project's fp32 bar); exact zeros where the
              scale is 0.  Every measured error / scale goes to the parity log (tools/parity_summary.py sums it up).
  discrete    sampled actions and the support of dq / dlogits / dtheta equal the float64 reference exactly; a row may be left
              out only if its decision margin is under 1e-5 (scores) / 1e-6 (cumulative probabilities), at most 1 % of a
              case's rows, none in "exact" cases.
The loss kernels run on NaN-filled outputs (every element must be written) and twice (the second result bit for bit)."""
import numpy as np
import pytest
import torch

import loss_edge_cases as E
from parity_log import record_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    from deeprl_amd.support import select_device, Config
    select_device(0)
    return Config.DEVICE


def _ids(cases):
    return [c["name"] for c in cases]


def _d(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _close(kernel, case, what, got, want, rows=None):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (kernel, case, what, got.shape, want.shape)
    if rows is not None:
        got, want = got[rows], want[rows]
    assert np.all(np.isfinite(got)), "%s[%s] %s: non-finite output (an element the kernel never wrote?)" % (kernel, case, what)
    scale = np.abs(want).max() if want.size else 0.0
    if scale == 0.0:
        record_parity("loss_edges %s.%s[%s]" % (kernel, what, case), zero_scale_abs=np.abs(got).max() if got.size else 0.0)
        assert not np.any(got), "%s[%s] %s: float64 says exactly zero" % (kernel, case, what)
        return
    err = np.abs(got - want).max()
    print("%s[%s] %s: err/scale %.3g (bar %.1g), scale %.3g" % (kernel, case, what, err / scale, E.BAR, scale))
    record_parity("loss_edges %s.%s[%s]" % (kernel, what, case), err_over_scale=err / scale, scale=scale)
    assert err <= E.BAR * scale, "%s[%s] %s: max abs err %.3e vs scale %.3e (%.2e of it, bar %.0e)" % (
        kernel, case, what, err, scale, err / scale, E.BAR)


def _discrete(kernel, case, what, got, want, margin, threshold, exact, strict=None):
    """Exact agreement with the float64 decision, apart from the capped rows whose margin is under the threshold."""
    got, want = np.asarray(got), np.asarray(want)
    ex, n_ex, cap = E.exempt_rows(margin, threshold, len(want), exact, strict)
    used = int(((got != want) & ex).sum())
    print("%s[%s] %s: %d rows under the margin %.0e (cap %d), %d of them differ" % (kernel, case, what, n_ex, threshold, cap, used))
    record_parity("loss_edges %s.%s[%s]" % (kernel, what, case), exemptable_rows=n_ex, exemptions_used=used, rows=len(want))
    assert n_ex <= cap, "%s[%s] %s: %d rows under the margin, cap %d" % (kernel, case, what, n_ex, cap)
    bad = np.nonzero((got != want) & ~ex)[0]
    assert bad.size == 0, "%s[%s] %s: rows %s differ from the float64 decision (got %s, want %s, margins %s)" % (
        kernel, case, what, bad[:8], got[bad[:8]], want[bad[:8]], np.asarray(margin)[bad[:8]])
    return ex


def _support(kernel, case, what, grad, action):
    """Only the row of the (clamped) stored action may be non-zero: the kernels zero the rest."""
    g = grad.detach().cpu().numpy()
    assert np.all(np.isfinite(g)), "%s[%s] %s: element never written" % (kernel, case, what)
    off = np.ones(g.shape[:2], bool)
    off[np.arange(g.shape[0]), action] = False
    assert not np.any(g[off]), "%s[%s] %s: gradient outside the stored action's row" % (kernel, case, what)


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.int32), b[k].reshape(-1).view(torch.int32)), what + ": " + k


def _action(c, dev):
    return _d(c["action"].astype(np.float32) if c.get("act_f32") else c["action"], dev)


# ------------------------------------------------------------------------------------------------------------ td_loss
def _snapshot(out):
    return {k: v.clone() for k, v in out.items()}


def _td_bufs(c, dev, per):
    """Inputs (uploaded once) and NaN-filled outputs of one case; _td_launch may run on them any number of times."""
    b, a = c["B"], c["A"]
    out = dict(loss=_nan((), dev), dq=_nan((b, a), dev), delta=_nan((b,), dev))
    if per:
        out.update(prio=_nan((b,), dev), weights=_nan((b,), dev))
    return dict(act=_action(c, dev), t=[_d(c[k], dev) for k in ("q", "qt", "qo", "reward", "mask")]), out


def _td_launch(c, bufs, out, per, beta, sp):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    act, t = bufs["act"], bufs["t"]
    lib.dra_td_loss(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(act), int(act.dtype == torch.int64), ptr(t[3]), ptr(t[4]), c["B"], c["A"],
                    float(c["gamma_n"]), ptr(sp), float(beta), float(c["eps"]), float(c["per"][0] if per else 0.5),
                    ptr(out["loss"]), ptr(out["dq"]), ptr(out["delta"]), ptr(out.get("prio")), ptr(out.get("weights")), stream_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", E.td_cases(), ids=_ids(E.td_cases()))
def test_td_loss_edges(dev, c):
    w = E.want_td(c)
    per = c["per"] is not None
    sp = _d(c["sp"], dev) if per else None
    bufs, out = _td_bufs(c, dev, per)
    _td_launch(c, bufs, out, per, c["per"][1] if per else 0.0, sp)
    for k in ("loss", "delta", "dq") + (("prio", "weights") if per else ()):
        _close("td_loss", c["name"], k, out[k], w[k])
    _support("td_loss", c["name"], "dq", out["dq"], w["action"])
    first = _snapshot(out)      # the second launch writes over the first one's results, in the same buffers
    _same_bits(first, _td_launch(c, bufs, out, per, c["per"][1] if per else 0.0, sp), "td_loss[%s] second call" % c["name"])
    if per:   # the exponent read from sampling_prob[B] (beta < 0) gives the host-beta result bit for bit
        sp_ext = _d(np.concatenate([c["sp"], np.float32([c["per"][1]])]), dev)
        _same_bits(first, _td_launch(c, bufs, _td_bufs(c, dev, per)[1], per, -1.0, sp_ext), "td_loss[%s] device beta" % c["name"])


# ----------------------------------------------------------------------------------------------------------- c51_loss
def _c51_bufs(c, dev):
    b, a, n = c["B"], c["A"], c["N"]
    out = dict(kl=_nan((b,), dev), dlogits=_nan((b, a, n), dev))
    return dict(act=_action(c, dev),
                t=[_d(c[k], dev) for k in ("logits", "logits_t", "logits_o", "reward", "mask", "atoms", "weights")]), out


def _c51_launch(c, bufs, out):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    act, t = bufs["act"], bufs["t"]
    lib.dra_c51_loss(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(act), int(act.dtype == torch.int64), ptr(t[3]), ptr(t[4]), c["B"], c["A"],
                     c["N"], float(c["gamma_n"]), float(c["v_min"]), float(c["v_max"]), ptr(t[5]), ptr(out["kl"]),
                     ptr(out["dlogits"]), ptr(t[6]), stream_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", E.c51_cases(), ids=_ids(E.c51_cases()))
def test_c51_loss_edges(dev, c):
    from deeprl_amd import ops
    w = E.want_c51(c)
    bufs, out = _c51_bufs(c, dev)
    _c51_launch(c, bufs, out)
    _close("c51_loss", c["name"], "kl", out["kl"], w["kl"])          # the weights leave kl alone ...
    _close("c51_loss", c["name"], "dlogits", out["dlogits"], w["dlogits"])     # ... and scale the gradient
    _support("c51_loss", c["name"], "dlogits", out["dlogits"], w["action"])
    first = _snapshot(out)
    _same_bits(first, _c51_launch(c, bufs, out), "c51_loss[%s] second call" % c["name"])
    full = ops.c51_loss(*[_d(c[k], dev) for k in ("logits", "logits_t", "action", "reward", "mask")], c["gamma_n"], _d(c["atoms"], dev),
                        c["v_min"], c["v_max"], logits_next_online=_d(c["logits_o"], dev), weights=_d(c["weights"], dev))
    _close("c51_loss", c["name"], "loss", full["loss"], w["loss"])   # the weighted mean of kl
    assert torch.equal(full["kl"], out["kl"]) and torch.equal(full["dlogits"], out["dlogits"])


# ------------------------------------------------------------------------------------------------------------ qr_loss
def _qr_bufs(c, dev):
    b, a, n = c["B"], c["A"], c["N"]
    out = dict(loss_vec=_nan((n,), dev), loss=_nan((), dev), dtheta=_nan((b, a, n), dev))
    return dict(act=_action(c, dev), ws=_nan((b * n,), dev), t=[_d(c[k], dev) for k in ("theta", "theta_t", "reward", "mask")]), out


def _qr_launch(c, bufs, out):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    act, t = bufs["act"], bufs["t"]
    lib.dra_qr_loss(ptr(t[0]), ptr(t[1]), ptr(act), int(act.dtype == torch.int64), ptr(t[2]), ptr(t[3]), c["B"], c["A"], c["N"],
                    float(c["gamma_n"]), ptr(bufs["ws"]), ptr(out["loss_vec"]), ptr(out["loss"]), ptr(out["dtheta"]), stream_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", E.qr_cases(), ids=_ids(E.qr_cases()))
def test_qr_loss_edges(dev, c):
    w = E.want_qr(c)
    bufs, out = _qr_bufs(c, dev)
    _qr_launch(c, bufs, out)
    for k in ("loss_vec", "loss", "dtheta"):
        _close("qr_loss", c["name"], k, out[k], w[k])
    _support("qr_loss", c["name"], "dtheta", out["dtheta"], w["action"])
    first = _snapshot(out)      # the workspace is reused as well
    _same_bits(first, _qr_launch(c, bufs, out), "qr_loss[%s] second call" % c["name"])


# ------------------------------------------------------------------------------------------------ ppo_loss / a2c_loss
@pytest.mark.parametrize("c", E.ppo_cases(), ids=_ids(E.ppo_cases()))
def test_ppo_loss_edges(dev, c):
    from deeprl_amd import ops
    w = E.want_ppo(c)
    args = [_d(c[k], dev) for k in ("lp", "ent", "v", "old_lp", "adv", "ret")]
    out3, g = ops.ppo_loss(*args, c["clip"], c["ew"])
    _close("ppo_loss", c["name"], "out", out3, w["out"])
    # the clip gate is a discrete decision on the ratio: rows within 1e-5 of a clip bound may be gated either way
    ex, n_ex, cap = E.exempt_rows(w["margins"]["clip_gap"], E.SCORE_GAP, c["M"], c["exact"])
    record_parity("loss_edges ppo_loss.clip_gate[%s]" % c["name"], exemptable_rows=n_ex, rows=c["M"])
    assert n_ex <= cap
    _close("ppo_loss", c["name"], "g_lp", g[0], w["g_lp"], rows=~ex)
    gate_got, gate_want = g[0].cpu().numpy() != 0.0, w["g_lp"] != 0.0
    assert np.array_equal(gate_got[~ex], gate_want[~ex]), "ppo_loss[%s]: clip gate differs from float64" % c["name"]
    _close("ppo_loss", c["name"], "g_ent", g[1], w["g_ent"])
    _close("ppo_loss", c["name"], "g_v", g[2], w["g_v"])
    out3b, gb = ops.ppo_loss(*args, c["clip"], c["ew"])
    _same_bits(dict(out=out3, g_lp=g[0], g_ent=g[1], g_v=g[2]), dict(out=out3b, g_lp=gb[0], g_ent=gb[1], g_v=gb[2]),
               "ppo_loss[%s] second call" % c["name"])


@pytest.mark.parametrize("c", E.a2c_cases(), ids=_ids(E.a2c_cases()))
def test_a2c_loss_edges(dev, c):
    from deeprl_amd import ops
    w = E.want_a2c(c)
    args = [_d(c[k], dev) for k in ("lp", "ent", "v", "adv", "ret")]
    out4, g = ops.a2c_loss(*args, c["ew"], c["vw"])
    _close("a2c_loss", c["name"], "out", out4, w["out"])
    for got, k in zip(g, ("g_lp", "g_ent", "g_v")):
        _close("a2c_loss", c["name"], k, got, w[k])
    out4b, gb = ops.a2c_loss(*args, c["ew"], c["vw"])
    _same_bits(dict(out=out4, g_lp=g[0], g_ent=g[1], g_v=g[2]), dict(out=out4b, g_lp=gb[0], g_ent=gb[1], g_v=gb[2]),
               "a2c_loss[%s] second call" % c["name"])


# ------------------------------------------------------------------------------------------- per_weights, weighted_mean
@pytest.mark.parametrize("c", E.per_cases(), ids=_ids(E.per_cases()))
def test_per_weights_edges(dev, c):
    from deeprl_amd import ops
    w = E.want_per(c)
    lv, sp = _d(c["loss_vec"], dev), _d(c["sp"], dev)
    prio, wt = ops.per_weights(lv, sp, c["beta"], c["eps"], c["alpha"])
    _close("per_weights", c["name"], "prio", prio, w["prio"])
    _close("per_weights", c["name"], "weights", wt, w["weights"])
    none_prio, wt2 = ops.per_weights(None, sp, c["beta"], c["eps"], c["alpha"])
    assert none_prio is None and torch.equal(wt2, wt)
    prio_d, wt_d = ops.per_weights_dev(lv, sp, _d(np.float32([c["beta"]]), dev), c["eps"], c["alpha"])
    _close("per_weights_dev", c["name"], "prio", prio_d, w["prio"])
    _close("per_weights_dev", c["name"], "weights", wt_d, w["weights"])
    none_prio, wt_d2 = ops.per_weights_dev(None, sp, _d(np.float32([c["beta"]]), dev), c["eps"], c["alpha"])
    assert none_prio is None and torch.equal(wt_d2, wt_d)


@pytest.mark.parametrize("c", E.wmean_cases(), ids=_ids(E.wmean_cases()))
@pytest.mark.parametrize("weighted", [False, True])
def test_weighted_mean_edges(dev, c, weighted):
    from deeprl_amd import ops
    got = ops.weighted_mean(_d(c["x"], dev), _d(c["w"], dev) if weighted else None)
    _close("weighted_mean", "%s%s" % (c["name"], "w" if weighted else ""), "mean", got, E.want_wmean(c, weighted))


# -------------------------------------------------------------------------------------------------------- categorical
@pytest.mark.parametrize("c", E.cat_cases(), ids=_ids(E.cat_cases()))
def test_categorical_edges(dev, c):
    from deeprl_amd import ops
    w = E.want_cat(c)
    logits = _d(c["logits"], dev)
    act, lp, ent = ops.categorical_fwd(logits, action=_d(c["action"], dev))
    assert np.array_equal(act.cpu().numpy(), c["action"])
    _close("categorical_fwd", c["name"], "log_pi_a", lp, w["log_pi_a"])
    _close("categorical_fwd", c["name"], "entropy", ent, w["entropy"])
    dl = ops.categorical_bwd(logits, _d(c["action"], dev), _d(c["g_lp"], dev), _d(c["g_ent"], dev))
    _close("categorical_bwd", c["name"], "dlogits", dl, w["dlogits"])
    ent_np = ent.cpu().numpy()
    if c["peaked"].any():     # one logit 50 above the rest: p log p of the others must not turn into NaN or noise
        assert np.all(np.isfinite(ent_np[c["peaked"]])) and np.all(np.abs(ent_np[c["peaked"]]) <= 1e-6)
        np.testing.assert_allclose(ent_np[c["equal"]], np.log(c["A"]), rtol=E.BAR, atol=0 if c["A"] > 1 else 1e-30)
    # sampling: the action is the float64 inverse CDF of the uniform; u = 1.0 gives the last action whatever the rounding
    got, lp_s, ent_s = ops.categorical_fwd(logits, uniform=_d(c["u"], dev))
    got = got.cpu().numpy()
    assert got.min() >= 0 and got.max() < c["A"]
    _discrete("categorical_fwd", c["name"], "sampled", got, w["sampled"], w["margins"]["cdf_gap"], E.CUM_GAP, c["exact"], w["strict"])
    _close("categorical_fwd", c["name"], "log_pi_sampled", lp_s, w["logp"][np.arange(c["B"]), got])
    assert torch.equal(ent_s, ent)


# ------------------------------------------------------------------------------------------------------ gumbel_sample
@pytest.mark.parametrize("c", E.gumbel_cases(), ids=_ids(E.gumbel_cases()))
def test_gumbel_sample_edges(dev, c):
    from deeprl_amd import ops
    n, a, lo = c["n"], c["A"], c["lo"]
    logits = _d(c["logits"], dev)
    step_dev = torch.tensor([c["step"]], dtype=torch.int64, device=dev)
    launches = []
    for k in range(2):      # the kernel itself advances the device step, by exactly one per launch
        got = ops.gumbel_sample(logits, c["seed"], step_dev, lo).cpu().numpy()
        assert step_dev.item() == c["step"] + k + 1
        want, gap, _ = E.gumbel_ref(c["logits"], c["seed"], c["step"] + k, lo)
        _discrete("gumbel_sample", c["name"], "action_step%d" % k, got, want, gap, E.SCORE_GAP, c["exact"])
        launches.append(got)
    if n >= 16 and a > 1:
        assert not np.array_equal(launches[0], launches[1]), "consecutive launches drew the same actions"
    # rank invariance: rows [lo, lo + n) of ONE call over all lo + n rows are what the shard's own call drew
    full = E.gumbel_full_logits(c)
    step_dev.fill_(c["step"])
    got_full = ops.gumbel_sample(_d(full, dev), c["seed"], step_dev, 0).cpu().numpy()
    assert np.array_equal(got_full[lo:], launches[0]), "gumbel_sample[%s]: a shard differs from the same rows of the full call" % c["name"]
    want_full, gap_full, _ = E.gumbel_ref(full, c["seed"], c["step"], 0)
    _discrete("gumbel_sample", c["name"], "action_full", got_full, want_full, gap_full, E.SCORE_GAP, c["exact"])


# ---------------------------------------------------------------------------------------------- gae, adv_normalize_
@pytest.mark.parametrize("c", E.gae_cases(), ids=_ids(E.gae_cases()))
def test_gae_edges(dev, c):
    from deeprl_amd import ops
    w = E.want_gae(c)
    args = [_d(c[k], dev) for k in ("reward", "mask", "value")]
    adv, ret = ops.gae(*args, c["gamma"], c["tau"], c["use_gae"])
    _close("gae", c["name"], "adv", adv, w["adv"])
    _close("gae", c["name"], "ret", ret, w["ret"])
    adv2, ret2 = ops.gae(*args, c["gamma"], c["tau"], c["use_gae"])
    _same_bits(dict(adv=adv, ret=ret), dict(adv=adv2, ret=ret2), "gae[%s] second call" % c["name"])


@pytest.mark.parametrize("c", E.advnorm_cases(), ids=_ids(E.advnorm_cases()))
def test_adv_normalize_edges(dev, c):
    from deeprl_amd import ops
    a = _d(c["adv"], dev)
    ops.adv_normalize_(a)
    _close("adv_normalize_", c["name"], "adv", a, E.want_advnorm(c))


# ------------------------------------------------------------------------------------------- soft_update, copy_f32
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("n", E.FLAT_SIZES)
@pytest.mark.parametrize("mix", E.SOFT_MIXES)
def test_soft_update_bit_exact(dev, n, mix):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, ptr, stream_ptr
    t_np, s_np = E.flat_case(n, 9000 + n % 1000)
    t, s = _d(t_np, dev), _d(s_np, dev)
    if n:
        ops.soft_update(t[:n], s[:n], mix)
    else:   # an empty torch view has no address: n = 0 is a call on the buffers themselves
        lib.dra_soft_update(ptr(t), ptr(s), 0, float(np.float32(1.0 - mix)), float(mix), stream_ptr())
    got = t.cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits(E.polyak_ref(t_np[:n], s_np[:n], mix))), "soft_update: not the float32 expression"
    assert np.array_equal(_bits(got[n:]), _bits(t_np[n:])), "soft_update wrote behind n"
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(s_np))


@pytest.mark.parametrize("n", E.FLAT_SIZES)
def test_copy_f32_bit_exact(dev, n):
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, ptr, stream_ptr
    t_np, s_np = E.flat_case(n, 9500 + n % 1000)
    t, s = _d(t_np, dev), _d(s_np, dev)
    if n:
        ops.copy_f32(t[:n], s[:n])
    else:
        lib.dra_copy_f32(ptr(t), ptr(s), 0, stream_ptr())
    got = t.cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits(s_np[:n]))
    assert np.array_equal(_bits(got[n:]), _bits(t_np[n:])), "copy_f32 wrote behind n"


# ---------------------------------------------------------------------------------------------------- argument limits
def test_argument_limits_are_refused_before_any_launch(dev):
    """Sizes beyond what one workgroup / the LDS can hold: DRA_EINVAL from the host-side checks (nothing is launched)."""
    from deeprl_amd import ops
    from deeprl_amd._lib import DraError
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    zi = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
    with pytest.raises(DraError):
        ops.td_loss(z(1025, 4), z(1025, 4), zi(1025), z(1025), z(1025), 0.99)
    with pytest.raises(DraError):
        ops.per_weights(z(1025), z(1025) + 1.0 / 1025, 0.4, 0.01, 0.5)
    with pytest.raises(DraError):
        ops.per_weights_dev(z(1025), z(1025) + 1.0 / 1025, z(1) + 0.4, 0.01, 0.5)
    for n in (1, 257):
        with pytest.raises(DraError):
            ops.c51_loss(z(2, 3, n), z(2, 3, n), zi(2), z(2), z(2), 0.99, z(n), -10.0, 10.0)
    with pytest.raises(DraError):
        ops.qr_loss(z(2, 3, 1025), z(2, 3, 1025), zi(2), z(2), z(2), 0.99)
    with pytest.raises(DraError):
        ops.categorical_fwd(z(4, 65), action=zi(4))
    with pytest.raises(DraError):
        ops.categorical_fwd(z(4, 65), uniform=z(4))
    with pytest.raises(DraError):
        ops.categorical_bwd(z(4, 65), zi(4), z(4), z(4))
    with pytest.raises(DraError):     # 3 planes x 14000 steps: 173 KB, beyond the 160 KB LDS guard
        ops.gae(z(14000, 1, 1), z(14000, 1, 1), z(14001, 1, 1), 0.99, 0.95, True)
    torch.cuda.synchronize()
