"""GPU parity tests of csrc/a2c_mlp.hip at its shape and path edges, through the C ABI: dra_a2c_mlp_rollout at the cases of
tests/a2c_mlp_edge_cases.py (the two instantiations the workload-shape suite never launches, the corner of the supported range,
row blocks past the row groups, both paths of the statistics' fold, the normaliser's clip, differing step counters, reward_coef,
horizon 1) and dra_gauss_head_fwd / _bwd past one workgroup of rows and up to 64 action dimensions, against the float64
restatement and the bars of that module (whose cases tests/test_a2c_mlp_edge_cases_host.py proves on the CPU).  Every buffer has
guard elements behind it, every launch is repeated for equal bits, every refusal is checked to have launched nothing, and every
measured maximum goes to the parity log as a fraction of its bar."""
import ctypes

import numpy as np
import pytest
import torch

import a2c_mlp_edge_cases as E
from parity_log import record_parity
from test_gpu_a2c_continuous import _net_struct

pytestmark = pytest.mark.gpu
EINVAL = -22
GUARD = 8       # elements behind every buffer's stated size, filled with a sentinel that must survive
NAN = float("nan")


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """A test that left the device in error ends the session: nothing more is launched on a faulted GPU."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test, nothing more is launched: %s" % e, returncode=3)


def _guarded(shape, dtype, dev, fill):
    n = int(np.prod(shape))
    full = torch.full((n + GUARD,), fill, dtype=dtype, device=dev)
    return full, full[:n].view(*shape)


def _bits(a):
    """An array's bytes, for comparisons to the bit (NaN guard values included)."""
    return np.ascontiguousarray(a).view(np.uint8)


def _dev_bits(t):
    return _bits(t.detach().cpu().contiguous().numpy())


def _guards_intact(out, spec):
    for k, (shape, dt, fill) in spec.items():
        tail = out[k][int(np.prod(shape)):]
        assert tail.size == GUARD and (np.isnan(tail).all() if fill != fill else (tail == fill).all()), k


# ------------------------------------------------------------------------------------------------ rollout
def _launch(dra, case, start):
    """One dra_a2c_mlp_rollout from the case's start, every buffer guarded -> (dict of host arrays with their guards, the return
    code and the parameter buffer's bytes before and after; the structs and device buffers)."""
    from deeprl_amd import a2c_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    n, t_len, S, A, H, gate, kind, horizon, clip = case
    net, flat = _net_struct(start["params"], dev, S, A, H, gate)
    f32, f64, i64 = torch.float32, torch.float64, torch.int64
    spec = dict(env_state=((n, S), f64, NAN), env_counter=((n,), i64, -7), env_seed=((n,), i64, -7), rms=((2 * S + 1,), f64, NAN),
                cur_state=((n, S), f32, NAN), sampler=((1,), i64, -7), state=((t_len, n, S), f32, NAN), action=((t_len, n, A), f32, NAN),
                v=((t_len + 1, n), f32, NAN), reward=((t_len, n), f32, NAN), mask=((t_len, n), f32, NAN))
    full, view = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], view[k] = _guarded(shape, dt, dev, fill)
    view["env_state"].copy_(torch.from_numpy(np.ascontiguousarray(start["raw"])))
    view["env_counter"].copy_(torch.tensor(start["counters"], dtype=i64))
    view["env_seed"].copy_(torch.tensor(start["seeds"], dtype=i64))
    view["rms"].copy_(torch.from_numpy(np.ascontiguousarray(start["rms"])))
    view["sampler"].fill_(E.SAMPLER0)
    io = a2c_mlp.RolloutIO()
    io.env_state, io.env_counter, io.env_seed = view["env_state"].data_ptr(), view["env_counter"].data_ptr(), view["env_seed"].data_ptr()
    io.rms, io.cur_state, io.sampler_step = view["rms"].data_ptr(), view["cur_state"].data_ptr(), view["sampler"].data_ptr()
    io.out_state, io.out_action, io.out_v = view["state"].data_ptr(), view["action"].data_ptr(), view["v"].data_ptr()
    io.out_reward, io.out_mask = view["reward"].data_ptr(), view["mask"].data_ptr()
    io.env0, io.n_global, io.noise_seed, io.horizon = E.ENV0_EXTRA, n + E.ENV0_EXTRA + 1, E.NOISE_SEED, horizon
    io.reward_coef, io.t_len, io.n_env = E.REWARD_COEF, t_len, n
    if kind == "identity":
        io.rms_epsilon, io.rms_clip, io.rms_update = 0.0, float("inf"), 0
    else:
        io.rms_epsilon, io.rms_clip, io.rms_update = 1e-8, clip, 1 if kind == "meanstd-update" else 0
    flat_before = _dev_bits(flat)
    rc = lib.dra_a2c_mlp_rollout.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in full.items()}
    out.update(rc=rc, spec=spec, flat_before=flat_before, flat_after=_dev_bits(flat))
    return out, (net, io, full, flat)


def _body(out, k):
    shape = out["spec"][k][0]
    return out[k][:int(np.prod(shape))].reshape(shape)


@pytest.mark.parametrize("case", E.ROLLOUT_CASES, ids=E.case_id)
def test_rollout_edge_case_matches_restatement(dra, case):
    """dra_a2c_mlp_rollout against the float64 restatement at an edge case: rewards (which carry reward_coef), masks, the
    counters of the pre-stepped environments and the sampler position exact; stored observations, actions, values and the final
    normalised observation within 1e-5 of the largest magnitude; raw environment state at rtol 1e-6 / atol 1e-8; updated
    statistics at rtol 1e-7 with the count exact, statistics that are not updated unchanged to the bit; the guard elements behind
    all eleven buffers and the parameter buffer (leading gap and NaN padding included) untouched; a second launch from the same
    start gives the same bits everywhere."""
    from deeprl_amd import a2c_mlp
    n, t_len, S, A, H, gate, kind, horizon, clip = case
    cid = E.case_id(case)
    want, envs, norm, start = E.rollout_reference(case)
    assert a2c_mlp.supported(S, A, H, n, E.GATE_CODES[gate])
    out, _ = _launch(dra, case, start)
    assert out["rc"] == 0
    assert int(_body(out, "sampler")[0]) == E.SAMPLER0 + t_len + 1
    assert np.array_equal(_body(out, "env_counter"), [e.c for e in envs])
    assert np.array_equal(_body(out, "env_seed"), start["seeds"])
    assert np.array_equal(_bits(_body(out, "mask")), _bits(want["mask"]))
    assert np.array_equal(_bits(_body(out, "reward")), _bits(want["reward"]))
    errs = E.compare_rollout({k: _body(out, k) for k in E.ROLLOUT_KEYS}, want)
    errs["raw"] = E.fraction("raw", _body(out, "env_state"), want["raw_states"])
    rms = _body(out, "rms")
    if kind == "meanstd-update":
        errs["rms_mean"], errs["rms_var"], same_count = E.compare_stats(rms, E.final_stats(norm, start), S)
        assert same_count and rms[2 * S] > start["rms"][2 * S]
    else:
        assert np.array_equal(_bits(rms), _bits(start["rms"]))
    for key, r in errs.items():
        print("%s %s: %.4f of the bar" % (cid, key, r))
    record_parity("a2c_mlp rollout edge case %s vs restatement (fraction of the bar)" % cid, **errs)
    for key in E.ROLLOUT_KEYS:
        assert errs[key] <= E.bar(cid, "rollout"), (key, errs[key])
    assert errs["raw"] <= E.bar(cid, "raw"), errs["raw"]
    if kind == "meanstd-update":
        assert errs["rms_mean"] <= E.bar(cid, "stats") and errs["rms_var"] <= E.bar(cid, "stats"), (errs["rms_mean"], errs["rms_var"])
    _guards_intact(out, out["spec"])
    assert np.array_equal(out["flat_before"], out["flat_after"])        # (the parameter buffer is read only)
    again, _ = _launch(dra, case, start)
    assert again["rc"] == 0
    for k in out["spec"]:
        assert np.array_equal(_bits(out[k]), _bits(again[k])), k


def test_rollout_refuses_and_launches_nothing(dra):
    """After one good launch, every altered copy of the two structs is answered with DRA_EINVAL and leaves every guarded buffer
    and the parameter buffer as they were, to the bit."""
    from deeprl_amd import a2c_mlp
    from deeprl_amd._lib import lib, stream_ptr
    case = E.ROLLOUT_CASES[1]
    n = case[0]
    start = E.rollout_reference(case)[3]
    out, (net, io, full, flat) = _launch(dra, case, start)
    assert out["rc"] == 0
    before = {k: _dev_bits(v) for k, v in full.items()}
    before["param"] = _dev_bits(flat)

    def refused(**change):
        n2, io2 = a2c_mlp.Net.from_buffer_copy(net), a2c_mlp.RolloutIO.from_buffer_copy(io)
        for k, v in change.items():
            assert hasattr(n2, k) != hasattr(io2, k), k
            setattr(n2 if hasattr(n2, k) else io2, k, v)
        rc = lib.dra_a2c_mlp_rollout.raw(ctypes.byref(n2), ctypes.byref(io2), stream_ptr())
        torch.cuda.synchronize()
        return rc == EINVAL and all(np.array_equal(before[k], _dev_bits(full[k])) for k in full) and \
            np.array_equal(before["param"], _dev_bits(flat))

    assert refused(state_dim=65) and refused(state_dim=0) and refused(action_dim=17) and refused(action_dim=0)
    assert refused(hidden=16) and refused(hidden=48) and refused(hidden=128)
    assert refused(n_env=65) and refused(n_env=0) and refused(gate=0) and refused(gate=3)
    assert refused(t_len=0) and refused(horizon=0) and refused(n_global=n - 1) and refused(env0=-1)
    assert refused(a_w2=-1) and refused(off_std=-1)
    assert refused(out_v=None) and refused(rms=None) and refused(cur_state=None)
    # (and the unaltered structs still launch: the refusals above are the alterations', not the copies')
    n2, io2 = a2c_mlp.Net.from_buffer_copy(net), a2c_mlp.RolloutIO.from_buffer_copy(io)
    assert lib.dra_a2c_mlp_rollout.raw(ctypes.byref(n2), ctypes.byref(io2), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(before["env_counter"], _dev_bits(full["env_counter"]))


# ------------------------------------------------------------------------------------------------ head kernels
def _head_buffers(dev, n, a):
    f32 = torch.float32
    spec = dict(mean=((n, a), f32, NAN), log_pi_a=((n, 1), f32, NAN), entropy=((n, 1), f32, NAN), dz=((n, a), f32, NAN), dstd=((a,), f32, NAN))
    full, view = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], view[k] = _guarded(shape, dt, dev, fill)
    return spec, full, view


@pytest.mark.parametrize("n,a", E.HEAD_CASES)
def test_gauss_head_edge_shapes(dra, n, a):
    """dra_gauss_head_fwd / _bwd past one workgroup of rows (n > 256: the forward's second workgroup, the backward's second trip
    round its row loop) and up to kHeadMaxA = 64 action dimensions, into guarded buffers through the C ABI: mean, log_pi_a,
    entropy, dz and dstd within 1e-5 of each tensor's largest magnitude (floor 1) of the float64 restatement, the guards
    untouched; ops.gauss_head_fwd / _bwd (dstd written into a view of a guarded buffer) give the same bits, which is also the
    second backward launch's bit-repeat."""
    from deeprl_amd import ops
    from deeprl_amd._lib import lib, ptr, stream_ptr
    dev = dra.Config.DEVICE
    z, std, action, g_lp, g_ent = E.head_case(n, a)
    want = E.head_reference(n, a)
    up = lambda x: torch.from_numpy(x).to(dev)
    zt, st, at, glt, get = up(z), up(std), up(action), up(g_lp), up(g_ent)
    spec, full, view = _head_buffers(dev, n, a)
    lib.dra_gauss_head_fwd(ptr(zt), ptr(st), ptr(at), n, a, ptr(view["mean"]), ptr(view["log_pi_a"]), ptr(view["entropy"]), stream_ptr())
    lib.dra_gauss_head_bwd(ptr(zt), ptr(st), ptr(at), ptr(glt), ptr(get), n, a, ptr(view["dz"]), ptr(view["dstd"]), stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in full.items()}
    got = {k: out[k][:int(np.prod(shape))].reshape(shape) for k, (shape, _, _) in spec.items()}
    errs = {k: E.fraction("head", got[k], want[k]) for k in spec}
    for key, r in errs.items():
        print("[%d,%d] %s: %.4f of the bar" % (n, a, key, r))
    record_parity("gauss head kernels at edge shape [%d,%d] vs fp64 restatement (fraction of the bar)" % (n, a), **errs)
    for key, r in errs.items():
        assert r <= E.bar("head_%d_%d" % (n, a), "head"), (key, r)
    _guards_intact(out, spec)
    # the ops wrappers: the same kernels, the same bits; dstd lands in the caller's view and nowhere behind it
    mean, lp, ent = ops.gauss_head_fwd(zt, st, at)
    dfull, dview = _guarded((a,), torch.float32, dev, NAN)
    dz2, dstd2 = ops.gauss_head_bwd(zt, st, at, glt, get, dstd=dview)
    torch.cuda.synchronize()
    assert dstd2.data_ptr() == dview.data_ptr()
    assert np.array_equal(_dev_bits(mean), _bits(got["mean"])) and np.array_equal(_dev_bits(lp), _bits(got["log_pi_a"]))
    assert np.array_equal(_dev_bits(ent), _bits(got["entropy"]))
    assert np.array_equal(_dev_bits(dz2), _bits(got["dz"]))
    assert np.array_equal(_dev_bits(dfull), _bits(out["dstd"]))             # (dstd and the NaN guard behind it)
    # (the inputs are read only)
    assert np.array_equal(_dev_bits(zt), _bits(z)) and np.array_equal(_dev_bits(st), _bits(std)) and np.array_equal(_dev_bits(at), _bits(action))


def test_gauss_head_refuses_too_many_dimensions(dra):
    """a_dim = 65 is one past kHeadMaxA: both ops raise DraError, the C ABI answers DRA_EINVAL, and nothing is written."""
    from deeprl_amd import ops
    from deeprl_amd._lib import DraError, lib, ptr, stream_ptr
    dev = dra.Config.DEVICE
    n, a = 4, E.K_HEAD_MAX_A + 1
    rs = np.random.RandomState(65)
    up = lambda x: torch.from_numpy(x.astype(np.float32)).to(dev)
    zt, st, at, glt, get = up(rs.randn(n, a)), up(rs.randn(a)), up(rs.randn(n, a)), up(rs.randn(n, 1)), up(rs.randn(n, 1))
    dfull, dview = _guarded((a,), torch.float32, dev, NAN)
    with pytest.raises(DraError):
        ops.gauss_head_fwd(zt, st, at)
    with pytest.raises(DraError):
        ops.gauss_head_bwd(zt, st, at, glt, get, dstd=dview)
    spec, full, view = _head_buffers(dev, n, a)
    assert lib.dra_gauss_head_fwd.raw(ptr(zt), ptr(st), ptr(at), n, a, ptr(view["mean"]), ptr(view["log_pi_a"]), ptr(view["entropy"]),
                                      stream_ptr()) == EINVAL
    assert lib.dra_gauss_head_bwd.raw(ptr(zt), ptr(st), ptr(at), ptr(glt), ptr(get), n, a, ptr(view["dz"]), ptr(view["dstd"]),
                                      stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(dfull).all() and all(torch.isnan(v).all() for v in full.values())
    # one dimension fewer is served
    mean, lp, ent = ops.gauss_head_fwd(zt[:, :64].contiguous(), st[:64].contiguous(), at[:, :64].contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(mean).all() and torch.isfinite(lp).all() and torch.isfinite(ent).all()
