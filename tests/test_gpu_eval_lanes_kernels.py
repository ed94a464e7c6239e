"""The evaluation lane launches (csrc/dqn_mlp.hip: dra_dqn_mlp_eval_lanes; csrc/dist_mlp.hip: dra_dist_mlp_eval_lanes; both over
dra_mlp_eval_io tables) against the single entries dra_dqn_mlp_eval / dra_dist_mlp_eval on copies of the same buffers.  A lane runs
the single launch's text, so every comparison is bit for bit, guard elements behind every buffer included; a tolerance would hide
a lane-indexing bug.  Lane l has its own parameters (the case's parameter seed + l), its own environment seed (ENV_SEED + 7 l) and
the launch shape eval_cases.LAUNCHES[l % 4], so one batch mixes horizon 12 with horizon 1, one episode with five and a junk start
with a clean one: lanes end at different steps."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from feature_kernel_harness import GUARD, dra, _bits, _guarded      # noqa: F401  (dra: the fixture)
from test_gpu_dist_feature import _net_struct as _dist_net
from test_gpu_dqn_feature import _net_struct as _dqn_net

import dist_feature_restatement as DR
import dqn_feature_restatement as QR
import eval_cases as C

pytestmark = pytest.mark.gpu

EINVAL = -22
NAN = float("nan")
LANE_CASES = tuple(c for c in C.CASES if c[0] in ("dqn", "dist"))
SHAPES = tuple(C.LAUNCHES)          # lane l runs LAUNCHES[SHAPES[l % 4]]
assert len(LANE_CASES) == 8 and len(SHAPES) == 4      # every dqn and dist case of eval_cases.CASES: four each


@functools.lru_cache(maxsize=None)
def _params(case, lane):
    kind, hidden, seed = case[0], case[1], case[6] + lane
    return QR.init_params(hidden, seed=seed) if kind == "dqn" else DR.init_params(hidden, seed, C.spec_of(case))


def _entries(case):
    from deeprl_amd import dist_mlp, dqn_mlp
    from deeprl_amd._lib import lib
    if case[0] == "dqn":
        return dqn_mlp.Net, lib.dra_dqn_mlp_eval, lib.dra_dqn_mlp_eval_lanes
    return dist_mlp.Net, lib.dra_dist_mlp_eval, lib.dra_dist_mlp_eval_lanes


def _net(dev, case, lane, hidden=None):
    """-> (net struct of lane `lane`, the device tensors it points to)."""
    kind, gate = case[0], case[2]
    hidden = case[1] if hidden is None else hidden
    params = _params(case[:1] + (hidden,) + case[2:], lane)
    if kind == "dqn":
        net, flat, tflat, _ = _dqn_net(params, None, dev, hidden, gate, hidden == 16)
    else:
        net, flat, tflat, _ = _dist_net(params, None, dev, C.spec_of(case), hidden, gate, hidden == 16)
    return net, (flat, tflat)


def _io(dev, lane):
    """-> (dra_mlp_eval_io of lane `lane` over fresh guarded buffers, the buffers' full tensors by name).  Odd lanes pass a null
    out_q: their q buffer is allocated all the same and must stay as it is."""
    from deeprl_amd import dqn_mlp
    n_episodes, horizon, junk, _ = C.LAUNCHES[SHAPES[lane % 4]]
    spec = dict(env_state=((1, 4), torch.float64, NAN), env_counter=((1,), torch.int64, -7), ep_steps=((1,), torch.int32, -7),
                ep_return=((1,), torch.float64, NAN), env_seed=((1,), torch.int64, -7), out_return=((n_episodes,), torch.float64, NAN),
                out_length=((n_episodes,), torch.int32, -7), out_steps=((1,), torch.int64, -7),
                out_q=((n_episodes * horizon, 2), torch.float32, NAN))
    full, v = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], v[k] = _guarded(shape, dt, dev, fill)
    j = C.JUNK
    v["env_state"].copy_(torch.tensor([j["state"]], dtype=torch.float64))       # (a reset at the counter replaces it either way)
    v["env_counter"].fill_(j["counter"] if junk else 0)
    v["ep_steps"].fill_(j["ep_steps"] if junk else 0)
    v["ep_return"].fill_(j["ep_return"] if junk else 0.0)
    v["env_seed"].fill_(C.ENV_SEED + 7 * lane)
    io = dqn_mlp.EvalIO()
    for k in spec:
        if k != "out_q" or lane % 2 == 0:
            setattr(io, k, v[k].data_ptr())
    io.horizon, io.n_episodes = horizon, n_episodes
    return io, full


def _table(cls, structs):
    from deeprl_amd.seed_batch import LaneTable
    t = LaneTable(cls, len(structs))
    for k, s in enumerate(structs):
        t.rows[k] = s
    return t


def _host(full):
    return {k: t.cpu().numpy() for k, t in full.items()}


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _lanes_launch(dev, case, nets, n_lanes):
    net_cls, _, lanes_fn = _entries(case)
    from deeprl_amd import dqn_mlp
    from deeprl_amd._lib import stream_ptr
    ios = [_io(dev, l) for l in range(n_lanes)]
    t_net, t_io = _table(net_cls, [n for n, _ in nets]), _table(dqn_mlp.EvalIO, [io for io, _ in ios])
    rc = lanes_fn.raw(t_net.ptr, t_io.ptr, n_lanes, stream_ptr())
    torch.cuda.synchronize()
    return rc, [_host(full) for _, full in ios]


@pytest.mark.parametrize("n_lanes", [1, 3, 64])
@pytest.mark.parametrize("case", LANE_CASES, ids=C.case_id)
def test_eval_lanes_equal_the_single_launches(dra, case, n_lanes):
    """dra_*_mlp_eval_lanes against dra_*_mlp_eval lane by lane on copies: returns, lengths, the step count, the environment's
    words and its counter, out_q (untouched on the odd lanes, whose out_q is null) and every guard element, to the bit; the
    parameter buffers are not written; a second lane launch from the same start gives the same bits.  The condition, on the SINGLE
    launches' outputs: among the lanes of one launch shape no two have equal (returns, lengths, final state), and at least two
    lanes of the batch differ in out_steps -- otherwise a lane that read another lane's row could pass."""
    from deeprl_amd._lib import stream_ptr
    dev = dra.Config.DEVICE
    _, single_fn, _ = _entries(case)
    nets = [_net(dev, case, l) for l in range(n_lanes)]
    before = [[t.clone() for t in keep] for _, keep in nets]
    want = []
    for l in range(n_lanes):
        io, full = _io(dev, l)
        start = _host(full)
        assert single_fn.raw(ctypes.byref(nets[l][0]), ctypes.byref(io), stream_ptr()) == 0
        torch.cuda.synchronize()
        want.append(_host(full))
        if l % 2:
            _same(want[l]["out_q"], start["out_q"], (l, "the single launch wrote q through a null out_q"))
    # ---- the condition, on the reference side
    steps = [int(w["out_steps"][0]) for w in want]
    for shape in range(4):
        keys = [(want[l]["out_return"].tobytes(), want[l]["out_length"].tobytes(), want[l]["env_state"].tobytes(),
                 want[l]["env_counter"].tobytes()) for l in range(shape, n_lanes, 4)]
        assert len(set(keys)) == len(keys), ("two lanes of launch shape %s are indistinguishable" % SHAPES[shape])
    assert n_lanes == 1 or len(set(steps)) > 1, steps
    for l in range(n_lanes):
        n_episodes, horizon = C.LAUNCHES[SHAPES[l % 4]][:2]
        assert n_episodes <= steps[l] <= n_episodes * horizon and steps[l] == int(want[l]["out_length"][:n_episodes].sum())
    # ---- the lane launch, twice
    rc, got = _lanes_launch(dev, case, nets, n_lanes)
    assert rc == 0
    rc, again = _lanes_launch(dev, case, nets, n_lanes)
    assert rc == 0
    for l in range(n_lanes):
        for name in want[l]:
            _same(got[l][name], want[l][name], (l, name))
            _same(again[l][name], got[l][name], (l, name, "second launch"))
        for a, b in zip(nets[l][1], before[l]):
            _same(a.cpu().numpy(), b.cpu().numpy(), (l, "parameters"))
        q = got[l]["out_q"]         # (flat: [n_episodes * horizon][2], then the guard)
        if l % 2:
            assert np.isnan(q).all()
        else:
            assert np.isfinite(q[:2 * steps[l]]).all() and np.isnan(q[2 * steps[l]:]).all()


REFUSED = ("no_lanes", "too_many_lanes", "negative_lanes", "null_nets", "null_ios", "null_returns", "too_many_steps", "other_hidden")


@pytest.mark.parametrize("case", [LANE_CASES[0], LANE_CASES[4]], ids=C.case_id)
def test_refused_lane_launches_write_nothing(dra, case):
    """n_lanes 0, 65 and -1, a null table, and ONE lane of three that the single entry refuses -- a null out_return,
    n_episodes * horizon = 65537 -- or whose hidden size is not lane 0's (16 among 64: a net the single entry takes): DRA_EINVAL,
    and every buffer of EVERY lane, the good ones included, is as it was."""
    from deeprl_amd import dqn_mlp
    from deeprl_amd._lib import stream_ptr
    dev, s = dra.Config.DEVICE, stream_ptr()
    net_cls, single_fn, lanes_fn = _entries(case)
    nets = [_net(dev, case, l) for l in range(3)]
    small = _net(dev, case, 1, hidden=16)
    ios = [_io(dev, l) for l in range(3)]
    everything = [t for _, full in ios for t in full.values()] + [t for _, keep in nets + [small] for t in keep]
    before = [t.clone() for t in everything]
    rows = [io for io, _ in ios]
    no_returns = dqn_mlp.EvalIO.from_buffer_copy(bytes(rows[1]))
    no_returns.out_return = None
    long = dqn_mlp.EvalIO.from_buffer_copy(bytes(rows[1]))
    long.n_episodes, long.horizon = 1, 65537
    t_net, t_io = _table(net_cls, [n for n, _ in nets]), _table(dqn_mlp.EvalIO, rows)
    t_odd = _table(net_cls, [nets[0][0], small[0], nets[2][0]])
    t_no_returns, t_long = _table(dqn_mlp.EvalIO, [rows[0], no_returns, rows[2]]), _table(dqn_mlp.EvalIO, [rows[0], long, rows[2]])
    null = ctypes.c_void_p(None)
    calls = dict(no_lanes=(t_net.ptr, t_io.ptr, 0), too_many_lanes=(t_net.ptr, t_io.ptr, 65), negative_lanes=(t_net.ptr, t_io.ptr, -1),
                 null_nets=(null, t_io.ptr, 3), null_ios=(t_net.ptr, null, 3), null_returns=(t_net.ptr, t_no_returns.ptr, 3),
                 too_many_steps=(t_net.ptr, t_long.ptr, 3), other_hidden=(t_odd.ptr, t_io.ptr, 3))
    assert set(calls) == set(REFUSED)
    got = {what: lanes_fn.raw(*args, s) for what, args in calls.items()}
    torch.cuda.synchronize()
    assert got == {what: EINVAL for what in REFUSED}
    for t, b in zip(everything, before):
        _same(t.cpu().numpy(), b.cpu().numpy(), "a refused launch wrote")
    # (the odd lane's net is one the single entry takes: the refusal above is same_shape's)
    io, _ = _io(dev, 1)
    assert single_fn.raw(ctypes.byref(small[0]), ctypes.byref(io), s) == 0
    # (and the tables themselves are good: the same three lanes launch)
    assert lanes_fn.raw(t_net.ptr, t_io.ptr, 3, s) == 0
    torch.cuda.synchronize()


def test_lanes_supported_table(dra):
    from deeprl_amd._lib import lib
    ok = lib.dra_mlp_eval_lanes_supported.raw
    assert ok(10, 200, 64) == 0 and ok(10, 200, 1) == 0
    assert ok(10, 200, 65) == EINVAL and ok(257, 12, 4) == EINVAL and ok(1, 65537, 1) == EINVAL and ok(10, 200, 0) == EINVAL
