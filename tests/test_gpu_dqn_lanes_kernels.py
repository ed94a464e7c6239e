"""The seed-lane kernels (csrc/dqn_mlp.hip: dra_dqn_mlp_act_lanes, dra_dqn_mlp_update_lanes; csrc/optim.hip:
dra_clip_rmsprop_step_lanes, dra_copy_f32_lanes) against the single entries on copies of the same buffers.  A lane runs the single
launch's arithmetic, so every comparison is bit for bit, guard elements behind every buffer included; a tolerance would hide a
lane-indexing bug."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch
from feature_kernel_harness import GATE, GUARD, dra, _bits, _flat, _guarded      # noqa: F401  (dra: the fixture)

import dqn_feature_cases as K
import dqn_feature_restatement as R

pytestmark = pytest.mark.gpu

EINVAL = -22
NAN = float("nan")


def _same(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _net(dev, hidden, gate, seed):
    """-> (dra_q_mlp_net, the two flat buffers it points to): online parameters of `seed`, the target's of another."""
    from deeprl_amd import dqn_mlp
    flat, offs = _flat(R.KEYS, _params(hidden, seed), False)
    tflat, _ = _flat(R.KEYS, _params(hidden, seed + 50000), False)
    flat, tflat = torch.from_numpy(flat).to(dev), torch.from_numpy(tflat).to(dev)
    net = dqn_mlp.Net()
    net.param, net.target = flat.data_ptr(), tflat.data_ptr()
    net.w1, net.b1, net.w2, net.b2, net.wq, net.bq = [offs[k] for k in R.KEYS]
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, hidden, GATE[gate]
    return net, (flat, tflat)


@functools.lru_cache(maxsize=None)
def _params(hidden, seed):
    return R.init_params(hidden, seed)


def _table(cls, structs):
    from deeprl_amd.seed_batch import LaneTable
    t = LaneTable(cls, len(structs))
    for k, s in enumerate(structs):
        t.rows[k] = s
    return t


# ------------------------------------------------------------------------------------------ acting
CAP, HORIZON, EP_CAP, EP_COUNT0, STEP0 = 12, 200, 8, 6, 9
WRAP_LANE, END_LANE = 1, 2       # the lane whose first slot is the ring's last; the lane one step from its horizon


@functools.lru_cache(maxsize=None)
def _act_lane_host(lane, t_len):
    """Lane `lane`'s start as host arrays: its own environment seed, flags and random actions."""
    env, raw = K.make_env(500 + 7 * lane, HORIZON)
    rs = np.random.RandomState(900 + lane)
    explore, rand = (rs.rand(t_len) < 0.5).astype(np.uint8), rs.randint(2, size=t_len).astype(np.int64)
    end = lane == END_LANE
    return dict(raw=raw.copy(), seed=env.seed, explore=explore, rand=rand, slot0=CAP - 1 if lane == WRAP_LANE else lane,
                ep_steps=HORIZON - 1 if end else 0, counter=HORIZON - 1 if end else 0, ep_return=float(HORIZON - 1) if end else 0.0)


ACT_SPEC = dict(env_state=((1, 4), torch.float64, NAN), env_counter=((1,), torch.int64, -7), ep_steps=((1,), torch.int32, -7),
                ep_return=((1,), torch.float64, NAN), env_seed=((1,), torch.int64, -7), step=((1,), torch.int64, -7),
                ep_count=((1,), torch.int64, -7), ep_ring=((EP_CAP, 3), torch.float64, NAN), slot0=((1,), torch.int64, -7),
                frames=((CAP, 4), torch.float64, NAN), actions=((CAP,), torch.int64, -1), rewards=((CAP,), torch.float64, NAN),
                masks=((CAP,), torch.int32, -1), err=((1,), torch.int32, -7))


def _act_lane(dev, lane, t_len):
    """-> (dra_dqn_mlp_act_io of lane `lane` over fresh guarded buffers, the buffers' full tensors by name)."""
    from deeprl_amd import dqn_mlp
    h = _act_lane_host(lane, t_len)
    spec = dict(ACT_SPEC, explore=((t_len,), torch.uint8, 9), random_action=((t_len,), torch.int64, -7),
                q=((t_len, 2), torch.float32, NAN), action=((t_len,), torch.int64, -7))
    full, v = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], v[k] = _guarded(shape, dt, dev, fill)
    v["env_state"].copy_(torch.from_numpy(h["raw"]).view(1, 4))
    v["env_counter"].fill_(h["counter"]); v["ep_steps"].fill_(h["ep_steps"]); v["ep_return"].fill_(h["ep_return"]); v["err"].zero_()
    v["env_seed"].fill_(h["seed"]); v["step"].fill_(STEP0 + lane); v["ep_count"].fill_(EP_COUNT0); v["slot0"].fill_(h["slot0"])
    v["explore"].copy_(torch.from_numpy(h["explore"])); v["random_action"].copy_(torch.from_numpy(h["rand"]))
    io = dqn_mlp.ActIO()
    io.env_state, io.env_counter, io.ep_steps = v["env_state"].data_ptr(), v["env_counter"].data_ptr(), v["ep_steps"].data_ptr()
    io.ep_return, io.env_seed, io.step_counter = v["ep_return"].data_ptr(), v["env_seed"].data_ptr(), v["step"].data_ptr()
    io.ep_count, io.ep_ring = v["ep_count"].data_ptr(), v["ep_ring"].data_ptr()
    io.explore, io.random_action, io.slot0 = v["explore"].data_ptr(), v["random_action"].data_ptr(), v["slot0"].data_ptr()
    io.ring_frames, io.ring_actions = v["frames"].data_ptr(), v["actions"].data_ptr()
    io.ring_rewards, io.ring_masks = v["rewards"].data_ptr(), v["masks"].data_ptr()
    io.out_q, io.out_action, io.err = v["q"].data_ptr(), v["action"].data_ptr(), v["err"].data_ptr()
    io.horizon, io.ring_cap, io.capacity, io.reward_coef, io.t_len, io.n_env = HORIZON, EP_CAP, CAP, 1.0, t_len, 1
    return io, full


def _act_lanes_launch(dev, nets, n_lanes, t_len):
    from deeprl_amd import dqn_mlp
    from deeprl_amd._lib import lib, stream_ptr
    lanes = [_act_lane(dev, k, t_len) for k in range(n_lanes)]
    t_net, t_io = _table(dqn_mlp.Net, [n for n, _ in nets]), _table(dqn_mlp.ActIO, [io for io, _ in lanes])
    rc = lib.dra_dqn_mlp_act_lanes.raw(t_net.ptr, t_io.ptr, n_lanes, stream_ptr())
    torch.cuda.synchronize()
    return rc, [full for _, full in lanes]


@pytest.mark.parametrize("t_len", [1, 8])
@pytest.mark.parametrize("gate", ["relu", "tanh"])
@pytest.mark.parametrize("hidden", [16, 64])
@pytest.mark.parametrize("n_lanes", [1, 3, 5])
def test_act_lanes_equal_the_single_launches(dra, n_lanes, hidden, gate, t_len):
    """dra_dqn_mlp_act_lanes over lanes that differ in weights, environment seed, flags and random actions -- lane 1's first slot is
    the ring's last, so its rows wrap; lane 2's cart-pole is one step from its horizon, so it appends an episode row in its first
    transition -- against dra_dqn_mlp_act lane by lane on copies: the ring's four arrays, out_q and out_action, the environment's
    state and counters, step_counter, the episode ring and its count, err and every guard element, to the bit; no parameter
    buffer is written; a second launch from the same start gives the same bits."""
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    nets = [_net(dev, hidden, gate, 60 + k) for k in range(n_lanes)]
    before = [[t.clone() for t in keep] for _, keep in nets]
    want = []
    for k in range(n_lanes):
        io, full = _act_lane(dev, k, t_len)
        assert lib.dra_dqn_mlp_act.raw(ctypes.byref(nets[k][0]), ctypes.byref(io), stream_ptr()) == 0
        want.append(full)
    rc, got = _act_lanes_launch(dev, nets, n_lanes, t_len)
    assert rc == 0
    rc, again = _act_lanes_launch(dev, nets, n_lanes, t_len)
    assert rc == 0
    for k in range(n_lanes):
        for name in want[k]:
            _same(got[k][name], want[k][name], (k, name))
            _same(again[k][name], got[k][name], (k, name, "second launch"))
        assert int(got[k]["err"][0]) == 0 and int(got[k]["step"][0]) == STEP0 + k + t_len
        for a, b in zip(nets[k][1], before[k]):
            _same(a, b, (k, "parameters"))
        if k == END_LANE:       # the horizon's episode, stamped with the lane's own step counter, in the lane's own ring
            assert int(got[k]["ep_count"][0]) >= EP_COUNT0 + 1
            row = got[k]["ep_ring"][:3 * EP_CAP].view(EP_CAP, 3)[EP_COUNT0 % EP_CAP].cpu().numpy()
            assert row[0] == STEP0 + k and row[2] == float(HORIZON)
        if k == WRAP_LANE and t_len == 8:
            written = ~torch.isnan(got[k]["rewards"][:CAP]).cpu().numpy()
            assert written[CAP - 1] and written[:7].all() and not written[7:CAP - 1].any()
    assert n_lanes <= END_LANE or any(int(g["ep_count"][0]) == EP_COUNT0 for g in got)      # (a lane that appended nothing)


# ------------------------------------------------------------------------------------------ the update
RING_CAP = 40
BAD_LANE = 1


@functools.lru_cache(maxsize=None)
def _update_lane_host(lane, batch, bad):
    rs = np.random.RandomState(300 + lane)
    ring = dict(frames=rs.uniform(-0.5, 0.5, size=(RING_CAP, 4)), actions=rs.randint(2, size=RING_CAP).astype(np.int64),
                rewards=np.ones(RING_CAP), masks=(rs.rand(RING_CAP) < 0.8).astype(np.int32))
    idx = rs.randint(0, RING_CAP - 1, size=batch).astype(np.int64)
    if bad:
        idx[batch // 2] = RING_CAP + 5
    return ring, idx


def _update_lane(dev, net, lane, batch, double_q, bad):
    from deeprl_amd import dqn_mlp
    ring, idx = _update_lane_host(lane, batch, bad)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = [t(ring[k]) for k in ("frames", "actions", "rewards", "masks")] + [t(idx)]
    n = net[1][0].numel()
    full, v = {}, {}
    for k, shape in (("grad", (n,)), ("q_target", (batch,)), ("td", (batch,)), ("loss", (1,))):
        full[k], v[k] = _guarded(shape, torch.float32, dev, NAN)
    full["err"] = torch.zeros(1, dtype=torch.int32, device=dev)
    io = dqn_mlp.UpdateIO()
    io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks, io.idx = (x.data_ptr() for x in keep)
    io.grad, io.out_q_target, io.out_td, io.out_loss = v["grad"].data_ptr(), v["q_target"].data_ptr(), v["td"].data_ptr(), v["loss"].data_ptr()
    io.err, io.capacity, io.discount, io.batch, io.double_q = full["err"].data_ptr(), RING_CAP, K.DISCOUNT, batch, int(double_q)
    return io, full, keep


@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("gate", ["relu", "tanh"])
@pytest.mark.parametrize("hidden", [16, 64])
@pytest.mark.parametrize("batch", [1, 16, 17])
@pytest.mark.parametrize("n_lanes", [1, 3])
def test_update_lanes_equal_the_single_launches(dra, n_lanes, batch, hidden, gate, double_q):
    """dra_dqn_mlp_update_lanes over lanes with their own ring, indices, online and target parameters against dra_dqn_mlp_update lane
    by lane: the flat gradient (every element, the guard behind it), q_target, td and the loss to the bit.  With three lanes, lane
    1 carries an index outside its ring: only that lane's err counts it, and its outputs are the single entry's on the same
    indices, which clamps them."""
    from deeprl_amd import dqn_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    nets = [_net(dev, hidden, gate, 80 + k) for k in range(n_lanes)]
    bad = lambda k: n_lanes > 1 and k == BAD_LANE
    want = []
    for k in range(n_lanes):
        io, full, keep = _update_lane(dev, nets[k], k, batch, double_q, bad(k))
        assert lib.dra_dqn_mlp_update.raw(ctypes.byref(nets[k][0]), ctypes.byref(io), stream_ptr()) == 0
        want.append((full, keep))
    lanes = [_update_lane(dev, nets[k], k, batch, double_q, bad(k)) for k in range(n_lanes)]
    t_net, t_io = _table(dqn_mlp.Net, [n for n, _ in nets]), _table(dqn_mlp.UpdateIO, [io for io, _, _ in lanes])
    assert lib.dra_dqn_mlp_update_lanes.raw(t_net.ptr, t_io.ptr, n_lanes, stream_ptr()) == 0
    torch.cuda.synchronize()
    for k in range(n_lanes):
        for name in want[k][0]:
            _same(lanes[k][1][name], want[k][0][name], (k, name))
        assert int(lanes[k][1]["err"][0]) == (1 if bad(k) else 0)
        assert torch.isfinite(lanes[k][1]["grad"][:-GUARD]).all() and torch.isnan(lanes[k][1]["grad"][-GUARD:]).all()
    if n_lanes > 1:     # (the lanes computed different things: a lane that read another lane's row would show above)
        assert not torch.equal(lanes[0][1]["grad"][:-GUARD], lanes[2][1]["grad"][:-GUARD])


# ------------------------------------------------------------------------------------------ clip + RMSprop
def _optim_lane_host(n, lane):
    rs = np.random.RandomState(40 + lane)
    scale = (1.0, 1e-3, 0.0)[lane]          # a norm above max_norm 5 (about sqrt(n)), one below, an all-zero gradient
    return rs.randn(n).astype(np.float32), [(rs.randn(n) * scale).astype(np.float32) for _ in range(2)]


@pytest.mark.parametrize("max_norm", [5, None])
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("n", [386, 388, 4610])
def test_step_lanes_equal_the_fused_optimizer(dra, n, centered, max_norm):
    """dra_clip_rmsprop_step_lanes over three lanes -- a gradient norm above max_norm, one below it, an all-zero gradient -- against
    FusedOptimizer.step (dra_grad_sqnorm + dra_rmsprop_step) on copies, two steps in a row (the second over running averages that
    are no longer zero): parameters, both state buffers and out_norm per lane to the bit, the guards behind them intact.  n: the
    parameter counts of hidden 16 (386: a tail of 2 floats; 388 as the optimiser's flat buffer pads it) and hidden 64 (4 610: three
    step workgroups, five norm partials that are not zero).  max_norm None: no clipping, out_norm is left alone."""
    from deeprl_amd import seed_batch
    from deeprl_amd._lib import lib, stream_ptr
    from deeprl_amd.optim import FusedOptimizer
    dev = dra.Config.DEVICE
    hyper = dict(lr=0.01, alpha=0.95, eps=0.01, centered=centered)
    singles, lanes, rows = [], [], []
    for k in range(3):
        p0, grads = _optim_lane_host(n, k)
        flat = types.SimpleNamespace(flat=torch.from_numpy(p0).to(dev), grad=torch.zeros(n, dtype=torch.float32, device=dev), numel=n)
        singles.append((FusedOptimizer(flat, 'rmsprop', hyper), grads))
        full, v = {}, {}
        for name in ("param", "grad", "sq", "ga"):
            full[name], v[name] = _guarded((n,), torch.float32, dev, NAN)
            v[name].zero_()
        full["norm"], v["norm"] = _guarded((1,), torch.float32, dev, NAN)
        v["norm"].zero_()
        v["param"].copy_(torch.from_numpy(p0))
        o = seed_batch.OptimLane()
        o.param, o.grad, o.square_avg, o.grad_avg = v["param"].data_ptr(), v["grad"].data_ptr(), v["sq"].data_ptr(), v["ga"].data_ptr()
        o.out_norm, o.n = v["norm"].data_ptr(), n
        rows.append(o)
        lanes.append((full, v))
    table = _table(seed_batch.OptimLane, rows)
    for s in range(2):
        for k in range(3):
            opt, grads = singles[k]
            opt.flat.grad.copy_(torch.from_numpy(grads[s]))
            opt.step(max_norm)
            lanes[k][1]["grad"].copy_(torch.from_numpy(grads[s]))
        assert lib.dra_clip_rmsprop_step_lanes.raw(table.ptr, 3, float(max_norm or 0.0), hyper['lr'], hyper['alpha'], hyper['eps'],
                                                   int(centered), stream_ptr()) == 0
        torch.cuda.synchronize()
        for k in range(3):
            opt, (full, v) = singles[k][0], lanes[k]
            _same(v["param"], opt.flat.flat, (s, k, "param"))
            _same(v["sq"], opt.state1, (s, k, "square_avg"))
            _same(v["ga"], opt.state2, (s, k, "grad_avg"))
            _same(v["norm"], opt.norm, (s, k, "norm"))
            assert all(torch.isnan(full[name][-GUARD:]).all() for name in full)
    norms = [float(lanes[k][1]["norm"][0]) for k in range(3)]
    if max_norm:
        assert norms[0] > max_norm > norms[1] > 0 and norms[2] == 0
        _same(lanes[2][1]["param"], torch.from_numpy(_optim_lane_host(n, 2)[0]), "a zero gradient moves nothing")
    else:
        assert norms == [0, 0, 0]
    assert not centered or float(lanes[0][1]["ga"].abs().max()) > 0


def test_copy_lanes(dra):
    """dra_copy_f32_lanes: dst[i] = src[i], i < n, per lane (lengths that differ, one of them 0), nothing behind n."""
    from deeprl_amd import seed_batch
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    rows, bufs = [], []
    for k, n in enumerate((4610, 0, 388, 257)):
        src = torch.randn(n + 3, device=dev)
        full, dst = _guarded((n,), torch.float32, dev, NAN)
        c = seed_batch.CopyLane()
        c.dst, c.src, c.n = full.data_ptr(), src.data_ptr(), n
        rows.append(c)
        bufs.append((src, full, n))
    table = _table(seed_batch.CopyLane, rows)
    assert lib.dra_copy_f32_lanes.raw(table.ptr, len(rows), stream_ptr()) == 0
    torch.cuda.synchronize()
    for src, full, n in bufs:
        assert torch.equal(full[:n], src[:n]) and torch.isnan(full[n:]).all()


# ------------------------------------------------------------------------------------------ refusals
def test_lane_entries_refuse_and_write_nothing(dra):
    """n_lanes 0 and 65, a null table, and a lane with a hidden width the kernels are not built for: DRA_EINVAL from every lane
    entry, and the canary-filled outputs of EVERY lane -- the supported ones included -- are as they were."""
    from deeprl_amd import dqn_mlp, seed_batch
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    nets = [_net(dev, 16, "relu", 70 + k) for k in range(3)]
    odd = dqn_mlp.Net.from_buffer_copy(bytes(nets[1][0]))
    odd.hidden = 48
    t_net, t_odd = _table(dqn_mlp.Net, [n for n, _ in nets]), _table(dqn_mlp.Net, [nets[0][0], odd, nets[2][0]])
    acts = [_act_lane(dev, k, 4) for k in range(3)]
    ups = [_update_lane(dev, nets[k], k, 10, False, False) for k in range(3)]
    t_act, t_up = _table(dqn_mlp.ActIO, [io for io, _ in acts]), _table(dqn_mlp.UpdateIO, [io for io, _, _ in ups])
    n = 388
    opt_bufs = [[torch.full((n,), 3.0, device=dev) for _ in range(4)] + [torch.full((1,), 3.0, device=dev)] for _ in range(3)]
    rows = []
    for b in opt_bufs:
        o = seed_batch.OptimLane()
        o.param, o.grad, o.square_avg, o.grad_avg, o.out_norm = (x.data_ptr() for x in b)
        o.n = n
        rows.append(o)
    t_opt = _table(seed_batch.OptimLane, rows)
    short = seed_batch.OptimLane.from_buffer_copy(bytes(rows[1]))
    short.n = 384
    t_opt_odd = _table(seed_batch.OptimLane, [rows[0], short, rows[2]])
    copies = []
    for b in opt_bufs:
        c = seed_batch.CopyLane()
        c.dst, c.src, c.n = b[2].data_ptr(), b[0].data_ptr(), n
        copies.append(c)
    t_copy = _table(seed_batch.CopyLane, copies)
    outputs = [t for _, full in acts for t in full.values()] + [t for _, full, _ in ups for t in full.values()] + [t for b in opt_bufs for t in b]
    before = [t.clone() for t in outputs]
    s = stream_ptr()
    null = ctypes.c_void_p(None)
    calls = []
    for bad_n in (0, 65, -1):
        calls += [lib.dra_dqn_mlp_act_lanes.raw(t_net.ptr, t_act.ptr, bad_n, s), lib.dra_dqn_mlp_update_lanes.raw(t_net.ptr, t_up.ptr, bad_n, s),
                  lib.dra_clip_rmsprop_step_lanes.raw(t_opt.ptr, bad_n, 5.0, 0.01, 0.99, 1e-8, 0, s), lib.dra_copy_f32_lanes.raw(t_copy.ptr, bad_n, s)]
    calls += [lib.dra_dqn_mlp_act_lanes.raw(null, t_act.ptr, 3, s), lib.dra_dqn_mlp_act_lanes.raw(t_net.ptr, null, 3, s),
              lib.dra_dqn_mlp_update_lanes.raw(null, t_up.ptr, 3, s), lib.dra_dqn_mlp_update_lanes.raw(t_net.ptr, null, 3, s),
              lib.dra_clip_rmsprop_step_lanes.raw(null, 3, 5.0, 0.01, 0.99, 1e-8, 0, s), lib.dra_copy_f32_lanes.raw(null, 3, s),
              lib.dra_dqn_mlp_act_lanes.raw(t_odd.ptr, t_act.ptr, 3, s), lib.dra_dqn_mlp_update_lanes.raw(t_odd.ptr, t_up.ptr, 3, s),
              lib.dra_clip_rmsprop_step_lanes.raw(t_opt_odd.ptr, 3, 5.0, 0.01, 0.99, 1e-8, 0, s)]
    torch.cuda.synchronize()
    assert calls == [EINVAL] * len(calls)
    for t, b in zip(outputs, before):
        _same(t, b, "a refused launch wrote")
    sup = lib.dra_dqn_mlp_lanes_supported.raw
    assert sup(4, 2, 16, 4, 10, 1, 1) == 0 and sup(4, 2, 64, 8, 256, 2, 64) == 0
    assert all(sup(*a) == EINVAL for a in ((4, 2, 16, 4, 10, 1, 0), (4, 2, 16, 4, 10, 1, 65), (4, 2, 48, 4, 10, 1, 3), (4, 2, 16, 9, 10, 1, 3),
                                           (4, 2, 16, 4, 257, 1, 3), (4, 2, 16, 4, 10, 3, 3)))
