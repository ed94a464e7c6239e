"""The distributional seed-lane kernels (csrc/dist_mlp.hip: dra_dist_mlp_act_lanes, dra_dist_mlp_update_lanes) against the single
entries dra_dist_mlp_act / dra_dist_mlp_update on copies of the same buffers.  A lane runs the single launch's text on the same data,
so every comparison is bit for bit, guard elements behind every buffer included: the tolerance is zero, and a difference is a
lane-indexing bug.  (The single entries themselves are held to the fp64 restatement by tests/test_gpu_dist_feature.py.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch
from feature_kernel_harness import GATE, GUARD, dra, _bits, _flat, _guarded      # noqa: F401  (dra: the fixture)

import dist_feature_cases as K
import dist_feature_restatement as R

pytestmark = pytest.mark.gpu

EINVAL = -22
NAN = float("nan")
# (head, atoms per action): the smallest count and each head's largest in use (51: the kernels' cap; 20: the entry's quantiles)
HEADS = (("c51", 2), ("c51", 51), ("qr", 2), ("qr", 20))


def _same(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _spec(head, n, lane=0):
    """The head's spec; a categorical lane's support is its own (v_min / v_max are per-lane data): lane 0's times 1 + lane / 2."""
    lo, hi = K.SUPPORT[n] if n in K.SUPPORT else (-10.0, 10.0)
    return K.spec_of(head, n, (lo * (1 + lane / 2), hi * (1 + lane / 2)))


@functools.lru_cache(maxsize=None)
def _params(head, n, hidden, seed):
    return R.init_params(hidden, seed, _spec(head, n))


def _net(dev, head, n, hidden, gate, seed, lane=0):
    """-> (dra_dist_mlp_net, the two flat buffers it points to): online parameters of `seed`, the target's of another."""
    from deeprl_amd import dist_mlp
    spec = _spec(head, n, lane)
    flat, offs = _flat(R.keys(head), _params(head, n, hidden, seed), False)
    tflat, _ = _flat(R.keys(head), _params(head, n, hidden, seed + 50000), False)
    flat, tflat = torch.from_numpy(flat).to(dev), torch.from_numpy(tflat).to(dev)
    net = dist_mlp.Net()
    net.param, net.target = flat.data_ptr(), tflat.data_ptr()
    net.w1, net.b1, net.w2, net.b2, net.wq, net.bq = [offs[k] for k in R.keys(head)]
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, hidden, GATE[gate]
    net.head, net.n_atoms, net.v_min, net.v_max = K.HEAD_CODE[head], n, spec["v_min"], spec["v_max"]
    return net, (flat, tflat)


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
    return dict(raw=raw.copy(), seed=env.seed, explore=explore, rand=rand, slot0=CAP - 1 if lane == WRAP_LANE else lane % CAP,
                ep_steps=HORIZON - 1 if end else 0, counter=HORIZON - 1 if end else 0, ep_return=float(HORIZON - 1) if end else 0.0)


ACT_SPEC = dict(env_state=((1, 4), torch.float64, NAN), env_counter=((1,), torch.int64, -7), ep_steps=((1,), torch.int32, -7),
                ep_return=((1,), torch.float64, NAN), env_seed=((1,), torch.int64, -7), step=((1,), torch.int64, -7),
                ep_count=((1,), torch.int64, -7), ep_ring=((EP_CAP, 3), torch.float64, NAN), slot0=((1,), torch.int64, -7),
                frames=((CAP, 4), torch.float64, NAN), actions=((CAP,), torch.int64, -1), rewards=((CAP,), torch.float64, NAN),
                masks=((CAP,), torch.int32, -1), err=((1,), torch.int32, -7))


def _act_lane(dev, lane, t_len):
    """-> (dra_dqn_mlp_act_io of lane `lane` over fresh guarded buffers, the buffers' full tensors by name)."""
    from deeprl_amd import dist_mlp
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
    io = dist_mlp.ActIO()
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
    from deeprl_amd import dist_mlp
    from deeprl_amd._lib import lib, stream_ptr
    lanes = [_act_lane(dev, k, t_len) for k in range(n_lanes)]
    t_net, t_io = _table(dist_mlp.Net, [n for n, _ in nets]), _table(dist_mlp.ActIO, [io for io, _ in lanes])
    rc = lib.dra_dist_mlp_act_lanes.raw(t_net.ptr, t_io.ptr, n_lanes, stream_ptr())
    torch.cuda.synchronize()
    return rc, [full for _, full in lanes]


@pytest.mark.parametrize("t_len", [1, 8])
@pytest.mark.parametrize("head, n", HEADS)
@pytest.mark.parametrize("gate", ["relu", "tanh"])
@pytest.mark.parametrize("hidden", [16, 64])
@pytest.mark.parametrize("n_lanes", [1, 3])
def test_act_lanes_equal_the_single_launches(dra, n_lanes, hidden, gate, head, n, t_len):
    """dra_dist_mlp_act_lanes over lanes that differ in weights, categorical support, environment seed, flags and random actions --
    lane 1's first slot is the ring's last, so its rows wrap; lane 2's cart-pole is one step from its horizon, so it appends an
    episode row in its first transition -- against dra_dist_mlp_act lane by lane on copies: the ring's four arrays, out_q and
    out_action, the environment's state and counters, step_counter, the episode ring and its count, err and every guard element,
    to the bit; no parameter buffer is written; a second launch from the same start gives the same bits."""
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    nets = [_net(dev, head, n, hidden, gate, 60 + k, lane=k) for k in range(n_lanes)]
    before = [[t.clone() for t in keep] for _, keep in nets]
    want = []
    for k in range(n_lanes):
        io, full = _act_lane(dev, k, t_len)
        assert lib.dra_dist_mlp_act.raw(ctypes.byref(nets[k][0]), ctypes.byref(io), stream_ptr()) == 0
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
        assert torch.isfinite(got[k]["q"][:2 * t_len]).all()
        for a, b in zip(nets[k][1], before[k]):
            _same(a, b, (k, "parameters"))
        if k == END_LANE:       # the horizon's episode, stamped with the lane's own step counter, in the lane's own ring
            assert int(got[k]["ep_count"][0]) >= EP_COUNT0 + 1
            row = got[k]["ep_ring"][:3 * EP_CAP].view(EP_CAP, 3)[EP_COUNT0 % EP_CAP].cpu().numpy()
            assert row[0] == STEP0 + k and row[2] == float(HORIZON)
        if k == WRAP_LANE and t_len == 8:
            written = ~torch.isnan(got[k]["rewards"][:CAP]).cpu().numpy()
            assert written[CAP - 1] and written[:7].all() and not written[7:CAP - 1].any()
    if n_lanes > 1:      # (a lane that appended nothing; lanes that computed different things)
        assert int(got[0]["ep_count"][0]) == EP_COUNT0
        assert not torch.equal(got[0]["q"][:2 * t_len], got[1]["q"][:2 * t_len])


# ------------------------------------------------------------------------------------------ the update
RING_CAP = 40
BAD_LANE = 1
# (hidden, gate, atoms by head): the smallest network with the smallest heads, the largest with each head's largest
UPDATE_NETS = ((16, "tanh", dict(c51=2, qr=2)), (64, "relu", dict(c51=51, qr=20)))


@functools.lru_cache(maxsize=None)
def _update_lane_host(lane, batch, bad):
    rs = np.random.RandomState(300 + lane)
    ring = dict(frames=rs.uniform(-0.5, 0.5, size=(RING_CAP, 4)), actions=rs.randint(2, size=RING_CAP).astype(np.int64),
                rewards=np.ones(RING_CAP), masks=(rs.rand(RING_CAP) < 0.8).astype(np.int32))
    idx = rs.randint(0, RING_CAP - 1, size=batch).astype(np.int64)
    if bad:
        idx[batch // 2] = RING_CAP + 5
    return ring, idx


def _update_lane(dev, net, head, n, lane, batch, double_q, bad):
    """-> (dra_dist_mlp_update_io of lane `lane` over fresh guarded outputs, the outputs' full tensors by name, what it reads)."""
    from deeprl_amd import dist_mlp
    ring, idx = _update_lane_host(lane, batch, bad)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = [t(ring[k]) for k in ("frames", "actions", "rewards", "masks")] + [t(idx)]
    full, v = {}, {}
    shapes = dict(grad=(net[1][0].numel(),), loss=(1,), loss_vec=(batch if head == "c51" else n,), q_next=(batch, 2), target=(batch, n))
    for k, shape in shapes.items():
        full[k], v[k] = _guarded(shape, torch.float32, dev, NAN)
    full["err"] = torch.zeros(1, dtype=torch.int32, device=dev)
    io = dist_mlp.UpdateIO()
    io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks, io.idx = (x.data_ptr() for x in keep)
    io.grad, io.out_loss, io.out_loss_vec = v["grad"].data_ptr(), v["loss"].data_ptr(), v["loss_vec"].data_ptr()
    io.out_q_next, io.out_target = v["q_next"].data_ptr(), v["target"].data_ptr()
    io.err, io.capacity, io.discount, io.batch, io.double_q = full["err"].data_ptr(), RING_CAP, K.DISCOUNT, batch, int(double_q)
    return io, full, keep


@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("head", K.HEADS)
@pytest.mark.parametrize("hidden, gate, atoms", UPDATE_NETS, ids=lambda v: str(v) if not isinstance(v, dict) else "n%d_%d" % (v["c51"], v["qr"]))
@pytest.mark.parametrize("batch", [1, 16, 17])
@pytest.mark.parametrize("n_lanes", [1, 3])
def test_update_lanes_equal_the_single_launches(dra, n_lanes, batch, hidden, gate, atoms, head, double_q):
    """dra_dist_mlp_update_lanes over lanes with their own ring, indices, support, online and target parameters against
    dra_dist_mlp_update lane by lane (batches at and around the row block of 16): the flat gradient (every element, the guard behind
    it), the loss, loss_vec, q_next and the target to the bit.  With three lanes, lane 1 carries an index outside its ring: only
    that lane's err counts it, and its outputs are the single entry's on the same indices, which clamps them."""
    from deeprl_amd import dist_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    n = atoms[head]
    nets = [_net(dev, head, n, hidden, gate, 80 + k, lane=k) for k in range(n_lanes)]
    bad = lambda k: n_lanes > 1 and k == BAD_LANE
    want = []
    for k in range(n_lanes):
        io, full, keep = _update_lane(dev, nets[k], head, n, k, batch, double_q, bad(k))
        assert lib.dra_dist_mlp_update.raw(ctypes.byref(nets[k][0]), ctypes.byref(io), stream_ptr()) == 0
        want.append((full, keep))
    lanes = [_update_lane(dev, nets[k], head, n, k, batch, double_q, bad(k)) for k in range(n_lanes)]
    t_net, t_io = _table(dist_mlp.Net, [x for x, _ in nets]), _table(dist_mlp.UpdateIO, [io for io, _, _ in lanes])
    assert lib.dra_dist_mlp_update_lanes.raw(t_net.ptr, t_io.ptr, n_lanes, stream_ptr()) == 0
    torch.cuda.synchronize()
    for k in range(n_lanes):
        for name in want[k][0]:
            _same(lanes[k][1][name], want[k][0][name], (k, name))
        assert int(lanes[k][1]["err"][0]) == (1 if bad(k) else 0)
        for name in ("grad", "loss", "loss_vec", "q_next", "target"):
            assert torch.isfinite(lanes[k][1][name][:-GUARD]).all() and torch.isnan(lanes[k][1][name][-GUARD:]).all(), (k, name)
    if n_lanes > 1:     # (the lanes computed different things: a lane that read another lane's row would show above)
        assert not torch.equal(lanes[0][1]["grad"][:-GUARD], lanes[2][1]["grad"][:-GUARD])


@pytest.mark.parametrize("head, n", [("c51", 51), ("qr", 20)])
def test_64_lanes_equal_the_single_launches(dra, head, n):
    """The largest launch: 64 lanes of hidden 64 (the update's workgroups hold their full LDS, one per CU), acting 4 transitions and
    updating on 10 rows, every lane against its single launches to the bit."""
    from deeprl_amd import dist_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    n_lanes = 64
    nets = [_net(dev, head, n, 64, "relu", 200 + k, lane=k % 4) for k in range(n_lanes)]
    want_act, want_up = [], []
    for k in range(n_lanes):
        io, full = _act_lane(dev, k, 4)
        assert lib.dra_dist_mlp_act.raw(ctypes.byref(nets[k][0]), ctypes.byref(io), stream_ptr()) == 0
        want_act.append(full)
        io, full, keep = _update_lane(dev, nets[k], head, n, k, 10, False, False)
        assert lib.dra_dist_mlp_update.raw(ctypes.byref(nets[k][0]), ctypes.byref(io), stream_ptr()) == 0
        want_up.append((full, keep))
    rc, got_act = _act_lanes_launch(dev, nets, n_lanes, 4)
    assert rc == 0
    ups = [_update_lane(dev, nets[k], head, n, k, 10, False, False) for k in range(n_lanes)]
    t_net, t_io = _table(dist_mlp.Net, [x for x, _ in nets]), _table(dist_mlp.UpdateIO, [io for io, _, _ in ups])
    assert lib.dra_dist_mlp_update_lanes.raw(t_net.ptr, t_io.ptr, n_lanes, stream_ptr()) == 0
    torch.cuda.synchronize()
    for k in range(n_lanes):
        for name in want_act[k]:
            _same(got_act[k][name], want_act[k][name], (k, name))
        for name in want_up[k][0]:
            _same(ups[k][1][name], want_up[k][0][name], (k, name))
        assert int(ups[k][1]["err"][0]) == 0 and int(got_act[k]["err"][0]) == 0


# ------------------------------------------------------------------------------------------ refusals
def _copy_net(net, **fields):
    from deeprl_amd import dist_mlp
    out = dist_mlp.Net.from_buffer_copy(bytes(net))
    for k, v in fields.items():
        setattr(out, k, v)
    return out


def test_lane_entries_refuse_and_write_nothing(dra):
    """n_lanes 0, 65 and -1, a null table, a lane with another atom count, another head kind or another hidden width (each a lane
    the single entry accepts, or -- hidden 48 -- refuses), and a lane the single entry refuses (a null param): DRA_EINVAL from both
    lane entries, and the canary-filled outputs of EVERY lane -- the supported ones included -- are as they were."""
    from deeprl_amd import dist_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    head, n = "c51", 20
    nets = [_net(dev, head, n, 16, "relu", 70 + k, lane=k) for k in range(3)]
    plain = [x for x, _ in nets]
    other_atoms = _net(dev, head, 21, 16, "relu", 71)           # a whole net of 21 atoms: the single entries take it
    other_hidden = _net(dev, head, n, 64, "relu", 71)
    tables = dict(ok=_table(dist_mlp.Net, plain),
                  atoms=_table(dist_mlp.Net, [plain[0], other_atoms[0], plain[2]]),
                  head=_table(dist_mlp.Net, [plain[0], _copy_net(plain[1], head=K.HEAD_CODE["qr"]), plain[2]]),
                  hidden=_table(dist_mlp.Net, [plain[0], other_hidden[0], plain[2]]),
                  hidden48=_table(dist_mlp.Net, [plain[0], _copy_net(plain[1], hidden=48), plain[2]]),
                  null_param=_table(dist_mlp.Net, [plain[0], plain[1], _copy_net(plain[2], param=None)]))
    acts = [_act_lane(dev, k, 4) for k in range(3)]
    # the update's outputs are sized for the largest lane offered above (21 atoms, hidden 64's parameter count)
    ups = [_update_lane(dev, other_hidden, head, 21, k, 10, False, False) for k in range(3)]
    t_act, t_up = _table(dist_mlp.ActIO, [io for io, _ in acts]), _table(dist_mlp.UpdateIO, [io for io, _, _ in ups])
    outputs = [t for _, full in acts for t in full.values()] + [t for _, full, _ in ups for t in full.values()]
    before = [t.clone() for t in outputs]
    s = stream_ptr()
    null = ctypes.c_void_p(None)
    act, up = lib.dra_dist_mlp_act_lanes.raw, lib.dra_dist_mlp_update_lanes.raw
    calls = []
    for bad_n in (0, 65, -1):
        calls += [act(tables["ok"].ptr, t_act.ptr, bad_n, s), up(tables["ok"].ptr, t_up.ptr, bad_n, s)]
    calls += [act(null, t_act.ptr, 3, s), act(tables["ok"].ptr, null, 3, s), up(null, t_up.ptr, 3, s), up(tables["ok"].ptr, null, 3, s)]
    for name in ("atoms", "head", "hidden", "hidden48", "null_param"):
        calls += [act(tables[name].ptr, t_act.ptr, 3, s), up(tables[name].ptr, t_up.ptr, 3, s)]
    torch.cuda.synchronize()
    assert calls == [EINVAL] * len(calls)
    for t, b in zip(outputs, before):
        _same(t, b, "a refused launch wrote")
    # (the lanes that were offered are ones the single entries run: the refusals above are the lane entries' own)
    for net in (other_atoms[0], other_hidden[0], _copy_net(plain[1], head=K.HEAD_CODE["qr"])):
        io, _ = _act_lane(dev, 1, 4)
        assert lib.dra_dist_mlp_act.raw(ctypes.byref(net), ctypes.byref(io), s) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("head", K.HEADS)
def test_lanes_supported_agrees_with_the_launches(dra, head):
    """dra_dist_mlp_lanes_supported says what the two lane launches accept: over atoms {1, 2, 51, 52} x hidden {8, 16} x transitions
    {8, 9} x batch {256, 257} x lanes {1, 3} both launches return 0 exactly where the table says yes, DRA_EINVAL elsewhere; lane
    counts 0 and 65 are refused by the table as by the launches (test_lane_entries_refuse_and_write_nothing)."""
    from deeprl_amd import dist_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    sup = lib.dra_dist_mlp_lanes_supported.raw
    code = K.HEAD_CODE[head]
    yes = 0
    for n in (1, 2, K.MAX_ATOMS, K.MAX_ATOMS + 1):
        for hidden in (8, 16):
            for n_lanes in (1, 3):
                nets = [_net(dev, head, n, hidden, "relu", 90 + k, lane=k) for k in range(n_lanes)]
                t_net = _table(dist_mlp.Net, [x for x, _ in nets])
                for t_len, batch in ((8, 256), (9, 256), (8, 257)):
                    want = sup(4, 2, hidden, t_len, batch, 1, code, n, n_lanes)
                    assert want == (0 if 2 <= n <= K.MAX_ATOMS and hidden == 16 and t_len == 8 and batch == 256 else EINVAL)
                    rc_act, _ = _act_lanes_launch(dev, nets, n_lanes, t_len)
                    ups = [_update_lane(dev, nets[k], head, max(n, 1), k, batch, False, False) for k in range(n_lanes)]
                    t_io = _table(dist_mlp.UpdateIO, [io for io, _, _ in ups])
                    rc_up = lib.dra_dist_mlp_update_lanes.raw(t_net.ptr, t_io.ptr, n_lanes, stream_ptr())
                    torch.cuda.synchronize()
                    assert rc_act in (0, EINVAL) and rc_up in (0, EINVAL)
                    assert (rc_act == 0 and rc_up == 0) == (want == 0), (n, hidden, n_lanes, t_len, batch, rc_act, rc_up, want)
                    yes += want == 0
    assert yes == 2 * 2
    assert sup(4, 2, 64, 8, 256, 2, code, K.MAX_ATOMS, 64) == 0 and sup(4, 2, 16, 1, 1, 1, code, 2, 1) == 0
    assert all(sup(*a) == EINVAL for a in ((4, 2, 16, 4, 10, 1, code, 20, 0), (4, 2, 16, 4, 10, 1, code, 20, 65), (4, 2, 16, 4, 10, 1, 3, 20, 3),
                                           (4, 2, 16, 4, 10, 3, code, 20, 3), (5, 2, 16, 4, 10, 1, code, 20, 3)))
