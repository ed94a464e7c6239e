"""The window's seed-lane kernels (csrc/dqn_mlp.hip: dra_dqn_replay_mlp_update_lanes; csrc/np_mt.hip: dra_np_mt_draw_window_lanes)
against the single entry and the host twin on copies of the same buffers.  A lane runs the single launch's text, so every
comparison is bit for bit, guard elements behind every buffer included; a tolerance would hide a lane-indexing bug."""
import ctypes

import numpy as np
import pytest
import torch
from feature_kernel_harness import GUARD, dra, _bits, _guarded      # noqa: F401  (dra: the fixture)

import dqn_feature_cases as K
import np_mt_cases as C
import np_mt_window_cases as W
from test_gpu_dqn_lanes_kernels import _net, _same, _table

pytestmark = pytest.mark.gpu

EINVAL = -22
NAN = float("nan")
RING_CAP = 40
EDGE_LANE = 1       # the lane whose indices sit at the clamp edge, one of them outside the ring
OUTS = ("grad", "q_target", "td", "loss", "prio", "weights")


def _lane_host(lane, batch, n_step, edge):
    rs = np.random.RandomState(700 + lane)
    ring = dict(frames=rs.uniform(-0.5, 0.5, size=(RING_CAP, 4)), actions=rs.randint(2, size=RING_CAP).astype(np.int64),
                rewards=rs.uniform(0.5, 1.5, size=RING_CAP), masks=(rs.rand(RING_CAP) < 0.8).astype(np.int32))
    last = RING_CAP - 1 - n_step       # the largest index the kernel takes as it is
    idx = rs.randint(0, last + 1, size=batch).astype(np.int64)
    if edge:
        idx[:] = last
        idx[batch // 2] = RING_CAP + 5
    prob = rs.uniform(0.01, 0.2, size=batch).astype(np.float32)
    return ring, idx, prob, np.float32(0.4 + 0.05 * (lane % 12))


def _lane(dev, net, lane, batch, double_q, n_step, per, edge=False):
    """-> (dra_dqn_replay_mlp_update_io of lane `lane` over fresh guarded outputs, the outputs' full tensors by name, the inputs).
    A lane without priorities is handed the priority and weight buffers all the same: the launch must leave them alone."""
    from deeprl_amd import dqn_replay_mlp
    ring, idx, prob, beta = _lane_host(lane, batch, n_step, edge)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = [t(ring[k]) for k in ("frames", "actions", "rewards", "masks")] + [t(idx), t(prob), t(np.asarray([beta]))]
    n = net[1][0].numel()
    full, v = {}, {}
    for k, shape in (("grad", (n,)), ("q_target", (batch,)), ("td", (batch,)), ("loss", (1,)), ("prio", (batch,)), ("weights", (batch,))):
        full[k], v[k] = _guarded(shape, torch.float32, dev, NAN)
    full["err"] = torch.zeros(1, dtype=torch.int32, device=dev)
    io = dqn_replay_mlp.UpdateIO()
    io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks, io.idx = (x.data_ptr() for x in keep[:5])
    if per:
        io.prob, io.beta = keep[5].data_ptr(), keep[6].data_ptr()
    io.grad, io.out_q_target, io.out_td, io.out_loss = v["grad"].data_ptr(), v["q_target"].data_ptr(), v["td"].data_ptr(), v["loss"].data_ptr()
    io.out_prio, io.out_weights = v["prio"].data_ptr(), v["weights"].data_ptr()
    io.err, io.capacity = full["err"].data_ptr(), RING_CAP
    io.discount, io.step_discount = K.DISCOUNT ** n_step, K.DISCOUNT
    io.replay_eps, io.replay_alpha = 0.01, 0.5
    io.batch, io.double_q, io.n_step = batch, int(double_q), n_step
    return io, full, keep


# (n_lanes, hidden, gate, n_step, batch, double_q, per): every width with both gates; n_step 1, 3, 8; batch 1, 10, 64, 65 (the second
# row block) and 256; 1, 3 and 64 lanes; double_q on and off; priorities in every lane, in none, and in every other lane
CASES = [(1, 16, "relu", 1, 1, False, "none"), (3, 16, "tanh", 3, 10, True, "all"), (64, 16, "relu", 8, 10, False, "mixed"),
         (3, 32, "relu", 3, 64, True, "none"), (3, 32, "tanh", 8, 65, False, "all"), (1, 32, "tanh", 1, 256, True, "all"),
         (3, 64, "relu", 8, 256, False, "mixed"), (64, 64, "tanh", 3, 65, True, "all"), (3, 64, "tanh", 1, 10, False, "none"),
         (3, 64, "relu", 1, 64, True, "all"), (3, 16, "relu", 3, 1, False, "all"), (64, 32, "relu", 1, 10, True, "none")]


def _per(kind, lane):
    return kind == "all" or (kind == "mixed" and lane % 2 == 1)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "lanes%d-h%d-%s-n%d-b%d-dq%d-per_%s" % c)
def test_update_lanes_equal_the_single_launches(dra, case):
    """dra_dqn_replay_mlp_update_lanes over lanes with their own ring, indices, probabilities, beta word, online and target
    parameters against dra_dqn_replay_mlp_update lane by lane: the flat gradient (every element, the guard behind it), q_target,
    td, the loss, the priorities and the weights to the bit -- the last two untouched in a lane without priorities.  With more than
    one lane, lane 1's indices all sit at the clamp edge capacity - 1 - n_step and one lies outside the ring: only that lane's err
    counts it, and its outputs are the single entry's on the same indices, which clamps them."""
    from deeprl_amd import dqn_mlp, dqn_replay_mlp
    from deeprl_amd._lib import lib, stream_ptr
    n_lanes, hidden, gate, n_step, batch, double_q, per = case
    dev = dra.Config.DEVICE
    nets = [_net(dev, hidden, gate, 80 + k) for k in range(n_lanes)]
    edge = lambda k: n_lanes > 1 and k == EDGE_LANE
    assert lib.dra_dqn_replay_mlp_lanes_supported.raw(4, 2, hidden, 4, batch, nets[0][0].gate, n_step, n_lanes) == 0
    want = []
    for k in range(n_lanes):
        io, full, keep = _lane(dev, nets[k], k, batch, double_q, n_step, _per(per, k), edge(k))
        assert lib.dra_dqn_replay_mlp_update.raw(ctypes.byref(nets[k][0]), ctypes.byref(io), stream_ptr()) == 0
        want.append((full, keep))
    lanes = [_lane(dev, nets[k], k, batch, double_q, n_step, _per(per, k), edge(k)) for k in range(n_lanes)]
    t_net, t_io = _table(dqn_mlp.Net, [n for n, _ in nets]), _table(dqn_replay_mlp.UpdateIO, [io for io, _, _ in lanes])
    assert lib.dra_dqn_replay_mlp_update_lanes.raw(t_net.ptr, t_io.ptr, n_lanes, stream_ptr()) == 0
    torch.cuda.synchronize()
    for k in range(n_lanes):
        got = lanes[k][1]
        for name in want[k][0]:
            _same(got[name], want[k][0][name], (k, name))
        assert int(got["err"][0]) == (1 if edge(k) else 0), k
        assert torch.isfinite(got["grad"][:-GUARD]).all() and all(torch.isnan(got[name][-GUARD:]).all() for name in OUTS)
        if _per(per, k):
            assert torch.isfinite(got["prio"][:-GUARD]).all() and float(got["weights"][:-GUARD].max()) == 1.0
        else:
            assert torch.isnan(got["prio"]).all() and torch.isnan(got["weights"]).all()
    if n_lanes > 1:     # (the lanes computed different things: a lane that read another lane's row would show above)
        assert not torch.equal(lanes[0][1]["grad"][:-GUARD], lanes[2][1]["grad"][:-GUARD])


@pytest.mark.parametrize("hidden, gate, batch, double_q", [(16, "relu", 10, False), (64, "tanh", 65, True)])
def test_window_of_one_without_priorities_is_the_one_step_lane_launch(dra, hidden, gate, batch, double_q):
    """At n_step 1 with prob NULL the window's lane launch gives dra_dqn_mlp_update_lanes' bits on the same three lanes: the
    gradient, q_target, td and the loss."""
    from deeprl_amd import dqn_mlp, dqn_replay_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    nets = [_net(dev, hidden, gate, 80 + k) for k in range(3)]
    t_net = _table(dqn_mlp.Net, [n for n, _ in nets])
    new = [_lane(dev, nets[k], k, batch, double_q, 1, False) for k in range(3)]
    old = [_lane(dev, nets[k], k, batch, double_q, 1, False) for k in range(3)]
    rows = []
    for io, _, _ in old:
        o = dqn_mlp.UpdateIO()
        for name, _ in dqn_mlp.UpdateIO._fields_:
            setattr(o, name, getattr(io, name))
        rows.append(o)
    # (the kernels read their tables when they RUN: both tables live until the synchronize below)
    t_new, t_old = _table(dqn_replay_mlp.UpdateIO, [io for io, _, _ in new]), _table(dqn_mlp.UpdateIO, rows)
    assert lib.dra_dqn_replay_mlp_update_lanes.raw(t_net.ptr, t_new.ptr, 3, stream_ptr()) == 0
    assert lib.dra_dqn_mlp_update_lanes.raw(t_net.ptr, t_old.ptr, 3, stream_ptr()) == 0
    torch.cuda.synchronize()
    del t_new, t_old
    for k in range(3):
        for name in ("grad", "q_target", "td", "loss", "err"):
            _same(new[k][1][name], old[k][1][name], (k, name))
        assert torch.isfinite(new[k][1]["grad"][:-GUARD]).all()


def test_lane_entry_refuses_and_writes_nothing(dra):
    """Lanes that differ in n_step, a null pointer in lane 2, n_lanes 0 and 65, null tables, a lane of another width, priorities
    without a beta word: DRA_EINVAL, and the canary-filled outputs of EVERY lane are as they were.  The shape table says what the
    entry takes."""
    from deeprl_amd import dqn_mlp, dqn_replay_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    nets = [_net(dev, 16, "relu", 70 + k) for k in range(3)]
    t_net = _table(dqn_mlp.Net, [n for n, _ in nets])
    odd = dqn_mlp.Net.from_buffer_copy(bytes(nets[1][0]))
    odd.hidden = 32
    t_odd = _table(dqn_mlp.Net, [nets[0][0], odd, nets[2][0]])
    lanes = [_lane(dev, nets[k], k, 10, False, 3, True) for k in range(3)]
    ios = [io for io, _, _ in lanes]

    def changed(lane, **fields):
        rows = [dqn_replay_mlp.UpdateIO.from_buffer_copy(bytes(io)) for io in ios]
        for name, value in fields.items():
            setattr(rows[lane], name, value)
        return _table(dqn_replay_mlp.UpdateIO, rows)
    good = changed(0)
    tables = [changed(1, n_step=2), changed(2, n_step=8), changed(2, idx=None), changed(2, grad=None), changed(2, err=None),
              changed(2, beta=None), changed(0, n_step=9), changed(1, batch=257), changed(1, capacity=3)]
    outputs = [t for _, full, _ in lanes for t in full.values()]
    before = [t.clone() for t in outputs]
    s, null = stream_ptr(), ctypes.c_void_p(None)
    fn = lib.dra_dqn_replay_mlp_update_lanes.raw
    calls = [fn(t_net.ptr, t.ptr, 3, s) for t in tables]
    calls += [fn(t_net.ptr, good.ptr, bad_n, s) for bad_n in (0, 65, -1)]
    calls += [fn(null, good.ptr, 3, s), fn(t_net.ptr, null, 3, s), fn(t_odd.ptr, good.ptr, 3, s)]
    torch.cuda.synchronize()
    assert calls == [EINVAL] * len(calls)
    for t, b in zip(outputs, before):
        _same(t, b, "a refused launch wrote")
    sup = lib.dra_dqn_replay_mlp_lanes_supported.raw
    assert sup(4, 2, 16, 4, 10, 1, 1, 1) == 0 and sup(4, 2, 64, 8, 256, 2, 8, 64) == 0
    assert all(sup(*a) == EINVAL for a in ((4, 2, 16, 4, 10, 1, 3, 0), (4, 2, 16, 4, 10, 1, 3, 65), (4, 2, 48, 4, 10, 1, 3, 3),
                                           (4, 2, 16, 9, 10, 1, 3, 3), (4, 2, 16, 4, 257, 1, 3, 3), (4, 2, 16, 4, 10, 3, 3, 3),
                                           (4, 2, 16, 4, 10, 1, 0, 3), (4, 2, 16, 4, 10, 1, 9, 3)))


# ------------------------------------------------------------------------------------------ the window's draws
def _mt_pos(lane):
    """Every lane at another pos: one word before the twist, on it, at the key's start, then spread over the key."""
    return (623, 624, 0, 300, 561)[lane] if lane < 5 else (lane * 97 + 1) % 623


@pytest.mark.parametrize("n_step", [1, 3, 8])
@pytest.mark.parametrize("n_lanes", [1, 5, 64])
def test_draw_window_lanes_equal_the_host_twin(dra, n_lanes, n_step):
    """dra_np_mt_draw_window_lanes against dra_np_mt_draw_window_host on the same states, twelve steps through the ring states of
    np_mt_window_cases.rings (either range of valid indices empty, one valid slot, both populated; two steps do not learn): every
    lane's block and generator state byte for byte after every step, the err words 0."""
    from deeprl_amd import seed_batch
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    assert len({_mt_pos(k) for k in range(64)}) == 64
    hosts = [W.WindowLane(C.start_state(("pos", 40 + k, _mt_pos(k))), W.K, W.BATCH, W.N_ACTIONS, n_step) for k in range(n_lanes)]
    lay = hosts[0].lay
    assert lib.dra_np_mt_window_lanes_supported.raw(n_lanes, W.K, W.BATCH, W.N_ACTIONS, W.CAPACITY, n_step) == 0
    mt = torch.from_numpy(np.stack([h.words for h in hosts]).view(np.int32)).to(dev)
    blocks = torch.zeros(n_lanes * lay['stride'], dtype=torch.uint8, device=dev)
    err = torch.zeros(n_lanes, dtype=torch.int32, device=dev)
    eps = [0.9, 0.0, 0.37, 1.0]
    for step, (name, ring) in enumerate(W.rings(n_step) * 2):
        learn = step % 6 != 1
        common = seed_batch.NpMtCommon()
        C.fill_common(common, eps, step % ring[0], ring)
        common_dev = torch.from_numpy(np.frombuffer(bytes(common), dtype=np.uint8).copy()).to(dev)
        for h in hosts:
            h.step(eps, step % ring[0], ring, learn)
            assert h.err.value == 0
        assert lib.dra_np_mt_draw_window_lanes.raw(mt.data_ptr(), blocks.data_ptr(), common_dev.data_ptr(), err.data_ptr(), n_lanes, W.K,
                                                   W.BATCH, W.N_ACTIONS, int(learn), lay['idx'], lay['rand'], lay['flag'], lay['stride'],
                                                   n_step, stream_ptr()) == 0
        torch.cuda.synchronize()
        got_mt, got_blocks = mt.cpu().numpy().view(np.uint32), blocks.cpu().numpy().reshape(n_lanes, lay['stride'])
        assert not err.cpu().numpy().any(), (step, name)
        for k, h in enumerate(hosts):
            assert np.array_equal(got_mt[k][:625], h.words[:625]), (step, name, k, "generator")
            assert got_blocks[k][:lay['size']].tobytes() == h.block[:lay['size']].tobytes(), (step, name, k, "block")
            if learn:
                assert all(W.valid(int(i), ring[1], ring[0], n_step) for i in h.idx()), (step, name, k)
    if n_lanes > 1:
        assert not np.array_equal(got_blocks[0], got_blocks[1])


def test_draw_window_entry_refuses(dra):
    """n_step 0 and 9, n_lanes 65 and a null state table: DRA_EINVAL, the blocks as they were."""
    from deeprl_amd import seed_batch
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    host = W.WindowLane(C.start_state(("seed", 4)), W.K, W.BATCH, W.N_ACTIONS, 3)
    lay = host.lay
    mt = torch.from_numpy(np.stack([host.words] * 3).view(np.int32)).to(dev)
    blocks = torch.full((3 * lay['stride'],), 7, dtype=torch.uint8, device=dev)
    err = torch.zeros(3, dtype=torch.int32, device=dev)
    common = seed_batch.NpMtCommon()
    C.fill_common(common, [0.5] * 4, 7, (24, 11))
    common_dev = torch.from_numpy(np.frombuffer(bytes(common), dtype=np.uint8).copy()).to(dev)
    tail = (W.K, W.BATCH, W.N_ACTIONS, 1, lay['idx'], lay['rand'], lay['flag'], lay['stride'])
    fn = lib.dra_np_mt_draw_window_lanes.raw
    calls = [fn(mt.data_ptr(), blocks.data_ptr(), common_dev.data_ptr(), err.data_ptr(), 3, *tail, n, stream_ptr()) for n in (0, 9, -1)]
    calls += [fn(mt.data_ptr(), blocks.data_ptr(), common_dev.data_ptr(), err.data_ptr(), 65, *tail, 3, stream_ptr()),
              fn(None, blocks.data_ptr(), common_dev.data_ptr(), err.data_ptr(), 3, *tail, 3, stream_ptr())]
    torch.cuda.synchronize()
    assert calls == [EINVAL] * len(calls)
    assert (blocks == 7).all() and not err.any()
