"""dra_np_mt_draw_lanes (csrc/np_mt.hip) alone on the device against np.random.RandomState driven through
support.plan_actor_epsilon_greedy and replay.draw_uniform_indices (np_mt_cases.numpy_step: numpy itself, not the host entry): per
step every lane's first slot, indices, random actions and flags, at the end every lane's key and pos.

np_mt_cases.CASES with 3 lanes each; every fourth case also with 1 lane and every eighth with 64.  Lane j of a case starts from
the (j-th next) starting state of np_mt_cases.STARTS under a seed of its own, whatever the lane count, so the numpy side of a
lane is computed once.  100 steps per case, each step writing blocks of its own (filled with 0xff beforehand: what a step must
leave alone shows), so that a case costs one synchronisation.  Nothing is provoked: the budget path is the host entry's test."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from feature_kernel_harness import dra      # noqa: F401  (the fixture)

import np_mt_cases as C

pytestmark = pytest.mark.gpu

STEPS = 100


def _learns(step):
    return step % 5 != 1


def _lane_start(case, j):
    start = C.STARTS[(C.STARTS.index(case[0]) + j) % len(C.STARTS)]
    return (start[0], 1000 + 17 * j + start[1]) + tuple(start[2:])


@functools.lru_cache(maxsize=None)
def _numpy_lane(case, j, steps=STEPS, always_learn=False):
    """Lane j of `case` drawn by numpy: (the uploaded words, per step numpy_step's dict, the final (key, pos))."""
    from deeprl_amd import seed_batch
    _, n_actions, k, batch, ring, eps_kind = case
    rs = C.start_state(_lane_start(case, j))
    words = seed_batch.np_mt_words(rs)
    schedule = C.make_schedule(eps_kind)
    out = [C.numpy_step(rs, schedule, k, batch, n_actions, ring, always_learn or _learns(s)) for s in range(steps)]
    state = rs.get_state()
    return words, out, (state[1], state[2])


def _commons(case, steps):
    """The [steps] dra_np_mt_common blocks of a case (the epsilons are lane 0's: the schedule is common to the lanes)."""
    from deeprl_amd import seed_batch
    _, _, _, _, ring, _ = case
    table = (seed_batch.NpMtCommon * len(steps))()
    for c, st in zip(table, steps):
        C.fill_common(c, st["eps"], st["slot0"], ring)
    return torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy())


def _launch(lib, mt, blocks, common, err, n, case, learn, lay):
    from deeprl_amd._lib import stream_ptr
    _, n_actions, k, batch, _, _ = case
    lib.dra_np_mt_draw_lanes(mt.data_ptr(), blocks.data_ptr(), common.data_ptr(), err.data_ptr(), n, k, batch, n_actions, int(learn),
                             lay['idx'], lay['rand'], lay['flag'], lay['stride'], stream_ptr())


def _assert_block(blk, lay, k, want, learn, what):
    idx = blk[lay['idx']:lay['rand']].view(np.int64)
    assert int(blk[:8].view(np.int64)[0]) == want["slot0"], what
    assert np.array_equal(idx, want["idx"]) if learn else (idx == -1).all(), what
    assert np.array_equal(blk[lay['rand']:lay['flag']].view(np.int64), want["rand"]), what
    assert np.array_equal(blk[lay['flag']:lay['flag'] + k], want["explore"].astype(np.uint8)), what
    assert (blk[lay['flag'] + k:] == 0xff).all(), what      # (the block's padding is nobody's)


def _run_case(d, case, n):
    from deeprl_amd._lib import lib
    from deeprl_amd import seed_batch
    dev = torch.device("cuda:0")
    _, n_actions, k, batch, ring, _ = case
    lay = C.layout(k, batch)
    lanes = [_numpy_lane(case, j) for j in range(n)]
    assert lib.dra_np_mt_lanes_supported.raw(n, k, batch, n_actions, ring[0]) == 0
    mt = torch.from_numpy(np.stack([w for w, _, _ in lanes]).view(np.int32)).to(dev)
    commons = _commons(case, lanes[0][1]).to(dev)
    size = ctypes.sizeof(seed_batch.NpMtCommon)
    blocks = torch.full((STEPS, n * lay['stride']), 0xff, dtype=torch.uint8, device=dev)
    err = torch.zeros(n, dtype=torch.int32, device=dev)
    for s in range(STEPS):
        _launch(lib, mt, blocks[s], commons[s * size:(s + 1) * size], err, n, case, _learns(s), lay)
    torch.cuda.synchronize()
    got, words = blocks.cpu().numpy(), mt.cpu().numpy().view(np.uint32)
    assert not err.cpu().numpy().any()
    for j, (_, steps, (key, pos)) in enumerate(lanes):
        for s, want in enumerate(steps):
            _assert_block(got[s, j * lay['stride']:(j + 1) * lay['stride']], lay, k, want, _learns(s), (C.case_id(case), n, j, s))
        assert int(words[j, 624]) == pos and np.array_equal(words[j, :624], key), (C.case_id(case), n, j)
        assert not words[j, 625:].any()
    return words


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_three_lanes_draw_numpys_stream(dra, case):
    words = _run_case(dra, case, 3)
    if case[3] >= 10:      # (80 minibatches of 10 alone are 800 words: the key was regenerated)
        assert not np.array_equal(words[0, :624], _numpy_lane(case, 0)[0][:624])


@pytest.mark.parametrize("case", C.CASES[::4], ids=C.case_id)
def test_one_lane_draws_numpys_stream(dra, case):
    _run_case(dra, case, 1)


@pytest.mark.parametrize("case", C.CASES[::8], ids=C.case_id)
def test_64_lanes_draw_numpys_stream(dra, case):
    _run_case(dra, case, 64)


def test_graph_replay_equals_eager(dra):
    """One case (6 actions, k 4, batch 10, the ring of 33 slots: both rejections) with 3 lanes through graphs.Region: two eager
    calls, the capture, replays -- 30 steps in all, each reading the common block sent before it -- against numpy, which the eager
    runs above equal."""
    from types import SimpleNamespace
    from deeprl_amd._lib import lib
    from deeprl_amd import seed_batch
    from deeprl_amd.graphs import Region
    dev = torch.device("cuda:0")
    case = (("pos", 9, 300), 6, 4, 10, (33, 5), "linear")
    n, steps, k = 3, 30, case[2]
    lay = C.layout(k, case[3])
    lanes = [_numpy_lane(case, j, steps, True) for j in range(n)]
    mt = torch.from_numpy(np.stack([w for w, _, _ in lanes]).view(np.int32)).to(dev)
    commons = _commons(case, lanes[0][1]).to(dev)
    size = ctypes.sizeof(seed_batch.NpMtCommon)
    common = torch.zeros(size, dtype=torch.uint8, device=dev)
    blocks = torch.full((n * lay['stride'],), 0xff, dtype=torch.uint8, device=dev)
    err = torch.zeros(n, dtype=torch.int32, device=dev)
    region = Region("the np_mt draw launch", SimpleNamespace(), 2)

    def body():
        _launch(lib, mt, blocks, common, err, n, case, True, lay)

    for s in range(steps):
        common.copy_(commons[s * size:(s + 1) * size])
        if region.due() and (region.graph is not None or region.capture(body)):
            region.replay()
        else:
            body()
        torch.cuda.synchronize()
        got = blocks.cpu().numpy()
        for j in range(n):
            _assert_block(got[j * lay['stride']:(j + 1) * lay['stride']], lay, k, lanes[j][1][s], True, ("replay", j, s))
    assert region.graph is not None and region.calls == steps and not region.failed
    words = mt.cpu().numpy().view(np.uint32)
    for j, (_, _, (key, pos)) in enumerate(lanes):
        assert int(words[j, 624]) == pos and np.array_equal(words[j, :624], key)
    assert not err.cpu().numpy().any()
