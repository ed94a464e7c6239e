"""GPU tests of the DDPG / TD3 acting launch over a device-resident environment (csrc/dpg_mlp.hip dra_dpg_env_act,
deeprl_amd/dpg_env.py) against tests/dpg_env_cases.py's restatement: everything but the fp32 actor output to the bit -- ring row,
environment, episode ring, Ornstein-Uhlenbeck state, counters --, the actor output within the family's bar (1e-5 of the largest
magnitude, feature_kernel_harness._fraction) of fp64 and bit-equal to dra_dpg_act on the same observation; every buffer carries
GUARD sentinels; a second run from the same start gives the same bits."""
import ctypes

import numpy as np
import pytest
import torch
from parity_log import record_parity

import dpg_env_cases as K
import dpg_restatement as R
from feature_kernel_harness import GUARD, _bits, _fraction, dra  # noqa: F401

pytestmark = pytest.mark.gpu

CAP = 6                 # replay slots: a run of 8 launches from slot 4 passes capacity - 1 and wraps
LEAD = 8                # unused floats in front of the first parameter tensor (a multiple of 4: optim.FlatParams' alignment)
SENT = {np.dtype(np.float64): -7.25, np.dtype(np.float32): -7.25, np.dtype(np.int64): -77, np.dtype(np.int32): -77}


class _Buf:
    """Host array -> device tensor with GUARD sentinels behind it."""

    def __init__(self, dev, init):
        init = np.ascontiguousarray(init)
        self.n, self.shape, self.fill = init.size, init.shape, SENT[init.dtype]
        full = np.concatenate([init.reshape(-1), np.full(GUARD, self.fill, dtype=init.dtype)])
        self.t = torch.from_numpy(full).to(dev)

    def ptr(self):
        return self.t.data_ptr()

    def read(self):
        full = self.t.cpu().numpy()
        assert (full[self.n:] == self.fill).all(), "guard overwritten"
        return full[:self.n].reshape(self.shape).copy()


def _flat_actor(params):
    """(float32 flat array with a leading gap and NaN between 16-byte aligned tensors, offsets in dra_dpg_net's order)"""
    chunks, offs, o = [np.full(LEAD, np.nan, dtype=np.float32)], [], LEAD
    for lay in R.LAYERS:
        v = params["a." + lay].numpy().astype(np.float32).reshape(-1)
        offs.append(o)
        pad = (-v.size) % 4 + 4
        chunks += [v, np.full(pad, np.nan, dtype=np.float32)]
        o += v.size + pad
    return np.concatenate(chunks), offs


class _Case:
    """The device side of one case: every buffer of dra_dpg_env_act_io, guarded."""

    def __init__(self, dra, shape, seed, horizon, steps_before=1, slot0=CAP - 2):
        from deeprl_amd import dpg_mlp
        self.dev = dev = dra.Config.DEVICE
        self.shape, self.horizon = shape, horizon
        s, a = shape[0], shape[1]
        self.params = K.actor_params(shape, seed)
        flat, offs = _flat_actor(self.params)
        self.flat_host = flat
        self.env, self.obs = K.make_env(shape, seed, horizon, steps_before)
        st, c, steps, ret, sd = K.env_arrays(self.env)
        rs = np.random.RandomState(seed + 7)
        self.x0 = rs.standard_normal(a) * 0.05
        self.x = rs.standard_normal(a) * 0.1
        self.ring = dict(frames=rs.standard_normal((CAP, s)), actions=rs.standard_normal((CAP, a)),
                         rewards=rs.standard_normal(CAP), masks=np.full(CAP, 5, dtype=np.int32))
        self.ep = dict(rows=rs.standard_normal((K.EP_RING_CAP, 3)), count=K.EP_RING_COUNT0)
        self.step_counter, self.slot = K.STEP0, slot0
        f64, i64 = np.float64, np.int64
        self.b = dict(param=_Buf(dev, flat), env_state=_Buf(dev, st), env_counter=_Buf(dev, np.asarray([c], i64)),
                      ep_steps=_Buf(dev, np.asarray([steps], np.int32)), ep_return=_Buf(dev, np.asarray([ret], f64)),
                      env_seed=_Buf(dev, np.asarray([sd], i64)), step_counter=_Buf(dev, np.asarray([K.STEP0], i64)),
                      ep_count=_Buf(dev, np.asarray([K.EP_RING_COUNT0], i64)), ep_ring=_Buf(dev, self.ep["rows"]),
                      mode=_Buf(dev, np.zeros(1, i64)), slot=_Buf(dev, np.zeros(1, i64)), bounds=_Buf(dev, np.asarray([K.LOW, K.HIGH], f64)),
                      v=_Buf(dev, np.zeros(a, f64)), ou_x=_Buf(dev, self.x), ou_x0=_Buf(dev, self.x0),
                      ring_frames=_Buf(dev, self.ring["frames"]), ring_actions=_Buf(dev, self.ring["actions"]),
                      ring_rewards=_Buf(dev, self.ring["rewards"]), ring_masks=_Buf(dev, self.ring["masks"]),
                      out_action=_Buf(dev, np.full(a, 9.0, np.float32)), err=_Buf(dev, np.zeros(1, np.int32)),
                      act_in=_Buf(dev, np.zeros(s, f64)), act_out=_Buf(dev, np.full(a, 9.0, np.float32)))
        n = dpg_mlp.Net()
        n.param = self.b["param"].ptr()
        n.actor = (ctypes.c_int32 * 6)(*offs)
        n.state_dim, n.action_dim, n.h1, n.h2, n.gate, n.n_critics = s, a, shape[2], shape[3], shape[4], 1
        self.net = n

    def io(self, env_kind=None):
        from deeprl_amd import dpg_env
        io = dpg_env.ActIO()
        for k in ("env_state", "env_counter", "ep_steps", "ep_return", "env_seed", "step_counter", "ep_count", "ep_ring", "mode", "slot",
                  "bounds", "v", "ou_x", "ou_x0", "ring_frames", "ring_actions", "ring_rewards", "ring_masks", "out_action", "err"):
            setattr(io, k, self.b[k].ptr())
        io.horizon, io.ring_cap, io.capacity = self.horizon, K.EP_RING_CAP, CAP
        io.ou_theta, io.ou_mu, io.ou_dt = K.OU["theta"], K.OU["mu"], K.OU["dt"]
        io.env_kind = self.shape[5] if env_kind is None else env_kind
        return io

    def stage(self, mode, slot, v):
        for k, val, dt in (("mode", [mode], np.int64), ("slot", [slot], np.int64), ("v", v, np.float64)):
            b = self.b[k]
            b.t[:b.n].copy_(torch.from_numpy(np.asarray(val, dtype=dt)))

    def launch(self, net=None, env_kind=None):
        from deeprl_amd._lib import lib, stream_ptr
        io = self.io(env_kind)
        rc = lib.dra_dpg_env_act.raw(ctypes.byref(net or self.net), ctypes.byref(io), stream_ptr())
        torch.cuda.synchronize()
        return rc

    def dpg_act(self, obs):
        """dra_dpg_act on the observation, as DDPGAgent's host path calls it (fp64 in, one row)."""
        from deeprl_amd._lib import lib, stream_ptr
        b = self.b["act_in"]
        b.t[:b.n].copy_(torch.from_numpy(np.asarray(obs, dtype=np.float64)))
        lib.dra_dpg_act(ctypes.byref(self.net), b.ptr(), self.shape[0], 1, 1, self.b["act_out"].ptr(), stream_ptr())
        torch.cuda.synchronize()
        return self.b["act_out"].read()

    def snapshot(self):
        return {k: b.read() for k, b in self.b.items()}


def _noise(rs, a_dim, t):
    """The staged vector of launch t: the first launches reach both clip bounds in every mode (+3, -6, +3: the Ornstein-Uhlenbeck
    state, which sums them, goes to 3, to -3 and back to about 0)."""
    v = rs.standard_normal(a_dim) * 0.3
    if t < 3:
        v[0] = -6.0 if t == 1 else 3.0
        if a_dim > 1:
            v[1] = -v[0]
    return v


def _run(dra, shape, mode, horizon, seed, n_launches=8, check=True):
    """n_launches chained launches of one case against the restatement -> (snapshots, worst actor fraction, episodes seen)."""
    case = _Case(dra, shape, seed, horizon)
    rs = np.random.RandomState(seed + 99)
    a_dim, gate = shape[1], shape[4]
    obs, x, step, slot, errs = case.obs, case.x.copy(), case.step_counter, case.slot, 0
    snaps, worst, clipped = [], 0.0, set()
    for t in range(n_launches):
        v = _noise(rs, a_dim, t)
        case.stage(mode, slot, v)
        a32 = case.dpg_act(obs)
        assert case.launch() == 0
        got = case.snapshot()
        snaps.append(got)
        if not check:
            slot = (slot + 1) % CAP
            continue
        assert np.array_equal(_bits(got["out_action"]), _bits(a32)), "not dra_dpg_act's bits"
        worst = max(worst, _fraction(got["out_action"], K.actor64(case.params, obs, gate), "actor output, launch %d" % t))
        act, x, step, err, obs = K.restate(case.env, obs, a32, mode, v, x, case.x0, slot, CAP, case.ring, case.ep, step)
        clipped |= {b for b in (K.LOW, K.HIGH) if (act == b).any()}
        errs += err
        st, c, steps, ret, _ = K.env_arrays(case.env)
        for k, want in (("ring_frames", case.ring["frames"]), ("ring_actions", case.ring["actions"]), ("ring_rewards", case.ring["rewards"]),
                        ("env_state", st), ("ep_return", [ret]), ("ep_ring", case.ep["rows"]), ("ou_x", x), ("ou_x0", case.x0)):
            assert np.array_equal(_bits(got[k]), _bits(np.asarray(want, dtype=np.float64).reshape(got[k].shape))), (k, t)
        assert np.array_equal(got["ring_masks"], case.ring["masks"]), t
        assert (int(got["env_counter"][0]), int(got["ep_steps"][0]), int(got["step_counter"][0]), int(got["ep_count"][0]), int(got["err"][0])) == \
            (c, steps, step, case.ep["count"], errs), t
        assert np.array_equal(_bits(got["param"]), _bits(case.flat_host)), "a parameter was written"
        slot = (slot + 1) % CAP
    return snaps, worst, case.ep["count"] - K.EP_RING_COUNT0, clipped


@pytest.mark.parametrize("mode", sorted(K.MODES))
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "S%d_A%d_H%d_%d_g%d_env%d" % s)
def test_env_act_matches_restatement(dra, shape, mode):  # noqa: F811
    """Eight chained launches under horizon 3 from slot capacity - 2: both clip bounds, an episode end (mask 0, the OU state back at
    x0, an episode-ring row that wraps the ring of 5), the slot capacity - 1 and the wrap to 0; then the same run again, bit for bit."""
    snaps, worst, episodes, clipped = _run(dra, shape, K.MODES[mode], 3, seed=11)
    assert episodes >= 2 and clipped == {K.LOW, K.HIGH}
    record_parity("dpg_env_act_%s_S%d_H%d" % (mode, shape[0], shape[2]), actor=worst)
    assert worst <= 1.0
    again, _, _, _ = _run(dra, shape, K.MODES[mode], 3, seed=11, check=False)
    for a, b in zip(snaps, again):
        for k in set(a) - {"act_in", "act_out"}:          # (the unchecked run does not follow the observations for dra_dpg_act)
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("shape", [K.SHAPES[0], K.SHAPES[2]], ids=["pendulum", "synthetic"])
def test_env_act_horizon_one_ends_an_episode_in_every_launch(dra, shape):  # noqa: F811
    _, worst, episodes, _ = _run(dra, shape, K.MODE_OU, 1, seed=5, n_launches=3)
    assert episodes == 3 and worst <= 1.0


@pytest.mark.parametrize("shape", [K.SHAPES[0], K.SHAPES[2]], ids=["pendulum", "synthetic"])
def test_env_act_bad_slots_are_slot_zero_and_counted(dra, shape):  # noqa: F811
    def one(slot):
        case = _Case(dra, shape, 21, 3)
        case.stage(K.MODE_GAUSS, slot, np.full(shape[1], 0.25))
        assert case.launch() == 0
        return case.snapshot()
    want = one(0)
    assert int(want["err"][0]) == 0
    for bad in (-1, CAP, CAP + 1000):
        got = one(bad)
        assert int(got["err"][0]) == 1
        for k in want:
            if k not in ("err", "slot"):
                assert np.array_equal(_bits(got[k]), _bits(want[k])), (bad, k)


def test_env_act_refuses_shapes_outside_its_table_and_writes_nothing(dra):  # noqa: F811
    from deeprl_amd import dpg_env
    assert dpg_env.supported(K.ENV_PENDULUM, 3, 1, 400, 300, 1) and dpg_env.supported(K.ENV_SYNTHETIC, 64, 16, 512, 512, 2)
    for kind, s, a, h1, h2, gate in ((K.ENV_PENDULUM, 4, 1, 32, 24, 1), (K.ENV_PENDULUM, 3, 2, 32, 24, 1), (K.ENV_SYNTHETIC, 65, 6, 32, 24, 1),
                                     (K.ENV_SYNTHETIC, 17, 17, 32, 24, 1), (K.ENV_SYNTHETIC, 17, 6, 513, 24, 1), (K.ENV_SYNTHETIC, 17, 6, 32, 0, 1),
                                     (K.ENV_SYNTHETIC, 17, 6, 32, 24, 3), (2, 17, 6, 32, 24, 1)):
        assert not dpg_env.supported(kind, s, a, h1, h2, gate), (kind, s, a, h1, h2, gate)
    case = _Case(dra, K.SHAPES[2], 3, 3)
    case.stage(K.MODE_GAUSS, 1, np.full(6, 0.25))
    before = case.snapshot()
    assert case.launch(env_kind=K.ENV_PENDULUM) != 0          # a 17-dimensional "pendulum"
    assert case.launch(env_kind=2) != 0
    wide = type(case.net)()
    ctypes.memmove(ctypes.byref(wide), ctypes.byref(case.net), ctypes.sizeof(wide))
    wide.h1 = 513
    assert case.launch(net=wide) != 0
    after = case.snapshot()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
