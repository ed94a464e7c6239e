"""GPU tests of the DDPG / TD3 evaluation launch (csrc/dpg_mlp.hip dra_dpg_eval) on its own recorded trajectory: with the debug
outputs on, every action is bit-equal to dra_dpg_act on the one observation formed from the recorded state and within 1e-5 of the
fp64 actor (tests/test_gpu_dpg_env.py's bar for this forward), every recorded state is python's envs.Pendulum advanced from the one
before under that action, to the bit, every episode starts in the reset state of its counter, every return is the in-order fp64
sum of those rewards, and the words the environment is left with are the host loop's; then the whole launch against a host loop of
envs.Pendulum driven by dra_dpg_act one row at a time (tests/dpg_eval_restatement.py), to the bit.  Every buffer carries GUARD
sentinels, the parameters stay as they are, a second launch gives the same bits, the debug pointers change nothing, and a refused
launch writes nothing."""
import ctypes

import numpy as np
import pytest
import torch
from parity_log import record_parity

import dpg_env_cases as K
import dpg_eval_cases as C
import dpg_eval_restatement as E
import dpg_restatement as R
from feature_kernel_harness import GUARD, _bits, _guarded, dra  # noqa: F401

pytestmark = pytest.mark.gpu

LEAD = 8                # unused floats in front of the first parameter tensor (a multiple of 4: optim.FlatParams' alignment)
ACTOR_BAR = 1e-5        # of max(|fp64 action|, 1): test_gpu_dpg_env.py's bar for this forward


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
    """The device side of one launch: every buffer of dra_dpg_eval_io behind GUARD sentinels, the actor's flat parameters, and
    dra_dpg_act's one-row buffers."""
    SPEC = dict(env_state=(torch.float64, float("nan")), env_counter=(torch.int64, -7), ep_steps=(torch.int32, -7),
                ep_return=(torch.float64, float("nan")), env_seed=(torch.int64, -7), out_return=(torch.float64, float("nan")),
                out_steps=(torch.int64, -7), arrive=(torch.int32, -7), out_state=(torch.float64, float("nan")),
                out_action=(torch.float32, float("nan")), act_in=(torch.float64, float("nan")), act_out=(torch.float32, float("nan")))

    def __init__(self, dra, shape, n, horizon, junk):
        from deeprl_amd import dpg_mlp
        self.dev = dev = dra.Config.DEVICE
        self.shape, self.n, self.horizon, self.junk = shape, n, horizon, junk
        self.params = C.params(shape)
        self.flat_host, offs = _flat_actor(self.params)
        self.shapes = dict(env_state=(2,), env_counter=(1,), ep_steps=(1,), ep_return=(1,), env_seed=(1,), out_return=(n,), out_steps=(1,),
                           arrive=(1,), out_state=(n, horizon + 1, 2), out_action=(n, horizon), act_in=(n * horizon, 3),
                           act_out=(n * horizon,), param=(self.flat_host.size,))
        self.full, self.view = {}, {}
        for k, (dt, fill) in self.SPEC.items():
            self.full[k], self.view[k] = _guarded(self.shapes[k], dt, dev, fill)
        self.full["param"], self.view["param"] = _guarded(self.shapes["param"], torch.float32, dev, -7.25)
        self.fill = dict({k: f for k, (_, f) in self.SPEC.items()}, param=-7.25)
        self.view["param"].copy_(torch.from_numpy(self.flat_host))
        self.reset()
        net = dpg_mlp.Net()
        net.param = self.view["param"].data_ptr()
        net.actor = (ctypes.c_int32 * 6)(*offs)
        net.state_dim, net.action_dim, net.h1, net.h2, net.gate, net.n_critics = shape[0], shape[1], shape[2], shape[3], shape[4], 1
        self.net = net

    def reset(self):
        """The environment's words as the launch finds them: a fresh environment as Task.reset() leaves it (the counter 0), or
        JUNK in the state and episode words behind a non-zero counter; the outputs back to their sentinels."""
        v = self.view
        env = C.make_env(self.junk, self.horizon)
        if not self.junk:
            env.reset()
        self.c0 = int(env.c)
        v["env_state"].copy_(torch.from_numpy(np.asarray(env.s, dtype=np.float64)))
        v["env_counter"].fill_(env.c); v["ep_steps"].fill_(env.steps); v["ep_return"].fill_(env.ret); v["env_seed"].fill_(env.seed)
        v["arrive"].zero_()
        for k in ("out_return", "out_steps", "out_state", "out_action"):
            v[k].fill_(self.fill[k])

    def io(self, debug=True, **over):
        from deeprl_amd import dpg_mlp
        io = dpg_mlp.EvalIO()
        for k in ("env_state", "env_counter", "ep_steps", "ep_return", "env_seed", "out_return", "out_steps", "arrive"):
            setattr(io, k, self.view[k].data_ptr())
        if debug:
            io.out_state, io.out_action = self.view["out_state"].data_ptr(), self.view["out_action"].data_ptr()
        io.horizon, io.n_episodes = self.horizon, self.n
        for k, val in over.items():
            setattr(io, k, val)
        return io

    def launch(self, debug=True, net=None, **over):
        from deeprl_amd._lib import lib, stream_ptr
        io = self.io(debug, **over)
        rc = lib.dra_dpg_eval.raw(ctypes.byref(net or self.net), ctypes.byref(io), stream_ptr())
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        """Every buffer's body, after checking the sentinels behind it."""
        out = {}
        for k, full in self.full.items():
            host = full.cpu().numpy()
            n = int(np.prod(self.shapes[k]))
            tail, fill = host[n:], self.fill[k]
            assert tail.size == GUARD and (np.isnan(tail).all() if fill != fill else (tail == fill).all()), "guard behind %s overwritten" % k
            out[k] = host[:n].reshape(self.shapes[k]).copy()
        return out

    def dpg_act_rows(self, obs):
        """dra_dpg_act on each of the observations [m][3] ALONE -- one launch of one row each, fp64 in, as DDPGAgent's host path
        calls it -- -> fp32 [m]."""
        from deeprl_amd._lib import lib, stream_ptr
        m = obs.shape[0]
        self.view["act_in"][:m].copy_(torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float64)))
        a_in, a_out = self.view["act_in"].data_ptr(), self.view["act_out"].data_ptr()
        for i in range(m):
            lib.dra_dpg_act(ctypes.byref(self.net), a_in + 24 * i, 3, 1, 1, a_out + 4 * i, stream_ptr())
        torch.cuda.synchronize()
        return self.view["act_out"][:m].cpu().numpy()


def _observe(state):
    from deeprl_amd.envs import Pendulum
    env = Pendulum(0)
    env.s = np.asarray(state, dtype=np.float64)
    return env._obs()


def _check_trajectory(case, got):
    """The launch on its own recorded trajectory -> the worst actor error as a fraction of the bar."""
    from deeprl_amd.envs import Pendulum
    n, horizon, c0 = case.n, case.horizon, case.c0
    states, actions = got["out_state"], got["out_action"]
    assert not np.isnan(states).any() and not np.isnan(actions).any()
    obs = np.stack([_observe(states[e, t]) for e in range(n) for t in range(horizon)])
    # each action: dra_dpg_act's bits on the one observation, and within the bar of the fp64 actor
    alone = case.dpg_act_rows(obs)
    assert np.array_equal(_bits(alone.reshape(n, horizon)), _bits(actions)), "not dra_dpg_act's bits"
    want = R.actor(case.params, R.f64(obs), case.shape[4]).numpy().reshape(n, horizon)
    frac = float((np.abs(actions.astype(np.float64) - want) / (ACTOR_BAR * np.maximum(np.abs(want), 1.0))).max())
    print("actor: worst %.3f of the bar over %d observations" % (frac, n * horizon))
    # each step: python's Pendulum from the recorded state under (double)action; each return: the in-order sum of those rewards
    for e in range(n):
        env = Pendulum(C.ENV_SEED, horizon=horizon)
        env.c = c0 + e * horizon
        env.reset()
        assert np.array_equal(_bits(np.asarray(env.s)), _bits(states[e, 0])), ("start", e)
        ret = 0.0
        for t in range(horizon):
            env.s, env.steps = states[e, t].copy(), 0
            _, reward, _, _ = env.step(np.asarray([np.float64(actions[e, t])]))
            assert np.array_equal(_bits(np.asarray(env.s)), _bits(states[e, t + 1])), (e, t)
            ret = ret + reward
        assert np.array_equal(_bits(np.asarray([ret])), _bits(got["out_return"][e:e + 1])), ("return", e)
    return frac


def _check_words(case, got):
    """The environment as the host loop leaves it after its last auto reset, the step count, the ticket back at zero."""
    from deeprl_amd.envs import Pendulum
    n, horizon = case.n, case.horizon
    last = Pendulum(C.ENV_SEED, horizon=horizon)
    last.c = case.c0 + n * horizon
    last.reset()
    assert (int(got["env_counter"][0]), int(got["ep_steps"][0]), int(got["out_steps"][0]), int(got["arrive"][0]), int(got["env_seed"][0])) == \
        (case.c0 + n * horizon, 0, n * horizon, 0, C.ENV_SEED)
    assert np.array_equal(_bits(got["env_state"]), _bits(np.asarray(last.s))) and np.array_equal(_bits(got["ep_return"]), _bits(np.zeros(1)))
    assert np.array_equal(_bits(got["param"]), _bits(case.flat_host)), "a parameter was written"


def _check_launch(dra, shape, n, horizon, junk, label):
    case = _Case(dra, shape, n, horizon, junk)
    assert case.launch() == 0
    got = case.snapshot()
    frac = _check_trajectory(case, got)
    _check_words(case, got)
    # the whole launch: a host loop of envs.Pendulum driven by dra_dpg_act on one row at a time
    host = E.evaluate(lambda obs: case.dpg_act_rows(np.asarray(obs).reshape(1, 3)), C.make_env(junk, horizon), n)
    for k, want in (("out_return", host["returns"]), ("out_state", host["states"]), ("env_state", host["state"])):
        assert np.array_equal(_bits(got[k]), _bits(np.asarray(want, dtype=np.float64).reshape(got[k].shape))), k
    assert np.array_equal(_bits(got["out_action"]), _bits(host["actions"].astype(np.float32)))
    assert (host["counter"], host["ep_steps"], host["ep_return"], host["steps"]) == (int(got["env_counter"][0]), 0, 0.0, int(got["out_steps"][0]))
    # a second launch from the same start: the same bits; the debug pointers null: the same returns and words, nothing recorded
    case.reset()
    assert case.launch() == 0
    again = case.snapshot()
    for k in got:
        if k not in ("act_in", "act_out"):
            assert np.array_equal(_bits(got[k]), _bits(again[k])), k
    case.reset()
    assert case.launch(debug=False) == 0
    plain = case.snapshot()
    for k in ("out_return", "out_steps", "env_state", "env_counter", "ep_steps", "ep_return", "env_seed", "arrive", "param"):
        assert np.array_equal(_bits(got[k]), _bits(plain[k])), k
    assert np.isnan(plain["out_state"]).all() and np.isnan(plain["out_action"]).all()
    record_parity("dpg_eval_%s_%s" % (label, C.shape_id(shape)), actor=frac)
    assert frac <= 1.0
    return got


@pytest.mark.parametrize("label", list(C.LAUNCHES))
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_eval_launch_on_its_own_trajectory_and_against_the_host_loop(dra, shape, label):  # noqa: F811
    n, horizon, junk = C.LAUNCHES[label]
    got = _check_launch(dra, shape, n, horizon, junk, label)
    want = C.restated(shape, label)
    worst = float(np.abs(got["out_return"] - want["returns"]).max())
    print("returns against the fp64 restatement: worst %.3e" % worst)
    assert int(got["env_counter"][0]) == want["counter"] and np.array_equal(_bits(got["env_state"]), _bits(want["state"]))


def test_eval_launch_at_the_zoo_s_count(dra):  # noqa: F811
    """20 episodes of 200 steps at (32, 24): two workgroups, the second with four live rows."""
    n, horizon = C.ZOO_LAUNCH
    _check_launch(dra, C.SHAPES[0], n, horizon, False, "zoo")


def test_refused_launches_return_einval_and_write_nothing(dra):  # noqa: F811
    case = _Case(dra, C.SHAPES[0], 5, 12, True)
    before = case.snapshot()
    assert case.launch(n_episodes=0) == -22 and case.launch(n_episodes=129) == -22 and case.launch(n_episodes=-1) == -22
    assert case.launch(horizon=0) == -22 and case.launch(horizon=65536 // 5 + 1) == -22
    assert case.launch(out_return=None) == -22 and case.launch(arrive=None) == -22 and case.launch(env_counter=None) == -22
    for field, bad in (("state_dim", 4), ("action_dim", 2), ("h1", 513), ("gate", 3)):
        wide = type(case.net)()
        ctypes.memmove(ctypes.byref(wide), ctypes.byref(case.net), ctypes.sizeof(wide))
        setattr(wide, field, bad)
        assert case.launch(net=wide) == -22, field
    after = case.snapshot()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
