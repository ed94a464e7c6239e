"""The acting launch of csrc/dpg_mlp.hip (dra_dpg_env_act) restated for tests/test_gpu_dpg_env.py: cases (parameters, environment
starts, staged words) from fixed seeds and `restate`, the launch in numpy fp64 scalars in the kernel's written operation order.
The environments are deeprl_amd.envs.Pendulum / SyntheticContinuous stepped from python (tests/test_dpg_env_host.py pins the
pendulum to csrc/pendulum_env.h's host build, tests/test_ppo_mlp_host.py the synthetic one to csrc/cont_env.h's)."""
import numpy as np
import torch

import dpg_restatement as R

ENV_PENDULUM, ENV_SYNTHETIC = 0, 1
MODE_WARMUP, MODE_GAUSS, MODE_OU = 0, 1, 2
MODES = {"warmup": MODE_WARMUP, "gauss": MODE_GAUSS, "ou": MODE_OU}
# (S, A, H1, H2, gate, environment): the issue's table
SHAPES = [(3, 1, 32, 24, 1, ENV_PENDULUM), (3, 1, 400, 300, 1, ENV_PENDULUM), (17, 6, 20, 12, 2, ENV_SYNTHETIC),
          (64, 16, 512, 512, 1, ENV_SYNTHETIC)]
EP_RING_CAP, EP_RING_COUNT0, STEP0 = 5, 3, 41          # the episode ring starts at row 3 of 5: the second episode wraps
OU = dict(theta=0.15, mu=0.0, dt=1e-2)
LOW, HIGH = -1.0, 1.0


def actor_params(shape, seed):
    """Canonical fp64 dict {'a.w1': ...} with fp32-representable values (dpg_restatement's names) for the actor alone."""
    s, a, h1, h2 = shape[:4]
    rs = np.random.RandomState(seed)
    f = lambda *sh, scale: torch.as_tensor((rs.standard_normal(sh) * scale).astype(np.float32).astype(np.float64))
    return {"a.w1": f(h1, s, scale=1.0 / np.sqrt(s)), "a.b1": f(h1, scale=0.1), "a.w2": f(h2, h1, scale=1.0 / np.sqrt(h1)),
            "a.b2": f(h2, scale=0.1), "a.w3": f(a, h2, scale=1.0 / np.sqrt(h2)), "a.b3": f(a, scale=0.1)}


def make_env(shape, seed, horizon, steps_before):
    """The host environment of a case after `steps_before` steps under fixed actions (so that counters, episode steps and returns
    are not zero), and its observation."""
    from deeprl_amd.envs import Pendulum, SyntheticContinuous
    s, a, kind = shape[0], shape[1], shape[5]
    env = Pendulum(seed, horizon=horizon) if kind == ENV_PENDULUM else SyntheticContinuous(seed, s, a, horizon=horizon)
    obs = env.reset()
    rs = np.random.RandomState(seed + 1000)
    for _ in range(steps_before):
        obs, _, done, _ = env.step(rs.uniform(-1, 1, a))
        if done:
            obs = env.reset()
    return env, obs


def env_arrays(env):
    """(env_state, counter, ep_steps, ep_return, seed) as the device holds them."""
    return (np.asarray(env.s, dtype=np.float64).copy(), int(env.c), int(getattr(env, "steps", 0)), float(env.ret), int(env.seed))


def restate(env, obs, a32, mode, v, x, x0, slot, cap, ring, ep, step_counter):
    """One launch on host copies, IN PLACE: env (stepped, auto reset), ring (dict frames [cap][S], actions [cap][A], rewards,
    masks), ep (dict rows [R][3], count).  a32: the fp32 actor output.  -> (behaviour action, x after, step counter after, error
    count, the observation after)."""
    a_dim = len(v)
    act = np.empty(a_dim, dtype=np.float64)
    x = np.array(x, dtype=np.float64, copy=True)
    for d in range(a_dim):
        a = float(np.float64(a32[d]))
        if mode == MODE_WARMUP:
            y = float(v[d])
        elif mode == MODE_GAUSS:
            y = a + float(v[d])
        else:
            x[d] = (x[d] + ((OU["theta"] * (OU["mu"] - x[d])) * OU["dt"])) + float(v[d])
            y = a + x[d]
        act[d] = LOW if y < LOW else (HIGH if y > HIGH else y)
    err = 0
    if slot < 0 or slot >= cap:
        slot, err = 0, 1
    ring["frames"][slot] = obs
    ring["actions"][slot] = act
    nxt, reward, done, info = env.step(act)
    ring["rewards"][slot] = reward
    ring["masks"][slot] = 0 if done else 1
    if done:
        ep["rows"][ep["count"] % ep["rows"].shape[0]] = (float(step_counter), 0.0, float(info["episodic_return"]))
        ep["count"] += 1
        nxt = env.reset()
        x = np.array(x0, dtype=np.float64, copy=True)
    return act, x, step_counter + 1, err, nxt


def actor64(params, obs, gate):
    """tanh(actor(float32(obs))) in fp64."""
    s = torch.as_tensor(np.asarray(obs, dtype=np.float32).astype(np.float64)).reshape(1, -1)
    return R.actor(params, s, gate).numpy().reshape(-1)
