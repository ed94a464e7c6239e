"""Device-resident vector environment for the on-policy agents (SURVEY.md section 8 f1 for A2C / PPO).

The synthetic Atari environment is a pure function of its frame counter (envs.SyntheticAtari: counter-hash frames,
rewards and terminals), so N of them need no state on the device at all: the host shadow (learner.SyntheticEpisodeStream,
one per environment, the same class the DQN device pipeline uses) lays out a whole rollout ahead of time -- per step and
environment the counter of the observation, its episode age, the reward and the terminal flag -- uploads that plan with
one copy, and `states(plan, t)` produces the uint8 [N,4,84,84] observations of step t with one kernel
(dra_synth_stacks).  Nothing crosses the host boundary inside a rollout: no D2H of actions, no H2D of frames; the
observations go through the same image normaliser table (f32(f64(v) / 255)) as host frames, so the arithmetic an agent
performs is bit-identical to the host-emulator path.
"""
import collections
import ctypes
from collections import namedtuple

import numpy as np
import torch

from ._lib import lib, stream_ptr
from .support import Config, StagedUpload

Plan = namedtuple("Plan", ["counters", "ages", "reward", "mask", "infos", "t_len"])


class VecEpisodeShadow:
    """N learner.SyntheticEpisodeStream objects advanced in lockstep with numpy vector arithmetic (one python iteration per
    rollout STEP instead of one per transition: the scalar shadow costs ~20 us per transition, 20 ms of a PPO rollout of
    1024).  Same state per environment: the counter of the current observation (c), its episode age, the next counter to
    hand out, the running return."""

    def __init__(self, seeds, counters0, done_periods, history):
        n = len(seeds)
        self.seeds = np.asarray(seeds, dtype=np.int64)
        self.done_periods = np.asarray(done_periods, dtype=np.int64)
        self.history = int(history)
        self.next_counter = np.asarray(counters0, dtype=np.int64).copy()
        self.c = self.next_counter.copy()           # reset(): one new frame per environment
        self.next_counter += 1
        self.age = np.zeros(n, dtype=np.int32)
        self.ret = np.zeros(n, dtype=np.float64)

    def step(self):
        """One transition of every environment -> (counter, age, reward, done, episodic_return-or-nan) arrays."""
        from .envs import synthetic_reward_done_vec
        counter, age = self.c.copy(), self.age.copy()
        rc = self.next_counter.copy()               # reward / done are hashed from the counter of the frame step() generates
        reward, done = synthetic_reward_done_vec(rc, self.seeds, self.done_periods)
        self.next_counter += 1
        self.ret += reward
        ep_ret = np.where(done, self.ret, np.nan)
        # done: DummyVecEnv drops the post-step frame and resets (a new frame, the stack restarts, the return too)
        self.c = np.where(done, self.next_counter, rc)
        self.next_counter += done.astype(np.int64)
        self.age = np.where(done, 0, np.minimum(age + 1, self.history - 1)).astype(np.int32)
        self.ret = np.where(done, 0.0, self.ret)
        return counter, age, reward, done, ep_ret


class DeviceAtariVec:
    """Task surface (state_dim / action_dim / action_space ...) over the environments of `task`, observations on device."""
    on_device = True

    def __init__(self, task):
        envs = task.env.envs
        self.task = task
        self.name, self.state_dim, self.action_dim = task.name, task.state_dim, task.action_dim
        self.observation_space, self.action_space = task.observation_space, task.action_space
        self.num_envs, self.history = len(envs), envs[0].history
        self.shadow = VecEpisodeShadow([e.seed for e in envs], [e.counter for e in envs], [e.done_period for e in envs],
                                       envs[0].history)
        for e in envs:
            e.frames = "device"         # the host emulators are retired: stepping them too would fork the streams
        dev = Config.DEVICE
        self.seeds = torch.tensor([e.seed for e in envs], dtype=torch.int64, device=dev)
        self._bufs = {}
        self._no_info = tuple({'episodic_return': None} for _ in envs)

    @staticmethod
    def eligible(task, config):
        """`task` is an envs.Task over fresh synthetic Atari emulators and the configuration can consume device frames."""
        from .envs import DummyVecEnv, SyntheticAtari, Task
        from .normalizers import RescaleNormalizer
        if Config.DEVICE.type != 'cuda' or getattr(config, 'device_env', True) is False or type(task) is not Task:
            return False
        env = getattr(task, 'env', None)
        if type(env) is not DummyVecEnv or not env.envs:
            return False
        if not all(type(e) is SyntheticAtari and e.frames is None and e.history == env.envs[0].history for e in env.envs):
            return False
        return isinstance(config.state_normalizer, RescaleNormalizer)

    def reset(self):
        return None     # observations come from states(plan, t); the first one is every stream's initial reset

    def _static(self, t_len):
        """Persistent device buffer + rotating pinned staging of one rollout plan (graph replays read the same addresses)."""
        if t_len not in self._bufs:
            n = self.num_envs
            words = (t_len + 1) * n * 2 + (t_len + 1) * n + 2 * t_len * n      # i64 counters | i32 ages | f32 reward, mask
            self._bufs[t_len] = StagedUpload(words * 4 + 16, torch.uint8, Config.DEVICE)
        return self._bufs[t_len]

    def plan(self, t_len, reward_normalizer):
        """Advances every environment by t_len transitions on the host shadow and uploads what the device needs."""
        n = self.num_envs
        up = self._static(t_len)
        raw = up.stage().numpy()
        o1 = (t_len + 1) * n * 8
        o2 = o1 + (t_len + 1) * n * 4
        o3 = o2 + t_len * n * 4
        counters = raw[:o1].view(np.int64).reshape(t_len + 1, n)
        ages = raw[o1:o2].view(np.int32).reshape(t_len + 1, n)
        reward = raw[o2:o3].view(np.float32).reshape(t_len, n)
        mask = raw[o3:o3 + t_len * n * 4].view(np.float32).reshape(t_len, n)
        infos = []
        sh = self.shadow
        for t in range(t_len):
            c, age, rew, done, ep_ret = sh.step()
            counters[t], ages[t], mask[t] = c, age, 1.0 - done
            reward[t] = np.asarray(reward_normalizer(rew), dtype=np.float32)       # what tensor(rewards) uploads
            infos.append(tuple({'episodic_return': float(r) if d else None} for r, d in zip(ep_ret, done)) if done.any()
                         else self._no_info)
        counters[t_len], ages[t_len] = sh.c, sh.age   # the observation the NEXT rollout starts from (bootstrap value)
        d = up.send()
        return Plan(counters=d[:o1].view(torch.int64).view(t_len + 1, n), ages=d[o1:o2].view(torch.int32).view(t_len + 1, n),
                    reward=d[o2:o3].view(torch.float32).view(t_len, n, 1), mask=d[o3:o3 + t_len * n * 4].view(torch.float32).view(t_len, n, 1),
                    infos=infos, t_len=t_len)

    def states(self, plan, t):
        """uint8 [N, history, 84, 84] observations of rollout step t (t = t_len: the bootstrap observation)."""
        out = torch.empty((self.num_envs, self.history, 84, 84), dtype=torch.uint8, device=Config.DEVICE)
        lib.dra_synth_stacks(ctypes.c_void_p(plan.counters[t].data_ptr()), ctypes.c_void_p(plan.ages[t].data_ptr()),
                             ctypes.c_void_p(self.seeds.data_ptr()), self.num_envs, self.history,
                             ctypes.c_void_p(out.data_ptr()), stream_ptr())
        return out

    def states_all(self, plan):
        """uint8 [t_len + 1, N, history, 84, 84]: the observations of every step of the planned rollout (row t_len: the
        bootstrap observation) from ONE launch -- the environment is a pure function of the planned counters, so nothing orders
        observation t + 1 behind action t; states(plan, t) row by row costs a launch per rollout step."""
        rows = (plan.t_len + 1) * self.num_envs
        key = ('seeds', plan.t_len)
        if key not in self._bufs:
            self._bufs[key] = self.seeds.repeat(plan.t_len + 1).contiguous()
        out = torch.empty((plan.t_len + 1, self.num_envs, self.history, 84, 84), dtype=torch.uint8, device=Config.DEVICE)
        lib.dra_synth_stacks(ctypes.c_void_p(plan.counters.data_ptr()), ctypes.c_void_p(plan.ages.data_ptr()),
                             ctypes.c_void_p(self._bufs[key].data_ptr()), rows, self.history, ctypes.c_void_p(out.data_ptr()),
                             stream_ptr())
        return out

    def step(self, actions):
        raise RuntimeError("DeviceAtariVec is driven through plan() / states(); its environments are not steppable one by one")

    def close(self):
        return


class _RolloutVec:
    """What the device-resident vector environments behind a one-launch rollout share (DeviceContinuousVec, DeviceCartPoleVec):
    the Task surface, the task's own eligibility, the output buffers per rollout length and the environment-independent fields
    of a rollout_io struct."""
    on_device = True

    def __init__(self, task):
        envs = task.env.envs
        self.task = task
        self.name, self.state_dim, self.action_dim = task.name, task.state_dim, task.action_dim
        self.observation_space, self.action_space = task.observation_space, task.action_space
        self.num_envs, self.horizon = len(envs), int(envs[0].horizon)
        self._bufs = {}

    def _retire_host(self):
        for e in self.task.env.envs:
            e.s = "device"          # the host objects are retired: stepping them too would fork the streams

    @staticmethod
    def _host_envs(task, config):
        """The environments of an envs.Task over a DummyVecEnv of at most 64, with a device and config.device_env on; else None."""
        from .envs import DummyVecEnv, Task
        if Config.DEVICE.type != 'cuda' or getattr(config, 'device_env', True) is False or type(task) is not Task:
            return None
        env = getattr(task, 'env', None)
        if type(env) is not DummyVecEnv or not env.envs or len(env.envs) > 64:
            return None
        return env.envs

    def buffers(self, t_len):
        if t_len not in self._bufs:
            dev = Config.DEVICE
            self._bufs[t_len] = self._new_buffers(t_len, lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev))
        return self._bufs[t_len]

    def fill_io(self, io, agent, t_len):
        """The fields every rollout_io struct over these environments has, an out_* pointer per buffer it takes and, where the
        struct has them, the rank-invariant sampler's fields (an io struct without sampler_step brings a counter of its own);
        returns the buffers."""
        b = self.buffers(t_len)
        io.env_state, io.env_counter, io.env_seed = self.env_state.data_ptr(), self.env_counter.data_ptr(), self.env_seed.data_ptr()
        for k, v in b.items():
            if hasattr(io, 'out_' + k):
                setattr(io, 'out_' + k, v.data_ptr())
        if hasattr(io, 'sampler_step'):
            dp = agent.dp
            io.sampler_step = dp.step_dev.data_ptr()
            io.env0, io.n_global, io.noise_seed = dp.lo, dp.global_workers, agent._noise_seed
        io.horizon, io.reward_coef = self.horizon, float(agent.config.reward_normalizer.coef)
        io.t_len, io.n_env = int(t_len), self.num_envs
        return b

    def reset(self):
        return None

    close = reset

    def step(self, actions):
        raise RuntimeError("%s is driven through %s's device rollout; its environments are not steppable"
                           % (type(self).__name__, self.DRIVER))


class DeviceContinuousVec(_RolloutVec):
    """The SyntheticContinuous environments of a Task, resident on the device (BASELINE configs[2]: PPO, 16 HalfCheetah-shaped
    workers): raw fp64 observations, step counters and the observation normaliser's running statistics live in HBM and one
    launch (dra_ppo_mlp_rollout) walks a whole rollout -- normalise, both forwards, sample, environment step -- without a host
    round trip.  Rewards and terminals are hashes of (seed, counter) alone, so the host keeps a shadow of them (vectorised,
    one pass per rollout) for the episodic-return log lines; observations depend on the actions and exist only on the device.
    Same arithmetic as envs.SyntheticContinuous + normalizers.MeanStdNormalizer stepped from python (csrc/cont_env.h;
    tests/test_gpu_ppo_mlp.py compares the two paths)."""
    DRIVER = "PPOAgent"

    def __init__(self, task, agent_states, normalizer):
        """task: the envs.Task whose (already reset) environments move to the device; agent_states: the normalised observations
        the agent holds (what config.state_normalizer(task.reset()) returned); normalizer: config.state_normalizer."""
        from .normalizers import MeanStdNormalizer
        _RolloutVec.__init__(self, task)
        envs = task.env.envs
        dev = Config.DEVICE
        self.seeds_host = np.asarray([e.seed for e in envs], dtype=np.int64)
        self.counters_host = np.asarray([e.c for e in envs], dtype=np.int64)
        self.ret_host = np.asarray([e.ret for e in envs], dtype=np.float64)
        self.env_state = torch.from_numpy(np.stack([e.s for e in envs]).astype(np.float64)).to(dev)
        self.env_counter = torch.from_numpy(self.counters_host.copy()).to(dev)
        self.env_seed = torch.from_numpy(self.seeds_host.copy()).to(dev)
        self.cur_state = torch.from_numpy(np.ascontiguousarray(np.asarray(agent_states, dtype=np.float32))).to(dev)
        s = self.state_dim
        rms = np.zeros(2 * s + 1, dtype=np.float64)
        self.normalizer = normalizer
        if isinstance(normalizer, MeanStdNormalizer):
            rms[:s], rms[s:2 * s], rms[2 * s] = normalizer.rms.mean.reshape(-1), normalizer.rms.var.reshape(-1), normalizer.rms.count
            self.rms_epsilon, self.rms_clip, self.rms_kind = float(normalizer.epsilon), float(normalizer.clip), 'meanstd'
        else:       # RescaleNormalizer(1.0): (x - 0) / sqrt(1 + 0) = x exactly, no clipping, no statistics
            rms[s:2 * s] = 1.0
            self.rms_epsilon, self.rms_clip, self.rms_kind = 0.0, float('inf'), 'identity'
        self.rms = torch.from_numpy(rms).to(dev)
        if self.rms_kind == 'meanstd':
            normalizer.attach_device(self.rms, s)
        self._retire_host()

    @staticmethod
    def eligible(task, config):
        from .envs import SyntheticContinuous
        from .normalizers import MeanStdNormalizer, RescaleNormalizer
        envs = _RolloutVec._host_envs(task, config)
        if envs is None:
            return False
        e0 = envs[0]
        if not all(type(e) is SyntheticContinuous and e.horizon == e0.horizon and e.state_dim == e0.state_dim and
                   e.action_dim == e0.action_dim for e in envs):
            return False
        sn, rn = config.state_normalizer, config.reward_normalizer
        state_ok = type(sn) is MeanStdNormalizer or (type(sn) is RescaleNormalizer and sn.coef == 1.0)
        return state_ok and type(rn) is RescaleNormalizer

    def _new_buffers(self, t_len, f):
        n, s, a = self.num_envs, self.state_dim, self.action_dim
        return dict(state=f(t_len, n, s), action=f(t_len, n, a), log_pi_a=f(t_len, n, 1), v=f(t_len + 1, n, 1),
                    reward=f(t_len, n, 1), mask=f(t_len, n, 1))

    def fill_io(self, io, agent, t_len, read_only):
        """_RolloutVec.fill_io and the observation normaliser's fields (a2c_mlp.RolloutIO, ppo_mlp.RolloutIO)."""
        b = _RolloutVec.fill_io(self, io, agent, t_len)
        io.rms, io.cur_state = self.rms.data_ptr(), self.cur_state.data_ptr()
        io.rms_epsilon, io.rms_clip = self.rms_epsilon, self.rms_clip
        io.rms_update = 1 if (self.rms_kind == 'meanstd' and not read_only) else 0
        return b

    def shadow(self, t_len):
        """Advances the host shadow by t_len steps of every environment -> list of (t, env, episodic_return) for the episodes
        that end inside the rollout (envs.SyntheticContinuous.step's reward / done / return arithmetic, vectorised)."""
        from .envs import _GOLD, _mix64
        n = self.num_envs
        c = (self.counters_host[None, :] + np.arange(1, t_len + 1, dtype=np.int64)[:, None]).astype(np.uint64)     # [T, N]
        with np.errstate(over="ignore"):
            sd = self.seeds_host.astype(np.uint64)[None, :] * np.uint64(8)
            base_r = (sd + np.uint64(2)) * _GOLD + c * np.uint64(64)
            u = [(_mix64(base_r + np.uint64(j)) >> np.uint64(11)).astype(np.float64) * 1.1102230246251565e-16 for j in range(4)]
            done = (_mix64((sd + np.uint64(3)) * _GOLD + c * np.uint64(64)) % np.uint64(self.horizon)) == 0
        reward = (((u[0] + u[1]) + (u[2] + u[3])) - 2.0) * 1.7320508075688772
        events = []
        for i in range(n):
            ends = np.nonzero(done[:, i])[0]
            start, carry = 0, self.ret_host[i]
            for t in ends:
                carry = float(np.cumsum(np.concatenate([[carry], reward[start:t + 1, i]]))[-1])
                events.append((int(t), i, carry))
                start, carry = int(t) + 1, 0.0
            self.ret_host[i] = float(np.cumsum(np.concatenate([[carry], reward[start:, i]]))[-1])
        self.counters_host += t_len
        events.sort()
        return events


class DeviceCartPoleVec(_RolloutVec):
    """The envs.CartPole environments of a Task, resident on the device (a2c_feature, examples.py:340-358, under A2CAgent;
    n_step_dqn_feature, examples.py:408-424, under NStepDQNAgent; option_critic_feature, examples.py:450-468, under
    OptionCriticAgent): fp64 state, total step counters, episode steps and running returns live in HBM and one launch
    (dra_cat_mlp_rollout / dra_q_mlp_rollout / dra_oc_mlp_rollout) walks a whole rollout -- forward, action,
    environment step -- without a host round trip.  Same arithmetic as envs.CartPole stepped from python (csrc/cartpole_env.h;
    the two agents' GPU tests compare the two).  `buffers(t_len, n, zeros)`: what the kernel leaves besides state and action.

    The terminals depend on the actions, so the host cannot shadow them (DeviceContinuousVec.shadow has no counterpart here).
    Episode ends are REPORTED by the device instead: the rollout kernel (csrc/cartpole_rollout.h) appends one row (its stamp
    of the end -- A2C: the sampler step, n-step DQN and option-critic: their step counter --, global environment, episodic return) per finished
    episode to `ep_ring` [RING_CAP][3] and counts them in `ep_count`; `drain()` is one device-to-host copy (EpisodeRing)."""
    DRIVER = "A2CAgent / NStepDQNAgent / OptionCriticAgent"
    RING_CAP = 4096
    HOST_NOTE = 'the cart-pole environments stay on the host and this agent keeps the module path: %s'

    def __init__(self, task, buffers=None):
        _RolloutVec.__init__(self, task)
        self._more_buffers = buffers or (lambda t_len, n, f: dict(v=f(t_len + 1, n, 1), reward=f(t_len, n, 1), mask=f(t_len, n, 1)))
        envs = task.env.envs
        dev = Config.DEVICE
        self.ring_cap = int(self.RING_CAP)
        self.env_state = torch.from_numpy(np.stack([np.asarray(e.s, dtype=np.float64) for e in envs])).to(dev)
        self.env_counter = torch.tensor([e.c for e in envs], dtype=torch.int64, device=dev)
        self.ep_steps = torch.tensor([e.steps for e in envs], dtype=torch.int32, device=dev)
        self.ep_return = torch.tensor([e.ret for e in envs], dtype=torch.float64, device=dev)
        self.env_seed = torch.tensor([e.seed for e in envs], dtype=torch.int64, device=dev)
        # [0:3 cap] the ring's rows, [3 cap] the count (as fp64 bits of an int64 view): ONE buffer, so that drain() is one copy
        self._ring_buf = torch.zeros(3 * self.ring_cap + 1, dtype=torch.float64, device=dev)
        self.ep_ring = self._ring_buf[:3 * self.ring_cap].view(self.ring_cap, 3)
        self.ep_count = self._ring_buf[3 * self.ring_cap:].view(torch.int64)
        self._ring_host = torch.zeros(3 * self.ring_cap + 1, dtype=torch.float64).pin_memory()
        self.drained = 0
        self._retire_host()

    @staticmethod
    def eligible(task, config):
        from .envs import CartPole
        from .normalizers import RescaleNormalizer
        envs = _RolloutVec._host_envs(task, config)
        if envs is None or not all(type(e) is CartPole and e.horizon == envs[0].horizon for e in envs):
            return False
        sn, rn = config.state_normalizer, config.reward_normalizer
        return type(sn) is RescaleNormalizer and sn.coef == 1.0 and type(rn) is RescaleNormalizer

    def _new_buffers(self, t_len, f):
        n = self.num_envs
        return dict(state=f(t_len, n, self.state_dim), action=torch.zeros((t_len, n), dtype=torch.int64, device=Config.DEVICE),
                    **self._more_buffers(t_len, n, f))

    def fill_io(self, io, agent, t_len):
        """_RolloutVec.fill_io and the episode bookkeeping's fields (cat_mlp.RolloutIO, q_mlp.RolloutIO, oc_mlp.RolloutIO)."""
        b = _RolloutVec.fill_io(self, io, agent, t_len)
        io.ep_steps, io.ep_return = self.ep_steps.data_ptr(), self.ep_return.data_ptr()
        io.ep_count, io.ep_ring, io.ring_cap = self.ep_count.data_ptr(), self.ep_ring.data_ptr(), self.ring_cap
        return b

    def drain(self):
        """The episodes that ended since the last drain -> list of (the kernel's stamp, global environment, episodic return) in the
        order they were appended ((step, environment) order).  One device-to-host copy; raises when more than RING_CAP rows were
        pending (the oldest have been overwritten)."""
        self._ring_host.copy_(self._ring_buf, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.rows_since_drain(self._ring_host.numpy())

    def rows_since_drain(self, host):
        """drain() over `host`, a host copy of _ring_buf that the caller made (seed_batch.py: the rings of all lanes in one copy)."""
        count = int(host[3 * self.ring_cap:].view(np.int64)[0])
        pending = count - self.drained
        if pending > self.ring_cap:
            raise RuntimeError("DeviceCartPoleVec: %d episodes ended since the last drain, the ring holds %d: drain more often "
                               "(config.episode_drain_interval)" % (pending, self.ring_cap))
        rows = host[:3 * self.ring_cap].reshape(self.ring_cap, 3)
        out = [(int(r[0]), int(r[1]), float(r[2])) for r in (rows[k % self.ring_cap] for k in range(self.drained, count))]
        self.drained = count
        return out

    def state_dict(self):
        """Everything a loaded run needs to continue bit for bit (host copies)."""
        torch.cuda.current_stream().synchronize()
        keys = ("env_state", "env_counter", "ep_steps", "ep_return", "env_seed", "_ring_buf")
        d = {k: getattr(self, k).cpu().numpy().copy() for k in keys}
        d["drained"] = int(self.drained)
        return d

    def load_state_dict(self, d):
        for k in ("env_state", "env_counter", "ep_steps", "ep_return", "env_seed", "_ring_buf"):
            getattr(self, k).copy_(torch.from_numpy(np.asarray(d[k])))
        self.drained = int(d["drained"])


class DevicePendulumVec(DeviceCartPoleVec):
    """The ONE continuous-control environment of a DDPGAgent / TD3Agent's Task, resident on the device (ddpg_continuous /
    td3_continuous, examples.py:554-617, under config.fused_dpg_env): an envs.Pendulum -- env_state [1][2] = (theta, theta'), the
    observation [cos, sin, theta'] is formed by the kernel (csrc/pendulum_env.h) -- or an envs.SyntheticContinuous -- env_state
    [1][state_dim], csrc/cont_env.h; ep_steps stays 0.  DeviceCartPoleVec's surface as it is: counter, seed, episode steps /
    return, the episode ring and `drain()`; dra_dpg_env_act (dpg_env.EnvStep) walks one transition per launch and writes it
    straight into the replay ring."""
    DRIVER = "DDPGAgent / TD3Agent"
    HOST_NOTE = 'fused_dpg_env is on but the environment stays on the host and this agent keeps its host step: %s'

    def __init__(self, task):
        _RolloutVec.__init__(self, task)
        self._more_buffers = lambda t_len, n, f: {}
        env = task.env.envs[0]
        dev = Config.DEVICE
        self.ring_cap = int(self.RING_CAP)
        self.env_state = torch.from_numpy(np.asarray(env.s, dtype=np.float64).reshape(1, -1).copy()).to(dev)
        self.env_counter = torch.tensor([env.c], dtype=torch.int64, device=dev)
        # (a SyntheticContinuous ends its episodes by a hash of the counter and counts no episode steps)
        from .envs import Pendulum
        self.ep_steps = torch.tensor([env.steps if type(env) is Pendulum else 0], dtype=torch.int32, device=dev)
        self.ep_return = torch.tensor([env.ret], dtype=torch.float64, device=dev)
        self.env_seed = torch.tensor([env.seed], dtype=torch.int64, device=dev)
        self._ring_buf = torch.zeros(3 * self.ring_cap + 1, dtype=torch.float64, device=dev)      # DeviceCartPoleVec's layout
        self.ep_ring = self._ring_buf[:3 * self.ring_cap].view(self.ring_cap, 3)
        self.ep_count = self._ring_buf[3 * self.ring_cap:].view(torch.int64)
        self._ring_host = torch.zeros(3 * self.ring_cap + 1, dtype=torch.float64).pin_memory()
        self.drained = 0
        self._retire_host()

    @staticmethod
    def eligible(task, config):
        from .envs import Pendulum, SyntheticContinuous
        from .normalizers import RescaleNormalizer
        envs = _RolloutVec._host_envs(task, config)
        if envs is None or len(envs) != 1 or type(envs[0]) not in (Pendulum, SyntheticContinuous):
            return False
        sn, rn = config.state_normalizer, config.reward_normalizer
        return type(sn) is RescaleNormalizer and sn.coef == 1.0 and type(rn) is RescaleNormalizer and rn.coef == 1.0


class EpisodeRing:
    """The host's reader of DeviceCartPoleVec's episode ring, owned by the agent that drives the rollouts.  The kernel stamps a row
    with its own counter: t_len + `bootstrap_stamps` per rollout (A2C: 1, the sampler's bootstrap slot; n-step DQN: 0).  `stamp`
    follows it on the host; the anchor (stamp, agent.total_steps, t_len) taken at the first rollout of a rollout length turns a row
    into the step number the host path logs -- total_steps at the start of the episode's rollout + t * n_global + environment."""
    LOG = 16384

    def __init__(self, agent, bootstrap_stamps, n_global):
        self.agent, self.extra, self.n_global = agent, int(bootstrap_stamps), int(n_global)
        self.stamp, self.anchor, self.steps = 0, None, 0
        self.log = collections.deque(maxlen=self.LOG)

    def begin(self, t_len):
        # ahead of a rollout of t_len steps (and of the agent's total_steps advancing)
        if self.anchor is None or self.anchor[2] != t_len:
            self.drain()       # (what is pending was appended under the old rollout length)
            self.anchor = (self.stamp, self.agent.total_steps, t_len)
        self.stamp += t_len + self.extra

    def end(self):
        # behind an agent step: drains every config.episode_drain_interval of them
        self.steps += 1
        if self.steps % max(1, int(getattr(self.agent.config, 'episode_drain_interval', 64))) == 0:
            self.drain()

    def drain(self):
        """Fetches the episodes that ended on the device since the last drain (one copy) and emits the reference's
        'episodic_return_train' lines for them, late (up to config.episode_drain_interval agent steps) but with the host path's
        step numbers.  Returns the (step, return) pairs of this drain; nothing before the first device rollout."""
        if self.anchor is None:
            return []
        s0, total0, t_len = self.anchor
        out = []
        for s, i, ret in self.agent.task.drain():
            k, t = divmod(s - s0, t_len + self.extra)
            at = total0 + (k * t_len + t) * self.n_global + i
            self.agent.log_train_return(ret, at)
            out.append((at, ret))
        self.log.extend(out)
        return out

    def episodes(self):
        """(step, return) of the training episodes since the previous call (the newest LOG), after a drain; empty on host paths."""
        self.drain()
        out = list(self.log)
        self.log.clear()
        return out

    def state_dict(self):
        return dict(envs=self.agent.task.state_dict())

    def load_state_dict(self, state):
        """From a side file's dict: `step` is the kernel's counter, `envs` (absent in files older than the ring) the arrays."""
        self.drain()
        self.stamp, self.anchor = int(state['step']), None
        if 'envs' in state:
            self.agent.task.load_state_dict(state['envs'])
