"""Host side of csrc/dpg_mlp.hip's dra_dpg_env_act: ddpg_continuous / td3_continuous (examples.py:554-617) over ONE
device-resident environment -- envs.Pendulum (csrc/pendulum_env.h) or envs.SyntheticContinuous (csrc/cont_env.h) -- and the HBM
replay ring, behind the opt-in switch `config.fused_dpg_env` (with `config.fused_dpg_update`, which must be on too).

`why_not(agent)` names the first condition that keeps a DDPGAgent / TD3Agent on its host path; `EnvStep(agent)` is the agent step
without a host round trip (DDPG_agent.py:62-100): the host makes the step's draws in the reference's order -- `space.sample()`
during warm-up, else the random process's standard normals, then the minibatch's rejection loop once warm -- and stages mode,
noise vector, ring slot, the action bounds and the indices in ONE block at fixed addresses; dra_dpg_env_act runs the transition
and writes it into the ring; ring.gather on the staged device indices and dpg_mlp.Update.learn follow on the same stream.  All
launches are eager (Adam's step size and the smoothing-noise counter travel by value).  The Ornstein-Uhlenbeck state lives on
the device; the host keeps drawing its diffusion term.  Resuming the device environment from a checkpoint is not supported:
save / load keep the parameters, as on the host path.
There is no CPU / eager-PyTorch implementation here: without the HIP library every call raises.
"""
import ctypes

import numpy as np
import torch

from ._lib import DraError, lib, stream_ptr
from .device_env import DevicePendulumVec, EpisodeRing, _RolloutVec
from .support import Config, StagedUpload

SWITCH = 'fused_dpg_env'
ENV_PENDULUM, ENV_SYNTHETIC = 0, 1
MODE_WARMUP, MODE_GAUSS, MODE_OU = 0, 1, 2


class ActIO(ctypes.Structure):
    """Mirror of dra_dpg_env_act_io (include/deeprl_amd.h)."""
    _fields_ = [("env_state", ctypes.c_void_p), ("env_counter", ctypes.c_void_p), ("ep_steps", ctypes.c_void_p),
                ("ep_return", ctypes.c_void_p), ("env_seed", ctypes.c_void_p), ("step_counter", ctypes.c_void_p),
                ("ep_count", ctypes.c_void_p), ("ep_ring", ctypes.c_void_p),
                ("mode", ctypes.c_void_p), ("slot", ctypes.c_void_p), ("bounds", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("ou_x", ctypes.c_void_p), ("ou_x0", ctypes.c_void_p),
                ("ring_frames", ctypes.c_void_p), ("ring_actions", ctypes.c_void_p), ("ring_rewards", ctypes.c_void_p),
                ("ring_masks", ctypes.c_void_p), ("out_action", ctypes.c_void_p), ("err", ctypes.c_void_p),
                ("horizon", ctypes.c_int64), ("ring_cap", ctypes.c_int64), ("capacity", ctypes.c_int64),
                ("ou_theta", ctypes.c_double), ("ou_mu", ctypes.c_double), ("ou_dt", ctypes.c_double),
                ("env_kind", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def supported(env_kind, state_dim, action_dim, h1, h2, gate):
    """dra_dpg_env_act_supported: the shapes the acting kernel is built for (host-only: no GPU needed)."""
    return lib.dra_dpg_env_act_supported.raw(int(env_kind), int(state_dim), int(action_dim), int(h1), int(h2), int(gate)) == 0


def env_kind(env):
    from .envs import Pendulum, SyntheticContinuous
    return {Pendulum: ENV_PENDULUM, SyntheticContinuous: ENV_SYNTHETIC}.get(type(env))


def why_not(agent, supported_fn=supported, update_why_not=None):
    """None when `agent` (a DDPGAgent / TD3Agent nobody has stepped) may run on dra_dpg_env_act, else the first reason it may not."""
    from . import dpg_mlp
    from .normalizers import RescaleNormalizer
    from .random_process import GaussianProcess, OrnsteinUhlenbeckProcess
    from .replay import UniformReplay
    cfg = agent.config
    if getattr(cfg, SWITCH, False) is not True:
        return "config.%s is not on" % SWITCH
    why = (update_why_not or dpg_mlp.why_not)(agent)
    if why is not None:
        return "the fused update is not available (%s)" % why
    envs = _RolloutVec._host_envs(agent.task, cfg)
    if envs is None or len(envs) != 1 or env_kind(envs[0]) is None:
        return "the task is not one envs.Pendulum or envs.SyntheticContinuous environment, or there is no device"
    env = envs[0]
    if agent.state is not None or agent.total_steps != 0 or env.c != 0 or isinstance(env.s, str):
        return "the environment has already been stepped on the host"
    sn, rn = cfg.state_normalizer, cfg.reward_normalizer
    if type(sn) is not RescaleNormalizer or sn.coef != 1.0:
        return "the state normaliser is not RescaleNormalizer(1.0)"
    if type(rn) is not RescaleNormalizer or rn.coef != 1.0:
        return "the reward normaliser is not RescaleNormalizer(1.0)"
    rp = agent.random_process
    if type(rp) not in (GaussianProcess, OrnsteinUhlenbeckProcess):
        return "the random process is not exactly GaussianProcess or OrnsteinUhlenbeckProcess"
    shp = dpg_mlp.shape(agent.network)
    if tuple(rp.size) != (shp[1],):
        return "the random process does not draw one value per action dimension"
    ring = getattr(agent.replay, 'replay', agent.replay)
    if type(ring) is not UniformReplay or ring.n_step != 1 or ring.history_length != 1 or ring.size() != 0:
        return "the replay is not an empty one-step UniformReplay"
    if int(ring.memory_size) < 2:
        return "the replay holds fewer than two slots"
    if (agent.task.state_dim, agent.task.action_dim) != (shp[0], shp[1]):
        return "the network's state and action sizes are not the task's"
    if not supported_fn(env_kind(env), *shp[:5]):
        return "dra_dpg_env_act_supported refuses (S, A, H1, H2, gate) = %r on this environment" % (shp[:5],)
    return None


def adopt(agent):
    """An EnvStep with the agent's environment on the device when configuration, agent and task allow it; else None (the host
    path; with the switch on the reason is logged in one warning)."""
    why = why_not(agent)
    if why is not None:
        if getattr(agent.config, SWITCH, False) is True:
            getattr(agent.logger, 'warning', agent.logger.info)(DevicePendulumVec.HOST_NOTE % why)
        return None
    return EnvStep(agent)


class EnvStep:
    """One DDPGAgent / TD3Agent step on the kernels: see the module's docstring."""

    def __init__(self, agent):
        from .random_process import OrnsteinUhlenbeckProcess
        dev = Config.DEVICE
        self.agent = agent
        self.update = agent._fused_dpg()
        self.shape = shp = self.update.shape
        s_dim, a_dim = shp[0], shp[1]
        self.launches = 0
        # the environment moves as reset() leaves it (DDPG_agent.py:64-66: the first step resets the process and the task)
        agent.random_process.reset_states()
        task = agent.task
        self.kind = env_kind(task.env.envs[0])
        task.reset()
        self.vec = DevicePendulumVec(task)
        agent.task = self.vec           # (device_env.EpisodeRing reads the episodes through agent.task)
        agent.state = "device"
        self.ring_log = EpisodeRing(agent, 0, 1)
        rp = self.replay = getattr(agent.replay, 'replay', agent.replay)
        rp._lazy_ring(np.zeros(s_dim, dtype=np.float64), np.zeros(a_dim, dtype=np.float64))      # what the first feed() would create
        self.ring = rp._ring
        if self.ring.frame_bytes != 8 * s_dim or self.ring.action_bytes != 8 * a_dim:
            raise DraError("dpg_env: the replay ring holds frames of %d and actions of %d bytes" % (self.ring.frame_bytes, self.ring.action_bytes))
        self.capacity, self.batch = int(rp.memory_size), int(rp.batch_size)
        # ONE staged block at fixed addresses: int64 mode | int64 slot | fp64 low, high | fp64 v [A] | int64 indices [B]
        self._o_v, self._o_idx = 32, 32 + 8 * a_dim
        self._up = StagedUpload(self._o_idx + 8 * self.batch, torch.uint8, dev)
        d = self._up.dev
        self.mode, self.slot = d[:8].view(torch.int64), d[8:16].view(torch.int64)
        self.bounds, self.v = d[16:32].view(torch.float64), d[self._o_v:self._o_idx].view(torch.float64)
        self.idx = d[self._o_idx:].view(torch.int64)
        proc = agent.random_process
        self.ou = type(proc) is OrnsteinUhlenbeckProcess
        x0 = np.broadcast_to(np.asarray(proc.x_prev if self.ou else 0.0, dtype=np.float64), (a_dim,)).copy()
        self.ou_x0 = torch.from_numpy(x0).to(dev)
        self.ou_x = self.ou_x0.clone()
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)      # the kernel's own step counter (the episode rows' stamp)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)           # staged slots the kernel found out of range
        self.out_action = torch.zeros(a_dim, dtype=torch.float32, device=dev)
        self.static = None              # the minibatch's buffers (ring.gather refills them in place)
        self.last_draws = None          # (mode, v, slot, indices or None) of the last step, as drawn

    def act_io(self):
        """dra_dpg_env_act_io over the environment, the staged draws and the ring."""
        v, io, proc = self.vec, ActIO(), self.agent.random_process
        io.env_state, io.env_counter, io.env_seed = v.env_state.data_ptr(), v.env_counter.data_ptr(), v.env_seed.data_ptr()
        io.ep_steps, io.ep_return = v.ep_steps.data_ptr(), v.ep_return.data_ptr()
        io.ep_count, io.ep_ring, io.ring_cap = v.ep_count.data_ptr(), v.ep_ring.data_ptr(), v.ring_cap
        io.step_counter, io.err = self.step_dev.data_ptr(), self.err.data_ptr()
        io.mode, io.slot, io.bounds, io.v = self.mode.data_ptr(), self.slot.data_ptr(), self.bounds.data_ptr(), self.v.data_ptr()
        io.ou_x, io.ou_x0 = self.ou_x.data_ptr(), self.ou_x0.data_ptr()
        io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = self.ring.pointers()
        io.out_action = self.out_action.data_ptr()
        io.horizon, io.capacity = v.horizon, self.capacity
        if self.ou:
            io.ou_theta, io.ou_mu, io.ou_dt = float(proc.theta), float(proc.mu), float(proc.dt)
        io.env_kind = self.kind
        return io

    def act(self):
        """dra_dpg_env_act on the current stream (after prepare())."""
        io = self.act_io()
        lib.dra_dpg_env_act(ctypes.byref(self.update.online), ctypes.byref(io), stream_ptr())
        self.launches += 1

    def prepare(self):
        """The step's draws in the reference's order, the feed's bookkeeping, the staged block.  -> whether the step updates."""
        agent = self.agent
        cfg, rp, proc, space = agent.config, self.replay, agent.random_process, self.vec.action_space
        if agent.total_steps < cfg.warm_up:
            mode, v = MODE_WARMUP, space.sample()
        elif self.ou:       # OrnsteinUhlenbeckProcess.sample's diffusion term; the drift and x are the kernel's
            mode, v = MODE_OU, proc.std() * np.sqrt(proc.dt) * np.random.randn(*proc.size)
        else:
            mode, v = MODE_GAUSS, proc.sample()
        slot = int(rp.pos)
        rp.advance(1)
        self.ring_log.begin(1)
        agent.total_steps += 1
        learn = bool(agent.warm())
        idx = rp.draw_indices() if learn else None
        raw = self._up.stage().numpy()
        head = raw[:16].view(np.int64)
        head[0], head[1] = mode, slot
        raw[16:32].view(np.float64)[...] = (self.update.low, self.update.high)
        raw[self._o_v:self._o_idx].view(np.float64)[...] = v
        if idx is not None:
            raw[self._o_idx:].view(np.int64)[...] = idx
        self._up.send()
        self.last_draws = (mode, np.array(v, dtype=np.float64, copy=True), slot, idx)
        return learn

    def step(self):
        agent = self.agent
        learn = self.prepare()
        self.act()
        if learn:
            self.static = g = self.replay.gather(self.idx, want_f32=True, out=self.static)
            self.update.learn(g['state'], g['action'].view(self.batch, -1), g['reward_f32'], g['next_state'], g['mask_f32'],
                              policy_step=agent._policy_step())
        self.ring_log.end()

    # -- what the host reads back where it synchronises anyway ----------------------------------------------------------
    def check(self):
        """Raises when the kernel clamped a staged slot (a host bookkeeping error: the run's results are not the reference's)."""
        n = int(self.err.item())
        if n:
            raise DraError("dpg_env: %d staged ring slots were outside the ring and have been clamped" % n)

    def drain(self):
        self.check()
        return self.ring_log.drain()

    def episodes(self):
        self.check()
        return self.ring_log.episodes()
