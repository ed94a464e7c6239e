"""Host side of csrc/dpg_mlp.hip: the DDPG / TD3 update (DDPG_agent.py:75-100, TD3_agent.py:72-108) and the one-row acting
forward as a few eager launches, behind the opt-in switch `config.fused_dpg_update`.

`shape(network)` says whether a network is one the kernels walk (DeterministicActorCriticNet / TD3Net, identity phi_body,
two-layer FCBody stacks of one (H1, H2) and one relu or tanh gate, plain Linear layers with biases); `why_not(agent)` adds the
agent-side conditions and names the first one that fails; `Update(agent)` owns the workspace, the Adam moments over the online
flat parameter buffer and the step counts, builds the structs and issues the launches on the current stream.  With
`config.fused_eval` on top, `Update.evaluate(n)` runs n greedy episodes of config.eval_env -- an envs.Pendulum, moved onto the device
on first use -- as the rows of ONE launch of dra_dpg_eval and one copy back; an evaluation environment that cannot move stays on
the host (EVAL_HOST_NOTE).
There is no CPU / eager implementation here: without the HIP library every call raises.
"""
import ctypes

import numpy as np
import torch

from ._lib import DraError, lib, stream_ptr
from .mlp_rollout import fc_body, head_out

_I6 = ctypes.c_int32 * 6
EVAL_SWITCH = 'fused_eval'
EVAL_HOST_NOTE = 'fused_eval is on but the evaluation environment stays on the host and this agent keeps the host evaluation: %s'


class Net(ctypes.Structure):
    """Mirror of dra_dpg_net (include/deeprl_amd.h)."""
    _fields_ = [("param", ctypes.c_void_p), ("actor", _I6), ("critic", _I6 * 2),
                ("state_dim", ctypes.c_int32), ("action_dim", ctypes.c_int32), ("h1", ctypes.c_int32), ("h2", ctypes.c_int32),
                ("gate", ctypes.c_int32), ("n_critics", ctypes.c_int32)]


class Batch(ctypes.Structure):
    """Mirror of dra_dpg_batch."""
    _fields_ = [("state", ctypes.c_void_p), ("next_state", ctypes.c_void_p), ("action", ctypes.c_void_p),
                ("reward", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("noise", ctypes.c_void_p),
                ("state_stride", ctypes.c_int64), ("next_state_stride", ctypes.c_int64), ("action_stride", ctypes.c_int64),
                ("batch", ctypes.c_int32), ("in_f64", ctypes.c_int32)]


class Step(ctypes.Structure):
    """Mirror of dra_dpg_step."""
    _fields_ = [("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("step_size", ctypes.c_float), ("inv_sqrt_bc2", ctypes.c_float),
                ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float), ("discount", ctypes.c_float),
                ("td3_noise", ctypes.c_float), ("td3_noise_clip", ctypes.c_float),
                ("action_low", ctypes.c_float), ("action_high", ctypes.c_float),
                ("noise_seed", ctypes.c_uint64), ("noise_counter", ctypes.c_int64)]


class EvalIO(ctypes.Structure):
    """Mirror of dra_dpg_eval_io."""
    _fields_ = [("env_state", ctypes.c_void_p), ("env_counter", ctypes.c_void_p), ("ep_steps", ctypes.c_void_p),
                ("ep_return", ctypes.c_void_p), ("env_seed", ctypes.c_void_p), ("out_return", ctypes.c_void_p),
                ("out_steps", ctypes.c_void_p), ("arrive", ctypes.c_void_p), ("out_state", ctypes.c_void_p),
                ("out_action", ctypes.c_void_p), ("horizon", ctypes.c_int64), ("n_episodes", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


def modules(network):
    """[(actor_body, fc_action), (critic_body, fc_critic), ...] of a DeterministicActorCriticNet / TD3Net, or None."""
    from .nets import DeterministicActorCriticNet, DummyBody, TD3Net
    if type(network) is DeterministicActorCriticNet:
        if type(network.phi_body) is not DummyBody:
            return None
        return [(network.actor_body, network.fc_action), (network.critic_body, network.fc_critic)]
    if type(network) is TD3Net:
        return [(network.actor_body, network.fc_action), (network.critic_body_1, network.fc_critic_1),
                (network.critic_body_2, network.fc_critic_2)]
    return None


def shape(network):
    """(state_dim, action_dim, h1, h2, gate code, n_critics) when `network` is a DeterministicActorCriticNet (identity phi_body)
    or a TD3Net whose actor and critic bodies are two-layer FCBody stacks of ONE (h1, h2) with ONE relu or tanh gate, plain
    Linear layers with biases; else None."""
    mods = modules(network)
    if mods is None:
        return None
    bodies = [fc_body(b) for b, _ in mods]
    if any(b is None for b in bodies):
        return None
    s_dim, h1, h2, gate = bodies[0]
    outs = [head_out(h, h2) for _, h in mods]
    a_dim = outs[0]
    if a_dim is None or any(b != (s_dim + a_dim, h1, h2, gate) for b in bodies[1:]) or any(o != 1 for o in outs[1:]):
        return None
    return s_dim, a_dim, h1, h2, gate, len(mods) - 1


def supported(batch, state_dim, action_dim, h1, h2, gate, n_critics):
    """dra_dpg_supported: the shapes the kernels are built for (host-only: no GPU needed)."""
    return lib.dra_dpg_supported.raw(int(batch), int(state_dim), int(action_dim), int(h1), int(h2), int(gate), int(n_critics)) == 0


def eval_supported(n_episodes, horizon, state_dim, action_dim, h1, h2, gate):
    """dra_dpg_eval_supported: the launches the evaluation kernel is built for (host-only: no GPU needed)."""
    if not 0 <= int(horizon) < 1 << 62 or not -(1 << 31) <= int(n_episodes) < 1 << 31:
        return False
    return lib.dra_dpg_eval_supported.raw(int(n_episodes), int(horizon), int(state_dim), int(action_dim), int(h1), int(h2), int(gate)) == 0


def _plain_adam(opt):
    if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
        return False
    g = opt.param_groups[0]
    return not (g.get('amsgrad') or g.get('weight_decay') or g.get('maximize') or g.get('capturable') or g.get('differentiable'))


def why_not(agent, supported_fn=supported):
    """None when `agent` (a DDPGAgent / TD3Agent) may take the fused path, else the reason it may not, in words."""
    cfg = agent.config
    if getattr(cfg, 'fused_dpg_update', False) is not True:
        return "config.fused_dpg_update is off"
    shp = shape(agent.network)
    if shp is None or shape(agent.target_network) != shp:
        return ("the network is not an actor S -> H1 -> H2 -> A with critics S + A -> H1 -> H2 -> 1 of plain Linear layers with "
                "biases, one relu / tanh gate and an identity phi_body")
    if not (_plain_adam(agent.network.actor_opt) and _plain_adam(agent.network.critic_opt)):
        return "both optimisers must be plain torch.optim.Adam (no amsgrad, weight decay or maximize)"
    from .replay import UniformReplay
    ring = getattr(agent.replay, 'replay', agent.replay)
    if type(ring) is not UniformReplay or ring.n_step != 1 or ring.history_length != 1:
        return "the replay is not a one-step UniformReplay"
    batch = ring.batch_size
    if batch is None or not supported_fn(batch, *shp):
        return "dra_dpg_supported refuses batch %r with (S, A, H1, H2, gate, critics) = %r" % (batch, shp)
    space = agent.task.action_space
    low, high = np.asarray(space.low, dtype=np.float64).reshape(-1), np.asarray(space.high, dtype=np.float64).reshape(-1)
    if not (np.all(low == low[0]) and np.all(high == high[0])):
        return "the action space bounds are not the same scalar in every dimension"
    return None


def eligible(agent, supported_fn=supported):
    return why_not(agent, supported_fn) is None


def net_struct(network, flat, shp):
    """dra_dpg_net over `network`'s parameters inside the FlatParams `flat`."""
    n = Net()
    n.param = flat.flat.data_ptr()
    off = flat.offset_of
    for i, (body, head) in enumerate(modules(network)):
        six = _I6(off(body.layers[0].weight), off(body.layers[0].bias), off(body.layers[1].weight), off(body.layers[1].bias),
                  off(head.weight), off(head.bias))
        if i == 0:
            n.actor = six
        else:
            n.critic[i - 1] = six
    n.state_dim, n.action_dim, n.h1, n.h2, n.gate, n.n_critics = shp
    return n


def workspace_floats(batch, shp):
    out = ctypes.c_int64(0)
    lib.dra_dpg_workspace_floats(int(batch), shp[0], shp[1], shp[2], shp[3], shp[5], ctypes.byref(out))
    return out.value


class Update:
    """The fused update and acting forward of one DDPGAgent / TD3Agent (eligible: `why_not(agent) is None`)."""

    def __init__(self, agent):
        self.agent = agent
        self.shape = shp = shape(agent.network)
        t_flat, s_flat = agent._flat_pair(agent.target_network, agent.network)
        tf, sf = agent._soft_flat[0], agent._soft_flat[1]
        self.online, self.target = net_struct(agent.network, sf, shp), net_struct(agent.target_network, tf, shp)
        self.flat, self.target_flat = s_flat, t_flat
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(s_flat), torch.zeros_like(s_flat)
        self.t_critic = self.t_actor = 0
        self.updates = 0                      # position of TD3's smoothing-noise stream
        self.launches = 0
        # seed of the smoothing-noise stream: configured, else the run's torch seed (read without consuming any generator, as
        # dist.DataParallel does for the on-policy agents' action noise)
        seed = getattr(agent.config, 'dp_noise_seed', None)
        self.noise_seed = int(seed) if seed is not None else int(torch.initial_seed()) & 0x3fffffff
        self.batch_size = getattr(agent.replay, 'replay', agent.replay).batch_size
        dev = s_flat.device
        self.workspace = torch.zeros(workspace_floats(self.batch_size, shp), dtype=torch.float32, device=dev)
        self._act_in = torch.zeros(128 * shp[0], dtype=torch.float64, device=dev)
        space = agent.task.action_space
        self.low, self.high = float(np.asarray(space.low).reshape(-1)[0]), float(np.asarray(space.high).reshape(-1)[0])
        # config.fused_eval: the evaluation environment on the device (None: not decided yet, False: it stays on the host)
        self._eval_vec, self._eval_bufs, self._eval_arrive = None, {}, None
        self.eval_launches = self.eval_copies = self.eval_steps = 0
        self.eval_debug, self.eval_state, self.eval_action = False, None, None

    # ---- structs
    def _step(self, opt, t):
        g = opt.param_groups[0]
        hp = (ctypes.c_float * 2)()
        lib.dra_adam_hyper(float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), int(t), hp)
        cfg = self.agent.config
        s = Step()
        s.exp_avg, s.exp_avg_sq = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        s.step_size, s.inv_sqrt_bc2 = hp[0], hp[1]
        s.beta1, s.beta2, s.eps = float(g['betas'][0]), float(g['betas'][1]), float(g['eps'])
        s.discount = float(cfg.discount)
        if self.shape[5] == 2:
            s.td3_noise, s.td3_noise_clip = float(cfg.td3_noise), float(cfg.td3_noise_clip)
            s.action_low, s.action_high = self.low, self.high
        s.noise_seed, s.noise_counter = self.noise_seed, self.updates
        return s

    @staticmethod
    def batch_struct(state, action, reward, next_state, mask, noise=None):
        """dra_dpg_batch over device tensors: state / next_state / action fp32 or fp64 (one dtype; rows may be strided views of
        the replay's block), reward / mask fp32 [B]."""
        b = Batch()
        f64 = state.dtype == torch.float64
        for t in (state, next_state, action):
            if t.dtype != state.dtype or t.dim() != 2 or t.stride(1) != 1 or t.dtype not in (torch.float32, torch.float64):
                raise ValueError("dpg batch: state, next_state and action are [B, n] fp32 or fp64 of one dtype, unit inner stride")
        for t in (reward, mask):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != state.shape[0]:
                raise ValueError("dpg batch: reward and mask are contiguous fp32 [B]")
        b.state, b.next_state, b.action = state.data_ptr(), next_state.data_ptr(), action.data_ptr()
        b.reward, b.mask = reward.data_ptr(), mask.data_ptr()
        b.noise = None if noise is None else noise.data_ptr()
        b.state_stride, b.next_state_stride, b.action_stride = state.stride(0), next_state.stride(0), action.stride(0)
        b.batch, b.in_f64 = state.shape[0], 1 if f64 else 0
        return b

    # ---- launches
    def learn(self, state, action, reward, next_state, mask, policy_step=True, noise=None):
        """One agent update on the current stream: critic (2 launches), then -- on a policy step -- actor (2) and the soft
        target update (1).  The tensors must stay alive until the stream has run them (the caller holds the minibatch)."""
        a, net = self.agent, self.agent.network
        b = self.batch_struct(state, action, reward, next_state, mask, noise)
        self.t_critic += 1
        st = self._step(net.critic_opt, self.t_critic)
        lib.dra_dpg_critic_update(ctypes.byref(self.online), ctypes.byref(self.target), ctypes.byref(b), ctypes.byref(st),
                                  self.workspace.data_ptr(), stream_ptr())
        self.updates += 1
        self.launches += 2
        if policy_step:
            self.t_actor += 1
            st = self._step(net.actor_opt, self.t_actor)
            lib.dra_dpg_actor_update(ctypes.byref(self.online), ctypes.byref(b), ctypes.byref(st), self.workspace.data_ptr(),
                                     stream_ptr())
            a.soft_update(a.target_network, net)
            self.launches += 3

    def act(self, state):
        """tanh(actor(state)) for [n <= 128, S] observations (numpy or tensor) -> fp32 device tensor [n, A]."""
        s_dim, a_dim = self.shape[0], self.shape[1]
        if isinstance(state, torch.Tensor):
            x = state.to(self.flat.device).reshape(-1, s_dim)
            if x.dtype not in (torch.float32, torch.float64) or x.stride(1) != 1:
                x = x.float().contiguous()
        else:
            host = np.ascontiguousarray(np.asarray(state, dtype=np.float64).reshape(-1, s_dim))
            x = self._act_in[:host.size].view(-1, s_dim)
            x.copy_(torch.from_numpy(host))
        out = torch.empty((x.shape[0], a_dim), dtype=torch.float32, device=self.flat.device)
        lib.dra_dpg_act(ctypes.byref(self.online), x.data_ptr(), x.stride(0), 1 if x.dtype == torch.float64 else 0, x.shape[0],
                        out.data_ptr(), stream_ptr())
        self.launches += 1
        return out

    # ---- evaluation (config.fused_eval): config.eval_episodes greedy episodes of config.eval_env as the rows of ONE launch
    def _eval_why_not(self, n):
        """None when config.eval_env may move onto the device for evaluations of `n` episodes, else the reason."""
        from .device_env import _RolloutVec
        from .envs import Pendulum
        from .normalizers import RescaleNormalizer
        agent = self.agent
        cfg, task = agent.config, agent.config.eval_env
        if task is agent.task or task is getattr(agent.task, 'task', None):
            return "the evaluation environment is the agent's own task"
        envs = _RolloutVec._host_envs(task, cfg)
        if envs is None or len(envs) != 1 or type(envs[0]) is not Pendulum:
            return "the evaluation environment is not an envs.Task over one envs.Pendulum, or there is no device"
        env = envs[0]
        if env.c != 0 or env.steps != 0 or isinstance(env.s, str):
            return "the evaluation environment has already been stepped on the host"
        sn, rn = cfg.state_normalizer, cfg.reward_normalizer
        if type(sn) is not RescaleNormalizer or sn.coef != 1.0:
            return "the state normaliser is not RescaleNormalizer(1.0)"
        if type(rn) is not RescaleNormalizer or rn.coef != 1.0:
            return "the reward normaliser is not RescaleNormalizer(1.0)"
        if not eval_supported(n, env.horizon, *self.shape[:5]):
            return "dra_dpg_eval is not built for %d episodes of %d steps with (S, A, H1, H2, gate) = %r" % (n, env.horizon, self.shape[:5])
        return None

    def eval_vec(self, n=None):
        """The evaluation environment on the device (a DevicePendulumVec whose episode ring goes unused), or None where it stays on
        the host.  Decided on first use: an eligible config.eval_env moves as reset() leaves it and its host object retires; a
        refusal is logged in ONE warning and the host loop stays for good."""
        if self._eval_vec is None:
            from .device_env import DevicePendulumVec
            n = int(self.agent.config.eval_episodes if n is None else n)
            why = self._eval_why_not(n)
            if why is None:
                task = self.agent.config.eval_env
                task.reset()
                self._eval_vec = DevicePendulumVec(task)
                self._eval_arrive = torch.zeros(1, dtype=torch.int32, device=self.flat.device)
            else:
                getattr(self.agent.logger, 'warning', self.agent.logger.info)(EVAL_HOST_NOTE % why)
                self._eval_vec = False
        return self._eval_vec or None

    def _eval_buffers(self, n):
        """ONE device block per episode count -- fp64 returns [n] | int64 steps -- and its pinned host twin: one copy back."""
        if n not in self._eval_bufs:
            dev = torch.zeros(n + 1, dtype=torch.float64, device=self.flat.device)
            self._eval_bufs[n] = (dev, torch.zeros(n + 1, dtype=torch.float64).pin_memory())
        return self._eval_bufs[n]

    def evaluate(self, n):
        """`n` greedy episodes of the device evaluation environment as the rows of ONE dra_dpg_eval launch on the current stream
        (behind whatever the step queued) and ONE copy back -> the episodic returns, fp64 [n]; self.eval_steps holds the steps
        walked.  With self.eval_debug set, self.eval_state [n][horizon + 1][2] (fp64) and self.eval_action [n][horizon] (fp32) take
        the trajectory on the device."""
        n = int(n)
        vec = self.eval_vec(n)
        if vec is None:
            raise DraError("dpg_mlp: the evaluation environment is not on the device")
        if not eval_supported(n, vec.horizon, *self.shape[:5]):
            raise DraError("dra_dpg_eval is not built for %d episodes of %d steps" % (n, vec.horizon))
        dev, host = self._eval_buffers(n)
        io = EvalIO()
        io.env_state, io.env_counter, io.env_seed = vec.env_state.data_ptr(), vec.env_counter.data_ptr(), vec.env_seed.data_ptr()
        io.ep_steps, io.ep_return = vec.ep_steps.data_ptr(), vec.ep_return.data_ptr()
        io.out_return, io.out_steps, io.arrive = dev.data_ptr(), dev[n:].data_ptr(), self._eval_arrive.data_ptr()
        io.horizon, io.n_episodes = vec.horizon, n
        if self.eval_debug:
            self.eval_state = torch.full((n, vec.horizon + 1, 2), float('nan'), dtype=torch.float64, device=self.flat.device)
            self.eval_action = torch.full((n, vec.horizon), float('nan'), dtype=torch.float32, device=self.flat.device)
            io.out_state, io.out_action = self.eval_state.data_ptr(), self.eval_action.data_ptr()
        lib.dra_dpg_eval(ctypes.byref(self.online), ctypes.byref(io), stream_ptr())      # the ONLINE actor, as eval_step reads it
        self.eval_launches += 1
        host.copy_(dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        self.eval_copies += 1
        raw = host.numpy()
        self.eval_steps = int(raw[n:n + 1].view(np.int64)[0])
        return raw[:n].copy()

    # ---- views for tests / logging (the head of the workspace: y, q [2], per-row loss)
    def last(self):
        n = self.batch_size
        w = self.workspace
        return dict(y=w[:n], q=w[n:3 * n].view(2, n)[:self.shape[5]], loss=w[3 * n:4 * n])
