"""Host side of csrc/dqn_mlp.hip: dqn_feature (examples.py:11-52) over ONE device-resident cart-pole environment and the HBM
replay ring.

`shape(network)` is q_mlp's (VanillaNet over a two-layer FCBody of one width with a relu or tanh gate and a plain biased
fc_head); `why_not(agent)` names the first condition that keeps a DQNAgent on its host path; `Step(agent, shape)` is the agent
step without a host round trip (DQN_agent.py:101-138): the host makes the draws in the reference's order
(support.plan_actor_epsilon_greedy, then UniformReplay.advance / draw_indices) and stages them in ONE block at fixed addresses,
dra_dqn_mlp_act runs the sgd_update_frequency transitions and appends them to the ring, dra_dqn_mlp_update gathers the minibatch
and writes the gradient into the optimiser's flat buffer (config.fused_dqn_update False: ring.gather and the modules on the
same indices), then the fused clip + optimizer step -- after WARMUP eager steps replayed from captured graphs (graphs.Region:
acting alone while total_steps <= exploration_steps, acting + update + clip / step afterwards; single streams, no parallel
branches).  The target copy runs eagerly between replays.  With config.fused_eval, `Step.evaluate(n)` runs n greedy episodes of
config.eval_env -- moved onto the device on first use -- as ONE launch of the kind's evaluation kernel (csrc/eval_act.h) and one
copy back; an evaluation environment that cannot move stays on the host (EVAL_HOST_NOTE).  There is no CPU / eager-PyTorch implementation here: without the HIP
library every call raises.
"""
import ctypes

import numpy as np
import torch

from ._lib import DraError, lib, stream_ptr
from .device_env import DeviceCartPoleVec, _RolloutVec
from .graphs import Region, _fused_noisy
from .mlp_rollout import fill_net, shape_table, target_why_not, unowned
from .q_mlp import Net, _fields, shape      # noqa: F401  (the net struct is dra_q_mlp_net as it is)
from .support import Config, StagedUpload, plan_actor_epsilon_greedy

SWITCH = 'fused_dqn_feature'
NETWORK = "VanillaNet over a two-layer relu / tanh FCBody with a plain head"
MAX_K, MAX_B = 8, 256


class ActIO(ctypes.Structure):
    """Mirror of dra_dqn_mlp_act_io (include/deeprl_amd.h)."""
    _fields_ = [("env_state", ctypes.c_void_p), ("env_counter", ctypes.c_void_p), ("ep_steps", ctypes.c_void_p),
                ("ep_return", ctypes.c_void_p), ("env_seed", ctypes.c_void_p), ("step_counter", ctypes.c_void_p),
                ("ep_count", ctypes.c_void_p), ("ep_ring", ctypes.c_void_p),
                ("explore", ctypes.c_void_p), ("random_action", ctypes.c_void_p), ("slot0", ctypes.c_void_p),
                ("ring_frames", ctypes.c_void_p), ("ring_actions", ctypes.c_void_p), ("ring_rewards", ctypes.c_void_p),
                ("ring_masks", ctypes.c_void_p), ("out_q", ctypes.c_void_p), ("out_action", ctypes.c_void_p),
                ("err", ctypes.c_void_p),
                ("horizon", ctypes.c_int64), ("ring_cap", ctypes.c_int64), ("capacity", ctypes.c_int64),
                ("reward_coef", ctypes.c_double), ("t_len", ctypes.c_int32), ("n_env", ctypes.c_int32)]


class UpdateIO(ctypes.Structure):
    """Mirror of dra_dqn_mlp_update_io."""
    _fields_ = [("ring_frames", ctypes.c_void_p), ("ring_actions", ctypes.c_void_p), ("ring_rewards", ctypes.c_void_p),
                ("ring_masks", ctypes.c_void_p), ("idx", ctypes.c_void_p), ("grad", ctypes.c_void_p),
                ("out_q_target", ctypes.c_void_p), ("out_td", ctypes.c_void_p), ("out_loss", ctypes.c_void_p),
                ("err", ctypes.c_void_p), ("capacity", ctypes.c_int64), ("discount", ctypes.c_double),
                ("batch", ctypes.c_int32), ("double_q", ctypes.c_int32)]


class EvalIO(ctypes.Structure):
    """Mirror of dra_mlp_eval_io: the evaluation launch of all three kinds (dqn_mlp, dist_mlp, rainbow_mlp)."""
    _fields_ = [("env_state", ctypes.c_void_p), ("env_counter", ctypes.c_void_p), ("ep_steps", ctypes.c_void_p),
                ("ep_return", ctypes.c_void_p), ("env_seed", ctypes.c_void_p), ("out_return", ctypes.c_void_p),
                ("out_length", ctypes.c_void_p), ("out_steps", ctypes.c_void_p), ("out_q", ctypes.c_void_p),
                ("horizon", ctypes.c_int64), ("n_episodes", ctypes.c_int32), ("reserved", ctypes.c_int32)]


EVAL_SWITCH = 'fused_eval'
EVAL_HOST_NOTE = 'fused_eval is on but the evaluation environment stays on the host and this agent keeps the host evaluation: %s'
eval_supported = shape_table('dra_mlp_eval_supported')      # (n_episodes, horizon)

supported = shape_table('dra_dqn_mlp_supported')      # (state_dim, n_actions, hidden, t_len = transitions per launch, gate)
update_supported = shape_table('dra_dqn_mlp_update_supported')        # (state_dim, n_actions, hidden, batch, gate)


class Kind:
    """What tells this entry's device path from its siblings over the same Step (dist_mlp.py: the distributional heads): the
    switches, the agent classes, the network's shape and fields, the two kernels' shape tables.  `shape(network)` -> a tuple that
    starts (state_dim, n_actions, hidden, gate); its first N_SUPPORTED fields are what the `*_supported` tables read."""
    ENTRY, SWITCH, UPDATE_SWITCH = 'dqn_feature', SWITCH, 'fused_dqn_update'
    AGENTS, NOT_AGENT = ('DQNAgent',), "the agent is a %s, not a plain DQNAgent"
    NETWORK, ACT, UPDATE, N_SUPPORTED = NETWORK, 'dra_dqn_mlp_act', 'dra_dqn_mlp_update', 4
    EVAL = 'dra_dqn_mlp_eval'      # config.fused_eval: eval_episodes greedy episodes in one launch (Step.evaluate)
    ASYNC_ACTOR = False      # whether config.async_actor may be on (the Step runs in the sync path's order)
    # what a kind's kernels take beyond dqn_feature's own configuration (rainbow_mlp.py: all three)
    PRIORITIZED = False      # the replay is a PrioritizedReplay (else: a UniformReplay)
    MAX_N_STEP = 1           # the longest n-step window the update kernel folds
    NOISY = False            # config.noisy_linear is on, the layers on csrc/noisy.hip (else: off)
    Net, DIMS = Net, ("state_dim", "n_actions", "hidden", "gate")      # the net struct and its fields that hold shape(network)
    shape, fields = staticmethod(shape), staticmethod(_fields)
    supported, update_supported = staticmethod(supported), staticmethod(update_supported)

    @staticmethod
    def extra(agent, shp):
        """A reason of the kind's own behind the shape checks, or None."""
        return None

    @staticmethod
    def eval_net(agent, net):
        """What a kind changes in Step.net_struct()'s struct for the evaluation launch (rainbow_mlp.py: the noise it runs under)."""
        return net

    @classmethod
    def fused_update(cls, cfg, shp):
        """Whether the update runs on the kind's update kernel (else: ring.gather and the modules on the same indices)."""
        return getattr(cfg, cls.UPDATE_SWITCH, True) is not False


def _plain_optimizer(opt):
    """One parameter group under torch's RMSprop or Adam without momentum, weight decay, amsgrad or maximize."""
    if len(opt.param_groups) != 1:
        return False
    g = opt.param_groups[0]
    if g.get('weight_decay', 0) != 0 or g.get('maximize', False):
        return False
    if isinstance(opt, torch.optim.RMSprop):
        return g.get('momentum', 0) == 0
    return type(opt) is torch.optim.Adam and not g.get('amsgrad', False)


def _fresh_cartpole(agent):
    """The one envs.CartPole of the actor's Task when nobody has stepped it, else None and the reason."""
    from .envs import CartPole
    task = getattr(agent.actor, '_task', None)
    envs = _RolloutVec._host_envs(task, agent.config)
    if envs is None or len(envs) != 1 or type(envs[0]) is not CartPole:
        return None, "the task is not one envs.CartPole environment, or there is no device"
    env = envs[0]
    if agent.actor._state is not None or env.c != 0 or env.steps != 0 or isinstance(env.s, str):
        return None, "the environment has already been stepped on the host"
    return env, None


def why_not(agent, supported_fn=None, update_supported_fn=None, kind=Kind):
    """None when DQNAgent may run `agent` on the kernels of `kind`, else the first reason it may not."""
    from .normalizers import RescaleNormalizer
    from .replay import PrioritizedReplay, UniformReplay
    cfg = agent.config
    supported_fn, update_supported_fn = supported_fn or kind.supported, update_supported_fn or kind.update_supported
    shape, _fields, NETWORK = kind.shape, kind.fields, kind.NETWORK
    if getattr(cfg, kind.SWITCH, False) is not True:
        return "config.%s is not on" % kind.SWITCH
    if type(agent).__name__ not in kind.AGENTS:
        return kind.NOT_AGENT % type(agent).__name__
    rp = agent._inner_replay()
    if kind.PRIORITIZED:
        if type(rp) is not PrioritizedReplay:
            return "the replay is not a PrioritizedReplay"
        if rp.ordered_updates:
            return "the replay has ordered_updates forced"
    elif isinstance(rp, PrioritizedReplay):
        return "the replay is a PrioritizedReplay"
    elif type(rp) is not UniformReplay:
        return "the replay is not a UniformReplay"
    if kind.MAX_N_STEP == 1:
        if int(rp.n_step) != 1 or int(getattr(cfg, 'n_step', 1)) != 1:
            return "n_step is not 1"
    elif int(rp.n_step) != int(getattr(cfg, 'n_step', 1)) or not 1 <= int(rp.n_step) <= kind.MAX_N_STEP:
        return "n_step is not between 1 and %d, or the replay's is not the configuration's" % kind.MAX_N_STEP
    if int(rp.history_length) != 1 or int(getattr(cfg, 'history_length', None) or 1) != 1:
        return "history_length is not 1"
    if kind.NOISY:
        if not cfg.noisy_linear:
            return "noisy_linear is off"
        if not _fused_noisy(cfg, agent.network):
            return "the noisy layers are not on csrc/noisy.hip (config.fused_noisy)"
    elif cfg.noisy_linear:
        return "noisy_linear is on"
    if cfg.async_actor and not kind.ASYNC_ACTOR:
        return "async_actor is on"
    shp = shape(agent.network)
    if shp is None:
        return "the network is not %s" % NETWORK
    if getattr(agent, '_fused', None) is None or getattr(agent, '_target_flat', None) is None or not _plain_optimizer(agent.optimizer):
        return "the optimizer is not one plain RMSprop or Adam over every parameter"
    why = unowned(agent, _fields)
    if why is not None:
        return why
    if getattr(agent, 'grad_hook', None) is not None:
        return "a grad_hook is installed"
    dp = getattr(agent, 'dp', None)
    if dp is not None and dp.active:
        return "the agent is data parallel"
    why = target_why_not(agent, shape, _fields, shp, "the target network is not %s of the online network's shape" % NETWORK)
    if why is not None:
        return why
    rn, sn = cfg.reward_normalizer, cfg.state_normalizer
    if type(rn) is not RescaleNormalizer or rn.coef != 1.0:
        return "the reward normaliser is not RescaleNormalizer(1.0)"
    if type(sn) is not RescaleNormalizer or sn.coef != 1.0:
        return "the state normaliser is not RescaleNormalizer(1.0)"
    why = kind.extra(agent, shp)
    if why is not None:
        return why
    k, b = int(cfg.sgd_update_frequency), int(rp.batch_size)
    if not supported_fn(shp[0], shp[1], shp[2], k, *shp[3:kind.N_SUPPORTED]):
        return "%s is not built for state_dim %d, %d actions, hidden %d, %d transitions per step" % (kind.ACT, shp[0], shp[1], shp[2], k)
    if k > int(rp.memory_size) or int(rp.memory_size) < 2:
        return "the replay holds fewer slots than an agent step feeds"
    if kind.fused_update(cfg, shp) and not update_supported_fn(shp[0], shp[1], shp[2], b, *shp[3:kind.N_SUPPORTED]):
        return "%s is not built for minibatches of %d" % (kind.UPDATE, b)
    return _fresh_cartpole(agent)[1]


def adopt(agent, step_cls=None):
    """A Step (or `step_cls`, a subclass with its own KIND) with the actor's environment on the device when configuration, agent
    and task allow it; else None (the host path; with the switch on the reason is logged once)."""
    step_cls = step_cls or Step
    kind = step_cls.KIND
    why = why_not(agent, kind=kind)
    if why is not None:
        if getattr(agent.config, kind.SWITCH, False) is True:
            getattr(agent.logger, 'warning', agent.logger.info)(DeviceCartPoleVec.HOST_NOTE % why)
        return None
    return step_cls(agent, kind.shape(agent.network))


class Step:
    """One DQNAgent step on the kernels: see the module's docstring.  `regions`: the two captured regions by name."""
    WARMUP = 2
    KIND = Kind

    def __init__(self, agent, shp):
        from .device_env import EpisodeRing
        cfg = agent.config
        dev = Config.DEVICE
        self.agent, self.shape = agent, shp
        self.k, self.batch = int(cfg.sgd_update_frequency), int(agent._inner_replay().batch_size)
        self.launches = 0
        # the environment moves as reset() leaves it (DQN_agent.py:24-25: the actor's first transition resets it)
        task = agent.actor._task
        task.reset()
        self.vec = DeviceCartPoleVec(task, buffers=lambda t_len, n, f: {})
        agent.actor._task = self.vec
        agent.task = self.vec           # (device_env.EpisodeRing reads the episodes through agent.task)
        self.episodes = EpisodeRing(agent, 0, 1)
        rp = agent._inner_replay()
        self.ring = rp.device_ring((4,), np.float64, np.int64)
        if self.ring.frame_bytes != 32 or self.ring.action_bytes != 8:
            raise DraError("dqn_mlp: the replay ring holds frames of %d and actions of %d bytes" % (self.ring.frame_bytes, self.ring.action_bytes))
        self.capacity = int(rp.memory_size)
        # ONE staged block at fixed addresses: int64 first slot | int64 indices [B] | int64 random actions [K] | uint8 flags [K]
        k, b = self.k, self.batch
        self._o_idx, self._o_rand, self._o_flag = 8, 8 + 8 * b, 8 + 8 * b + 8 * k
        self._o_tail = self._o_flag + (k + 7) // 8 * 8
        self._up = StagedUpload(self._o_tail + self.staged_tail(), torch.uint8, dev)
        d = self._up.dev
        self.slot0 = d[:8].view(torch.int64)
        self.idx = d[self._o_idx:self._o_rand].view(torch.int64)
        self.random_action = d[self._o_rand:self._o_flag].view(torch.int64)
        self.explore = d[self._o_flag:self._o_flag + k]
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)      # the kernel's own step counter (the ring rows' stamp)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)           # staged words a kernel found out of range
        self.out_q = torch.zeros((k, 2), dtype=torch.float32, device=dev)
        self.out_action = torch.zeros(k, dtype=torch.int64, device=dev)
        self.make_outputs(dev)
        self.static = None              # the module-path update's minibatch buffers (ring.gather refills them in place)
        self.regions = dict(act=Region("the %s acting launch" % self.KIND.ENTRY, cfg, self.WARMUP),
                            learn=Region("the %s agent step" % self.KIND.ENTRY, cfg, self.WARMUP, opts=(agent._fused,)))
        self.last_draws = None          # (explore, random_action, first slot, indices or None) of the last step, as drawn
        # config.fused_eval: the evaluation environment on the device (None: not decided yet, False: it stays on the host)
        self._eval_vec, self._eval_bufs = None, {}
        self.eval_launches = self.eval_copies = self.eval_steps = 0
        self.eval_lengths, self.eval_debug_q, self.eval_q = None, False, None

    def staged_tail(self):
        """Bytes a kind stages behind the parent's block, from self._o_tail on (rainbow_mlp.py: the probabilities and beta)."""
        return 0

    def make_outputs(self, dev):
        """The update kernel's output buffers (a subclass has its own)."""
        b = self.batch
        self.q_target = torch.zeros(b, dtype=torch.float32, device=dev)
        self.td = torch.zeros(b, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)

    # -- the structs ---------------------------------------------------------------------------------------------------
    def net_struct(self):
        a, kind = self.agent, self.KIND
        return fill_net(kind.Net(), a._fused.flat, kind.fields(a.network), kind.DIMS, self.shape, a._target_flat)

    def act_io(self):
        """dra_dqn_mlp_act_io over the environment, the staged draws and the ring."""
        v, io = self.vec, ActIO()
        io.env_state, io.env_counter, io.env_seed = v.env_state.data_ptr(), v.env_counter.data_ptr(), v.env_seed.data_ptr()
        io.ep_steps, io.ep_return = v.ep_steps.data_ptr(), v.ep_return.data_ptr()
        io.ep_count, io.ep_ring, io.ring_cap = v.ep_count.data_ptr(), v.ep_ring.data_ptr(), v.ring_cap
        io.step_counter, io.err = self.step_dev.data_ptr(), self.err.data_ptr()
        io.explore, io.random_action, io.slot0 = self.explore.data_ptr(), self.random_action.data_ptr(), self.slot0.data_ptr()
        io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = self.ring.pointers()
        io.out_q, io.out_action = self.out_q.data_ptr(), self.out_action.data_ptr()
        io.horizon, io.capacity, io.reward_coef = v.horizon, self.capacity, float(self.agent.config.reward_normalizer.coef)
        io.t_len, io.n_env = self.k, 1
        return io

    def act(self):
        """The kind's acting kernel (dra_dqn_mlp_act) on the current stream (after prepare())."""
        net, io = self.net_struct(), self.act_io()
        getattr(lib, self.KIND.ACT)(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        self.launches += 1

    def launch_update(self, io):
        """The kind's update kernel on the staged indices over `io`, an update io struct with its outputs set: the ring, the
        indices, the optimiser's flat gradient buffer and the scalars are filled here.  -> self.loss"""
        cfg = self.agent.config
        io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = self.ring.pointers()
        io.idx, io.grad = self.idx.data_ptr(), self.agent._fused.flat.grad.data_ptr()
        io.err, io.capacity = self.err.data_ptr(), self.capacity
        io.discount, io.batch, io.double_q = float(cfg.discount) ** int(cfg.n_step), self.batch, int(bool(cfg.double_q))
        net = self.net_struct()
        getattr(lib, self.KIND.UPDATE)(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        return self.loss

    def update(self):
        """dra_dqn_mlp_update on the staged indices: the gradient lands in the optimiser's flat gradient buffer."""
        io = UpdateIO()
        io.out_q_target, io.out_td, io.out_loss = self.q_target.data_ptr(), self.td.data_ptr(), self.loss.data_ptr()
        return self.launch_update(io)

    def module_update(self):
        """The kind's update switch False: ring.gather on the staged indices, then the agent's own _loss_grad (the modules'
        forwards, the TD kernel -- ops.c51_loss / ops.qr_loss for dist_mlp's kinds --, autograd)."""
        agent = self.agent
        rp = agent._inner_replay()
        self.static = g = rp.gather(self.idx, out=self.static)
        tr = rp.TransitionCLS(state=g['state'], action=g['action'], reward=g['reward'], next_state=g['next_state'], mask=g['mask'])
        out, (net_out, grad) = agent._loss_grad(tr, None)
        agent._fused.zero_grad()
        agent._backward(net_out, grad)
        return out['loss']

    # -- one agent step ------------------------------------------------------------------------------------------------
    def prepare(self):
        """The step's draws in the reference's order -- per transition the epsilon of DQN_agent.py:34-39 and epsilon_greedy's
        two draws, then the feed's bookkeeping, then (total_steps > exploration_steps) the minibatch's rejection loop -- staged
        with one copy.  -> whether the step updates."""
        agent = self.agent
        cfg, actor, rp = agent.config, agent.actor, agent._inner_replay()
        k = self.k
        explore, rand = plan_actor_epsilon_greedy(cfg.random_action_prob, k, self.shape[1], actor._total_steps, cfg.exploration_steps)
        actor._total_steps += k
        slot0 = int(rp.pos)
        rp.advance(k)
        self.episodes.begin(k)
        agent.total_steps += k
        learn = agent.total_steps > cfg.exploration_steps
        idx = rp.draw_indices() if learn else None
        raw = self._up.stage().numpy()
        raw[:8].view(np.int64)[0] = slot0
        if idx is not None:
            raw[self._o_idx:self._o_rand].view(np.int64)[...] = idx
        raw[self._o_rand:self._o_flag].view(np.int64)[...] = rand
        raw[self._o_flag:self._o_flag + k] = explore
        self._up.send()
        self.last_draws = (explore, rand, slot0, idx)
        return learn

    def _learn(self):
        cfg = self.agent.config
        self.act()
        loss = self.update() if self.KIND.fused_update(cfg, self.shape) else self.module_update()
        self.agent._fused.step(cfg.gradient_clip)
        return loss

    def step(self):
        agent = self.agent
        cfg = agent.config
        learn = self.prepare()
        region, body = (self.regions['learn'], self._learn) if learn else (self.regions['act'], self.act)
        key = agent._fused.hyper_signature() if learn else None
        if region.due(key) and (region.graph is not None or region.capture(body, key)):
            out = region.replay()
        else:
            out = body()
        if learn:
            agent.last_loss = out
            self.after_learn()
        # DQN_agent.py:136-138, after the update of the step: eager, between graph replays
        if agent.total_steps / cfg.sgd_update_frequency % cfg.target_network_update_freq == 0:
            agent.sync_target()
        self.episodes.end()

    def after_learn(self):
        """What a kind runs eagerly behind the learn region of a step that updated (rainbow_mlp.py: the priorities' commit)."""

    # -- evaluation (config.fused_eval): config.eval_episodes greedy episodes of config.eval_env in ONE launch -------------
    def _eval_why_not(self, n):
        """None when config.eval_env may move onto the device for evaluations of `n` episodes, else the reason."""
        from .envs import CartPole
        task = self.agent.config.eval_env
        if task is self.vec or task is self.vec.task:
            return "the evaluation environment is the actor's task"
        envs = _RolloutVec._host_envs(task, self.agent.config)
        if envs is None or len(envs) != 1 or type(envs[0]) is not CartPole:
            return "the evaluation environment is not an envs.Task over one envs.CartPole, or there is no device"
        env = envs[0]
        if env.c != 0 or env.steps != 0 or isinstance(env.s, str):
            return "the evaluation environment has already been stepped on the host"
        if not eval_supported(n, env.horizon):
            return "%s is not built for %d episodes of at most %d steps" % (self.KIND.EVAL, n, env.horizon)
        return None

    def eval_vec(self, n=None):
        """The evaluation environment on the device (a DeviceCartPoleVec whose episode ring goes unused), or None where it stays
        on the host.  Decided on first use: an eligible config.eval_env moves as reset() leaves it and its host object retires,
        as the actor's task does in __init__; a refusal is logged in ONE warning."""
        if self._eval_vec is None:
            n = int(self.agent.config.eval_episodes if n is None else n)
            why = self._eval_why_not(n)
            if why is None:
                task = self.agent.config.eval_env
                task.reset()
                self._eval_vec = DeviceCartPoleVec(task, buffers=lambda t_len, n_env, f: {})
            else:
                getattr(self.agent.logger, 'warning', self.agent.logger.info)(EVAL_HOST_NOTE % why)
                self._eval_vec = False
        return self._eval_vec or None

    def _eval_buffers(self, n):
        """ONE device block per episode count -- fp64 returns [n] | int64 steps | int32 lengths [n] -- and its pinned host twin, so
        that what an evaluation leaves comes back in one copy."""
        if n not in self._eval_bufs:
            words = n + 1 + (n + 1) // 2
            dev = torch.zeros(words, dtype=torch.float64, device=Config.DEVICE)
            host = torch.zeros(words, dtype=torch.float64).pin_memory()
            self._eval_bufs[n] = (dev, host)
        return self._eval_bufs[n]

    def evaluate(self, n):
        """`n` greedy episodes of the device evaluation environment in ONE launch of the kind's evaluation kernel on the current
        stream (behind whatever the step queued) and ONE copy back -> the episodic returns, fp64 [n].  self.eval_lengths and
        self.eval_steps hold the episodes' lengths and their sum; with self.eval_debug_q set, self.eval_q [n * horizon][2] takes
        the action values per step on the device (rows behind eval_steps are NaN)."""
        n = int(n)
        vec = self.eval_vec(n)
        if vec is None:
            raise DraError("%s: the evaluation environment is not on the device" % self.KIND.ENTRY)
        if not eval_supported(n, vec.horizon):
            raise DraError("%s is not built for %d episodes of at most %d steps" % (self.KIND.EVAL, n, vec.horizon))
        dev, host = self._eval_buffers(n)
        io = EvalIO()
        io.env_state, io.env_counter, io.env_seed = vec.env_state.data_ptr(), vec.env_counter.data_ptr(), vec.env_seed.data_ptr()
        io.ep_steps, io.ep_return = vec.ep_steps.data_ptr(), vec.ep_return.data_ptr()
        io.out_return, io.out_steps, io.out_length = dev.data_ptr(), dev[n:].data_ptr(), dev[n + 1:].data_ptr()
        io.horizon, io.n_episodes = vec.horizon, n
        if self.eval_debug_q:
            self.eval_q = torch.full((n * vec.horizon, 2), float('nan'), dtype=torch.float32, device=Config.DEVICE)
            io.out_q = self.eval_q.data_ptr()
        net = self.KIND.eval_net(self.agent, self.net_struct())      # the ONLINE network as the host's eval_step reads it
        getattr(lib, self.KIND.EVAL)(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        self.eval_launches += 1
        host.copy_(dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        self.eval_copies += 1
        raw = host.numpy()
        self.eval_steps = int(raw[n:n + 1].view(np.int64)[0])
        self.eval_lengths = raw[n + 1:].view(np.int32)[:n].copy()
        return raw[:n].copy()

    # -- what the host reads back where it synchronises anyway ----------------------------------------------------------
    def check(self):
        """Raises when a kernel clamped a staged slot or index (a host bookkeeping error: the run's results are not the
        reference's)."""
        n = int(self.err.item())
        if n:
            raise DraError("%s: %d staged ring slots / indices were outside the ring and have been clamped" % (self.KIND.ENTRY, n))

    def drain(self):
        self.check()
        return self.episodes.drain()

    def state_dict(self):
        torch.cuda.current_stream().synchronize()
        state = dict(self.episodes.state_dict(), step=int(self.step_dev.item()))
        if self._eval_vec:              # the evaluation environment's arrays, once it lives on the device
            state['eval_env'] = self._eval_vec.state_dict()
        return state

    def load_state_dict(self, state):
        self.episodes.load_state_dict(state)
        self.step_dev.fill_(int(state['step']))
        if state.get('eval_env') is not None and getattr(self.agent.config, EVAL_SWITCH, False) is True:
            vec = self.eval_vec()
            if vec is None:
                raise DraError("%s: the checkpoint holds a device evaluation environment, this agent's stays on the host" % self.KIND.ENTRY)
            vec.load_state_dict(state['eval_env'])
