"""Agents with the reference's `Agent(config).step()` surface and control flow, whose per-step
arithmetic runs on the HIP kernels.

Reference: deep_rl/agent/BaseAgent.py:15-182 (BaseAgent, BaseActor), DQN_agent.py:14-138,
CategoricalDQN_agent.py:14-89, QuantileRegressionDQN_agent.py:14-77, A2C_agent.py:12-64,
PPO_agent.py:12-100, NStepDQN_agent.py:12-67.

Differences that are the point of the rewrite (results unchanged):
  * actor / replay "processes" are in-process objects: the replay is an HBM ring, so the
    pickle-over-pipe hops of BaseAgent.py:142-172 / replay.py:219-278 have nothing left to hide;
    `async_replay` is accepted and has no effect; `config.async_actor` selects, for DQNAgent on the dqn_pixel
    configuration with a device-resident environment, the two-stream actor / learner pipeline of csrc/learner.hip
    (DQNAgent._attach_device_pipeline) and is otherwise a no-op;
  * TD / C51 / QR / PPO / A2C losses are single fused kernels that emit the gradient w.r.t. the
    network output, which is pushed through the HIP contractions by autograd;
  * clip_grad_norm_ + optimizer.step() are two launches over one flat buffer (optim.py);
  * GAE / n-step returns are one chunked-scan launch instead of T python iterations;
  * DQNAgent on the dqn_pixel configuration (VanillaNet(NatureConvBody), RMSprop, UniformReplay of 84x84 uint8
    frames, history 4 -- examples.py:55-97) switches to the fused learner of csrc/learner.hip: one C call per
    update (gather + forward + TD loss + backward + clip + RMSprop as a captured hipGraph; PrioritizedReplay adds
    the IS-weight / priority kernel and runs the chain eagerly) and one C call per actor forward;
    `config.fused_learner = False` keeps the generic autograd path.
"""
import pickle
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .envs import LazyFrames
from .optim import FlatParams, FusedOptimizer, nature_conv_weights
from .replay import PrioritizedTransition, Storage
from ._lib import DraError
from .device_env import DeviceAtariVec, EpisodeRing
from .pixel_rollout import _OCRollout, _PixelRollout, _QRollout, hand_over, k_major     # noqa: F401  (the rollouts: this module's names too)
from .graphs import (_capture, _capture_failed, _fused_noisy, _GraphedAct, _GraphedPPO, _GraphedQ,   # noqa: F401  (the captured regions:
                     _GraphedUpdate, _OnPolicyGraph)                                               # this module's names too)
from .support import Config, LinearSchedule, close_obj, epsilon_greedy, get_logger, random_sample, range_tensor, tensor, to_np


class _NullLock:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class BaseAgent:
    """What every agent shares with the outside world (the surface of BaseAgent.py:15-105): checkpoint files in the
    reference's format, evaluation episodes, the episodic-return log lines / scalars its plotting tools parse, task
    switching.  The file formats and log strings are interchange formats and are kept byte for byte:
      '<name>.model'  torch.save of network.state_dict() -- the reference's key names, [OC,C,KH,KW] conv weights;
      '<name>.stats'  pickle of config.state_normalizer.state_dict();
      'steps %d, episodic_return_test %.2f(%.2f)' / 'steps %d, episodic_return_train %s' (logger.py / plot.py tags)."""

    def __init__(self, config):
        self.config = config
        self.logger = get_logger(tag=config.tag, log_level=config.log_level)
        self.task_ind = 0

    def close(self):
        close_obj(self.task)

    # -- checkpoints -------------------------------------------------------------------------------------------
    def save(self, filename):
        dp = getattr(self, 'dp', None)
        if dp is not None and not dp.is_main:
            return     # data parallel: every rank holds the same parameters; rank 0 writes the one checkpoint file
        # parameters may be strided views of a flat (KOC) buffer: write plain contiguous CPU tensors, as the reference does
        weights = {k: v.detach().cpu().contiguous().clone() for k, v in self.network.state_dict().items()}
        torch.save(weights, filename + '.model')
        with open(filename + '.stats', 'wb') as f:
            pickle.dump(self.config.state_normalizer.state_dict(), f)

    def load(self, filename):
        weights = torch.load(filename + '.model', map_location='cpu')
        self.network.load_state_dict(weights)
        with open(filename + '.stats', 'rb') as f:
            self.config.state_normalizer.load_state_dict(pickle.load(f))

    # -- evaluation --------------------------------------------------------------------------------------------
    def eval_step(self, state):
        raise NotImplementedError

    def eval_episode(self):
        env = self.config.eval_env
        state = env.reset()
        ret = None
        while ret is None:
            state, _, _, info = env.step(self.eval_step(state))
            ret = info[0]['episodic_return']
        return ret

    def eval_episodes(self):
        return self._report_eval(np.asarray([np.sum(self.eval_episode()) for _ in range(self.config.eval_episodes)]))

    def _report_eval(self, returns):
        """BaseAgent.py:70-77 behind the episodes themselves: mean and standard error, the two records, the dict."""
        mean, sem = returns.mean(), returns.std() / np.sqrt(len(returns))
        self.logger.info('steps %d, episodic_return_test %.2f(%.2f)' % (self.total_steps, mean, sem))
        self.logger.add_scalar('episodic_return_test', mean, self.total_steps)
        return {'episodic_return_test': mean}

    def record_online_return(self, info, offset=0):
        """info: one env's dict or the vector env's tuple of dicts; a finished episode logs its return at
        total_steps + the env's position in the tuple."""
        if isinstance(info, tuple):
            for i, one in enumerate(info):
                self.record_online_return(one, i)
            return
        if not isinstance(info, dict):
            raise NotImplementedError
        ret = info['episodic_return']
        if ret is not None:
            self.log_train_return(ret, self.total_steps + offset)

    def log_train_return(self, ret, at):
        """The reference's two 'episodic_return_train' lines for an episode that ended at step `at`."""
        self.logger.add_scalar('episodic_return_train', ret, at)
        self.logger.info('steps %d, episodic_return_train %s' % (at, ret))

    def _account_rollout(self, infos, stride):
        """A rollout that was planned ahead (DeviceAtariVec.plan), on the host's books: per planned step the returns of the episodes
        that end there, then total_steps advances by `stride`.  -> whether config.target_network_update_freq falls on one of the
        steps (the per-step loops copy the target network there; the parameters do not change inside a rollout, so the caller
        copies once, ahead of it)."""
        freq = self.config.target_network_update_freq
        sync = False
        for info in infos:
            self.record_online_return(info)
            self.total_steps += stride
            if freq is not None and self.total_steps // stride % freq == 0:
                sync = True
        return sync

    def switch_task(self):
        """config.tasks: consecutive equal shares of max_steps per task."""
        tasks = self.config.tasks
        if not tasks:
            return
        boundary = np.linspace(0, self.config.max_steps, len(tasks) + 1)[self.task_ind + 1]
        if self.total_steps > boundary:
            self.task_ind += 1
            self.task = tasks[self.task_ind]
            self.states = self.config.state_normalizer(self.task.reset())


def _write_side(filename, suffix, state):
    """`<filename><suffix>`: the pickle of `state`, what a device path keeps next to the reference's two checkpoint files."""
    with open(filename + suffix, 'wb') as f:
        pickle.dump(state, f)


def _read_side(filename, suffix):
    """The dict _write_side left, or None where there is no such file (checkpoints of the reference itself have none)."""
    if not os.path.isfile(filename + suffix):
        return None
    with open(filename + suffix, 'rb') as f:
        return pickle.load(f)


class _DeviceEpisodes:
    """In front of BaseAgent, for the agents whose training episodes may end on the device (device_env.EpisodeRing): whatever
    reads the log -- eval_episodes, close, and save in the agents' own methods -- drains the ring first."""

    def _episode_ring(self):
        """What drains: an EpisodeRing, something with its drain() / episodes(), or None on a path without one."""
        return self._episodes

    def drain_episodes(self):
        """EpisodeRing.drain: logs the episodes that ended on the device since the last drain -> their (step, return) pairs."""
        ring = self._episode_ring()
        return ring.drain() if ring is not None else []

    def episodes(self):
        """EpisodeRing.episodes: (step, episodic return) of the training episodes that ended since the previous call."""
        ring = self._episode_ring()
        return ring.episodes() if ring is not None else []

    def eval_episodes(self):
        self.drain_episodes()
        return super().eval_episodes()

    def close(self):
        self.drain_episodes()
        super().close()


class BaseActor:
    """BaseAgent.py:108-182 without the process: `step()` returns `sgd_update_frequency`
    transitions, in the order the reference's sync path (`async_actor=False`) produces them."""
    STEP, RESET, EXIT, SPECS, NETWORK, CACHE = range(6)

    def __init__(self, config):
        self.config = config
        self._state = None
        self._task = None
        self._network = None
        self._total_steps = 0
        self._set_up()
        self._task = config.task_fn()

    def start(self):
        return None

    def _sample(self):
        transitions = []
        for _ in range(self.config.sgd_update_frequency):
            transition = self._transition()
            if transition is not None:
                transitions.append(transition)
        return transitions

    def step(self):
        return self._sample()

    def _transition(self):
        raise NotImplementedError

    def _set_up(self):
        pass

    def close(self):
        close_obj(self._task)

    def set_network(self, net):
        self._network = net


# ==================================================================================================== DQN family
class DQNActor(BaseActor):
    """DQN_agent.py:14-45."""

    def __init__(self, config):
        BaseActor.__init__(self, config)
        self.config = config
        self._fast_q = None
        self._graphed_q = _GraphedQ(self) if Config.DEVICE.type == 'cuda' else None
        self.start()

    def compute_q(self, prediction):
        return to_np(prediction['q'])

    def q_device(self, prediction):
        """The action values compute_q() brings to the host, as a device tensor (graph-captured actor forward)."""
        return prediction['q']

    def _transition(self):
        if self._state is None:
            self._state = self._task.reset()
        config = self.config
        if config.noisy_linear:
            self._network.reset_noise()
        q_values = None
        if self._fast_q is not None:     # fused learner attached (DQNAgent._attach_fused_learner)
            q_values = self._fast_q(self._state)
        elif self._graphed_q is not None and self._graphed_q.usable(self._state):
            q_values = self._graphed_q(self._state)     # None during its warm-up calls
        if q_values is None:
            with config.lock:
                with torch.no_grad():
                    prediction = self._network(config.state_normalizer(self._state))
            q_values = self.compute_q(prediction)
        if config.noisy_linear:
            epsilon = 0
        elif self._total_steps < config.exploration_steps:
            epsilon = 1
        else:
            epsilon = config.random_action_prob()
        action = epsilon_greedy(epsilon, q_values)
        next_state, reward, done, info = self._task.step(action)
        entry = [self._state, action, reward, next_state, done, info]
        self._total_steps += 1
        self._state = next_state
        return entry


class DQNAgent(_DeviceEpisodes, BaseAgent):
    """DQN_agent.py:48-138."""
    ActorCLS = DQNActor
    _feature = None     # dqn_mlp.Step on the cart-pole device path (config.fused_dqn_feature), None on every other path

    def __init__(self, config):
        BaseAgent.__init__(self, config)
        self.config = config
        config.lock = _NullLock()
        self._pre_init()
        self.replay = config.replay_fn()
        self.actor = self.ActorCLS(config)
        self.network = config.network_fn()
        self.target_network = config.network_fn()
        for net in (self.network, self.target_network):
            if hasattr(net, 'set_fused_noisy'):     # noisy layers on csrc/noisy.hip (default) or on the module path
                net.set_fused_noisy(getattr(config, 'fused_noisy', True) is not False)
        self.target_network.load_state_dict(self.network.state_dict())
        self.optimizer = config.optimizer_fn(self.network.parameters())
        self._fused = FusedOptimizer.adopt(self.optimizer)           # re-homes network params in one flat buffer
        self._target_flat = FlatParams(list(self.target_network.parameters()),
                                       koc=nature_conv_weights(list(self.target_network.parameters())))
        self.actor.set_network(self.network)
        self.total_steps = 0
        self._learner = None            # fused learner (csrc/learner.hip), attached lazily when eligible
        self._host_async = False        # host environment + config.async_actor: the two-stream schedule of _step_host_async
        self._ahead = None
        self._learner_lr = None
        self._pipe = None               # device-resident actor / environment pipeline
        self._fused_checked = False
        self._graphed = _GraphedUpdate(self)   # generic path: whole update as one graph replay (uniform replay)
        self._post_init()
        env = self._device_env()
        if env is not None:
            self._attach_device_pipeline(env)
        self._noisy_actor = self._device_noisy_actor()
        # dqn_feature, examples.py:11-52 (opt-in, config.fused_dqn_feature): the cart-pole and the replay's feed live on the device,
        # one launch per agent step's transitions and one per update (csrc/dqn_mlp.hip); dqn_mlp.Step, None on every other path
        self._feature = None
        if getattr(config, 'fused_dqn_feature', False) is True:
            from . import dqn_mlp
            self._feature = dqn_mlp.adopt(self)
        # dqn_feature with n_step > 1 and / or a PrioritizedReplay (opt-in, config.fused_dqn_replay_feature): dqn_replay_mlp.Step
        if getattr(config, 'fused_dqn_replay_feature', False) is True and self._feature is None:
            from . import dqn_replay_mlp
            self._feature = dqn_replay_mlp.adopt(self)
        # categorical_dqn_feature / quantile_regression_dqn_feature, examples.py:164-193 / 101-127 (opt-in,
        # config.fused_dist_feature): the same Step over the distributional kernels (csrc/dist_mlp.hip) for CategoricalDQNAgent and
        # QuantileRegressionDQNAgent; any other agent class keeps its path and is told why
        if getattr(config, 'fused_dist_feature', False) is True and self._feature is None:
            from . import dist_mlp
            self._feature = dist_mlp.adopt(self)
        # rainbow_feature, examples.py:231-280 (opt-in, config.fused_rainbow_feature): the same Step over csrc/rainbow_mlp.hip for a
        # CategoricalDQNAgent with noisy layers, an n-step PrioritizedReplay and double_q
        if getattr(config, 'fused_rainbow_feature', False) is True and self._feature is None:
            from . import rainbow_mlp
            self._feature = rainbow_mlp.adopt(self)

    def _device_noisy_actor(self):
        """noisy_actor.NoisyActor when `config.device_noisy_actor` is on and the agent is eligible (Rainbow over one synthetic
        Atari environment: the transitions of an agent step as one batched, sync-free block on the device), else None: the
        host-stepped actor -- an opted-in agent that does not qualify says why, once."""
        if getattr(self.config, 'device_noisy_actor', False) is not True or self._pipe is not None:
            return None
        from . import noisy_actor
        why = noisy_actor.why_not(self)
        if why is not None:
            self.logger.warning('device_noisy_actor is on but this agent keeps the host-stepped actor: %s' % why)
            return None
        return noisy_actor.NoisyActor(self, noisy_actor._env_of(self))

    # -- fused fast path ---------------------------------------------------------------------------------
    def _inner_replay(self):
        return getattr(self.replay, 'replay', self.replay)

    def _fused_head(self):
        """(head_kind, n_atoms, v_min, v_max) when this agent class / network pair is one csrc/learner.hip implements:
        DQNAgent + VanillaNet, CategoricalDQNAgent + CategoricalNet, QuantileRegressionDQNAgent + QuantileNet, all over
        NatureConvBody (examples.py:55-97, 127-158, 192-222)."""
        from . import learner as L
        from .nets import CategoricalNet, NatureConvBody, QuantileNet, VanillaNet
        cfg, net = self.config, self.network
        if type(getattr(net, 'body', None)) is not NatureConvBody or len(list(net.parameters())) != 10:
            return None
        if type(self) is DQNAgent and type(net) is VanillaNet:
            return (L.HEAD_VANILLA, 0, 0.0, 0.0)
        if type(self) is CategoricalDQNAgent and type(net) is CategoricalNet:
            return (L.HEAD_CATEGORICAL, int(cfg.categorical_n_atoms), float(cfg.categorical_v_min), float(cfg.categorical_v_max))
        if type(self) is QuantileRegressionDQNAgent and type(net) is QuantileNet:
            return (L.HEAD_QUANTILE, int(cfg.num_quantiles), 0.0, 0.0)
        return None

    def _fused_optimizer(self):
        """Keyword arguments of DQNLearner for this agent's torch optimizer (RMSprop or Adam, plain: no momentum, weight
        decay, amsgrad), or None."""
        from . import learner as L
        opt = self.optimizer
        if len(opt.param_groups) != 1:
            return None
        g = opt.param_groups[0]
        if g.get('weight_decay', 0) != 0:
            return None
        if isinstance(opt, torch.optim.RMSprop) and g.get('momentum', 0) == 0:
            return dict(lr=g['lr'], alpha=g['alpha'], eps=g['eps'], centered=bool(g['centered']), optimizer=L.OPT_RMSPROP)
        if type(opt) is torch.optim.Adam and not g.get('amsgrad', False) and not g.get('maximize', False):
            return dict(lr=g['lr'], alpha=0.0, eps=g['eps'], centered=False, optimizer=L.OPT_ADAM, betas=tuple(g['betas']))
        return None

    def _fused_eligible(self):
        """The configurations csrc/learner.hip implements: examples.py:55-97 (dqn_pixel), :127-158 (categorical_dqn_pixel),
        :192-222 (quantile_regression_dqn_pixel) with uniform replay, the first two also with PrioritizedReplay."""
        from .normalizers import ImageNormalizer
        from .replay import PrioritizedReplay, UniformReplay
        cfg = self.config
        if getattr(cfg, 'fused_learner', True) is False or cfg.noisy_linear:
            return False
        head = self._fused_head()
        if head is None or self._fused_optimizer() is None:
            return False
        net = self.network
        rp = self._inner_replay()
        if type(rp) not in (UniformReplay, PrioritizedReplay) or rp._ring is None or rp.history_length != 4:
            return False
        if head[0] == 2 and type(rp) is not UniformReplay:     # QR-DQN + PER is not a valid reference configuration
            return False
        if rp._ring.frame_bytes != 7056 or rp._ring.action_bytes != 8 or rp._state_dtype != torch.uint8:
            return False
        if type(cfg.state_normalizer) is not ImageNormalizer:
            return False
        n_out = cfg.action_dim * max(1, head[1])
        return cfg.batch_size <= 1024 and cfg.action_dim <= 64 and n_out <= 4096 and net.body.conv1.weight.shape[1] == 4

    def _make_learner(self, rp, cu_partition, **extra):
        from .learner import DQNLearner
        cfg = self.config
        head_kind, n_atoms, v_min, v_max = self._fused_head()
        o = self._fused_optimizer()
        self._learner_lr = o['lr']
        return DQNLearner(self.network, self.target_network, rp._ring, cfg.batch_size, cfg.action_dim,
                          cfg.discount ** cfg.n_step, cfg.gradient_clip or 0.0, o['lr'], o['alpha'], o['eps'],
                          centered=o['centered'], double_q=bool(cfg.double_q), u8_coef=cfg.state_normalizer.coef,
                          cu_partition=cu_partition, replay_eps=getattr(cfg, 'replay_eps', 0.01),
                          replay_alpha=getattr(cfg, 'replay_alpha', 0.5), head_kind=head_kind, n_atoms=n_atoms, v_min=v_min,
                          v_max=v_max, optimizer=o['optimizer'], betas=o.get('betas', (0.9, 0.999)), **extra)

    def _attach_fused_learner(self):
        """Host environment (a real emulator, or device_env=False): the update runs in csrc/learner.hip, observations and
        actions cross the host link.  config.async_actor (BaseAgent.py:142-162) is honoured as a two-stream schedule here too:
        the transitions of agent step t+1 (batch-1 forwards on the actor stream + CU partition, from the parameters of
        update t-1, and the emulator steps on the host) are produced while update t runs on the update stream
        (_step_host_async); async_actor=False keeps everything in order on one stream."""
        from . import ops as _ops
        rp = self._inner_replay()
        torch.cuda.synchronize()        # everything issued so far (feeds, initialisation) is on other streams
        want_async = bool(self.config.async_actor) and not hasattr(rp, 'draw')      # (PER: its draw waits for the update anyway)
        self._learner = self._make_learner(rp, cu_partition=want_async)
        self._fused = None              # its flat buffer no longer backs the parameters
        self._target_flat = None
        learner = self._learner
        self._host_async = want_async and bool(learner.variant & _ops.VAR_ACTOR_PARAMS)
        if self._host_async:
            self._ahead = None
            self.actor._fast_q = lambda state: learner.q_host_async(np.asarray(state, dtype=np.uint8)).reshape(1, -1)
        else:
            self.actor._fast_q = lambda state: learner.q_host(np.asarray(state, dtype=np.uint8)).reshape(1, -1)

    # -- device-resident environment + actor (BaseAgent.py:108-182 for async_actor) -----------
    def _device_env(self):
        """The synthetic Atari environment of this agent's actor if the whole rollout -> replay -> update loop can live on
        the device: the dqn_pixel configuration (see _fused_eligible), UniformReplay, ONE SyntheticAtari environment,
        sign / identity reward normaliser.  `config.device_env = False` keeps the environment on the host."""
        from .envs import SyntheticAtari
        from .normalizers import RescaleNormalizer, SignNormalizer
        from .replay import PrioritizedReplay, UniformReplay
        cfg = self.config
        if Config.DEVICE.type != 'cuda' or getattr(cfg, 'device_env', True) is False:
            return None
        task = getattr(self.actor, '_task', None)
        envs = getattr(getattr(task, 'env', None), 'envs', None)
        if not envs or len(envs) != 1 or type(envs[0]) is not SyntheticAtari:
            return None
        env = envs[0]
        rn = cfg.reward_normalizer
        if not (type(rn) is SignNormalizer or (type(rn) is RescaleNormalizer and rn.coef == 1.0)):
            return None
        rp = self._inner_replay()
        if type(rp) not in (UniformReplay, PrioritizedReplay) or rp.history_length != 4 or env.history != 4 or env.n_actions != cfg.action_dim:
            return None
        if env.frames is not None:        # somebody already stepped it on the host: leave it there
            return None
        rp.device_ring()                  # the ring feed() would create from the first transition
        return env if self._fused_eligible() else None

    def _attach_device_pipeline(self, env):
        """config.async_actor (BaseAgent.py:142-162) is honoured as the two-stream pipeline of csrc/learner.hip: the actor
        (forward, epsilon-greedy, environment step, replay feed) runs one agent step ahead of the learner on its own
        stream and CU partition; async_actor=False runs the same kernels in order."""
        from .learner import DeviceActorPipeline, SyntheticEpisodeStream
        from .replay import PrioritizedReplay
        cfg = self.config
        rp = self._inner_replay()
        torch.cuda.synchronize()
        async_actor = bool(cfg.async_actor)
        self._learner = self._make_learner(rp, cu_partition=async_actor, env_seed=env.seed, env_done_period=env.done_period)
        self._fused = None
        self._target_flat = None
        self._fused_checked = True
        actor = self.actor

        def epsilon():                     # DQN_agent.py:34-39, the actor's own step counter
            if actor._total_steps < cfg.exploration_steps:
                eps = 1
            else:
                eps = cfg.random_action_prob()
            actor._total_steps += 1
            return eps

        stream = SyntheticEpisodeStream(env.seed, env.counter, env.done_period, env.history)
        self._pipe = DeviceActorPipeline(self._learner, rp, stream, cfg.action_dim, cfg.sgd_update_frequency, epsilon,
                                         async_actor, actor_seed=int(np.random.randint(1 << 31)) if async_actor else None,
                                         beta_fn=getattr(cfg, 'replay_beta', None))

    def _step_device(self):
        cfg = self.config

        def account(infos):               # DQN_agent.py:103-113 for transitions that never leave the device
            for reward, done, info in infos:
                self.record_online_return((info,))
                self.total_steps += 1
            return self.total_steps > cfg.exploration_steps

        pipe = self._pipe
        if pipe.async_actor and not pipe.per:
            # the uniform two-stream pipeline names its stream in every call (learner._sp): no torch stream context -- entering and
            # leaving one is ~15 us of host time per agent step, a sixth of the device-side step
            pipe.step(account)
            if self.total_steps / cfg.sgd_update_frequency % cfg.target_network_update_freq == 0:
                self.sync_target()
            return
        with torch.cuda.stream(self._learner.stream):
            pipe.step(account)
            if self.total_steps / cfg.sgd_update_frequency % cfg.target_network_update_freq == 0:
                self.sync_target()

    def _pre_init(self):
        pass

    def _post_init(self):
        pass

    def save(self, filename):
        """The reference's two files (BaseAgent.py:24-27); on the cart-pole device path (config.fused_dqn_feature) also
        `<filename>.envs`: the environment's arrays, the episode ring and the device step counter, so that a loaded run -- together
        with the replay's own save_full / load_full -- continues bit for bit."""
        if self._learner is not None:     # updates run asynchronously on the learner's streams
            self._learner.synchronize()
        if self._feature is not None:
            self._feature.drain()
        BaseAgent.save(self, filename)
        if self._feature is not None:
            _write_side(filename, '.envs', self._feature.state_dict())

    def load(self, filename):
        if self._learner is not None:
            self._learner.synchronize()
        BaseAgent.load(self, filename)
        state = _read_side(filename, '.envs') if self._feature is not None else None
        if state is not None:
            self._feature.load_state_dict(state)
        if self._learner is not None:     # parameters changed behind the learner: actor copies are stale
            torch.cuda.synchronize()
            self._learner.invalidate_actor_copy()
        self._ahead = None                # (host-emulator async actor) transitions produced ahead acted on the old parameters

    # -- true resume (the reference's save() keeps weights + normaliser only, BaseAgent.py:24-33) ------
    def save_full(self, filename):
        """Everything a bit-exact continuation needs, next to the unchanged `.model` / `.stats` files: parameters, target
        and optimizer state in their device layout, the learner's pipeline state (actor parameter copies, blocks generated
        ahead, the pending observation), the replay ring (sharded) and its cursor / priority tree, schedules, step counters
        and every random stream (numpy global, python `random`, torch CPU / device, the async actor's own RandomState).
        40 steps + save_full + a fresh process + load_full + 20 steps == 60 uninterrupted steps, bit for bit
        (tests/test_gpu_resume.py).  Device-resident pipeline (the benchmarked dqn_pixel-family configurations) only."""
        import pickle
        import random as pyrandom
        if getattr(self, '_noisy_actor', None) is not None:
            raise NotImplementedError("save_full: the device-resident noisy actor (config.device_noisy_actor) has no full resume "
                                      "-- its episode shadow and noise staging are not checkpointed; save() / load() keep the "
                                      "weights and the normaliser")
        if self._pipe is None or self._learner is None:
            raise NotImplementedError("save_full: this agent runs a host environment / the generic update path; only the "
                                      "device-resident pipeline (config.device_env, synthetic Atari) has a full resume")
        self.save(filename)
        cfg = self.config
        sched = {}
        for name in ("random_action_prob", "replay_beta"):
            sc = getattr(cfg, name, None)
            if isinstance(sc, LinearSchedule):
                sched[name] = dict(current=sc.current, inc=sc.inc, end=sc.end)
        state = dict(learner=self._learner.resume_state(), pipe=self._pipe.state_dict(), total_steps=self.total_steps,
                     actor_total_steps=self.actor._total_steps, schedules=sched, learner_lr=self._learner_lr,
                     shape=self._resume_shape(),
                     np_random=np.random.get_state(), py_random=pyrandom.getstate(), torch_cpu=torch.get_rng_state(),
                     torch_cuda=torch.cuda.get_rng_state(Config.DEVICE), agent=type(self).__name__)
        self._inner_replay().save_full(filename, ahead=2 * self._pipe.n_env)   # the actor is one agent step ahead of the cursor
        with open(filename + '.resume', 'wb') as f:
            pickle.dump(state, f)

    def _resume_shape(self):
        cfg = self.config
        return dict(n_env=int(self._pipe.n_env), batch_size=int(cfg.batch_size), history_length=int(cfg.history_length),
                    n_step=int(cfg.n_step), sgd_update_frequency=int(cfg.sgd_update_frequency), lr=float(self._learner_lr),
                    async_actor=bool(self._pipe.async_actor), per=bool(self._pipe.per))

    def load_full(self, filename):
        """Into a freshly constructed agent of the same Config (same network / replay / pipeline shape), before its first step."""
        import pickle
        import random as pyrandom
        if getattr(self, '_noisy_actor', None) is not None:
            raise NotImplementedError("load_full: the device-resident noisy actor (config.device_noisy_actor) has no full resume")
        if self._pipe is None or self._learner is None:
            raise NotImplementedError("load_full needs the device-resident pipeline (see save_full)")
        with open(filename + '.resume', 'rb') as f:
            state = pickle.load(f)
        if state["agent"] != type(self).__name__:
            raise DraError("%s.resume was written by a %s" % (filename, state["agent"]))
        # the Config fields that shape the pipeline state being restored (pending blocks, slots written ahead, minibatch
        # buffers, the optimizer's step size): a resume under a different Config must not continue silently
        mine, theirs = self._resume_shape(), state.get("shape")
        if theirs is not None and theirs != mine:
            diff = {k: (theirs.get(k), mine.get(k)) for k in set(mine) | set(theirs) if theirs.get(k) != mine.get(k)}
            raise DraError("%s.resume was written under a different Config (checkpoint, this agent): %s" % (filename, diff))
        with open(filename + '.stats', 'rb') as f:
            self.config.state_normalizer.load_state_dict(pickle.load(f))
        self._inner_replay().load_full(filename)
        self._learner.load_resume_state(state["learner"])
        self._pipe.load_state_dict(state["pipe"])
        self.total_steps, self.actor._total_steps = state["total_steps"], state["actor_total_steps"]
        for name, st in state["schedules"].items():
            sc = getattr(self.config, name)
            sc.current, sc.inc, sc.end = st["current"], st["inc"], st["end"]
        np.random.set_state(state["np_random"])
        pyrandom.setstate(state["py_random"])
        torch.set_rng_state(state["torch_cpu"])
        torch.cuda.set_rng_state(state["torch_cuda"], Config.DEVICE)

    def sync_host(self):
        """Between two step() calls: everything issued has been accounted for on the host and python's `random` stands where the
        reference's would (with PrioritizedReplay drawn on the device the generator runs ahead of the kernels otherwise:
        replay.DeviceDraw).  save_full(), eval_episodes() and close() call it."""
        if getattr(self, '_pipe', None) is not None:
            self._pipe.sync_host()

    def _fused_eval(self):
        """The cart-pole device path's Step when config.fused_eval is on and config.eval_env lives (from the first call on) on the
        device too: evaluation is then ONE launch and one copy (dqn_mlp.Step.evaluate); None on every other path, and where the
        evaluation environment has to stay on the host (one warning says why)."""
        step = getattr(self, '_feature', None)
        if step is None or getattr(self.config, 'fused_eval', False) is not True:
            return None
        return step if step.eval_vec() is not None else None

    def eval_episode(self):
        step = self._fused_eval()
        if step is None:
            return super().eval_episode()
        return float(step.evaluate(1)[0])

    def eval_episodes(self):
        self.sync_host()
        step = self._fused_eval()
        if step is None:
            return super().eval_episodes()
        self.drain_episodes()
        return self._report_eval(np.asarray([np.sum(r) for r in step.evaluate(self.config.eval_episodes)]))

    def _episode_ring(self):
        """The cart-pole device path's Step (its drain() runs check() first); None on every other path."""
        return getattr(self, '_feature', None)

    def episodes(self):
        step = self._episode_ring()
        if step is None:
            return []
        step.check()
        return step.episodes.episodes()

    def close(self):
        self.drain_episodes()
        if getattr(self, '_learner', None) is not None:
            self.sync_host()
            self._learner.synchronize()
            self._learner.close()
            self._learner = None
        close_obj(self.replay)
        close_obj(self.actor)

    def eval_step(self, state):
        self.config.state_normalizer.set_read_only()
        state = self.config.state_normalizer(state)
        if self._learner is not None:
            self._learner.synchronize()
        with torch.no_grad():
            q = self.network(state)['q']
        action = to_np(q.argmax(-1))
        self.config.state_normalizer.unset_read_only()
        return action

    # -- reference-shaped hooks, kept for callers that use them directly -------------------------------
    def reduce_loss(self, loss):
        return ops.weighted_mean(loss.pow(2).mul(0.5).contiguous())

    def compute_loss(self, transitions):
        """DQN_agent.py:81-99: returns the TD-error vector (no autograd graph; step() uses _loss_grad)."""
        out, _ = self._loss_grad(transitions, per=None)
        return out['delta']

    @staticmethod
    def _f32(x):
        return x if (isinstance(x, torch.Tensor) and x.dtype == torch.float32) else tensor(to_np(x) if isinstance(x, torch.Tensor) else x)

    def _batch_scalars(self, transitions):
        reward = transitions.reward
        mask = transitions.mask
        reward = reward.float() if isinstance(reward, torch.Tensor) else tensor(reward)
        mask = mask.float() if isinstance(mask, torch.Tensor) else tensor(mask)
        action = transitions.action
        if not isinstance(action, torch.Tensor):
            action = torch.from_numpy(np.asarray(action, dtype=np.int64)).to(reward.device)
        elif action.dtype not in (torch.int64, torch.float32):
            action = action.long()
        return action.contiguous(), reward.contiguous(), mask.contiguous()

    def _per_args(self, transitions, beta=None):
        config = self.config
        sp = transitions.sampling_prob
        sp = sp.float() if isinstance(sp, torch.Tensor) else tensor(sp)
        return dict(sampling_prob=sp.contiguous(), beta=config.replay_beta() if beta is None else beta,
                    replay_eps=config.replay_eps, replay_alpha=config.replay_alpha)

    def _noisy_on_kernels(self):
        return bool(self.config.noisy_linear) and _fused_noisy(self.config, self.network)

    def _backward(self, net_out, grad):
        """The update's backward pass.  With noisy layers on csrc/noisy.hip every layer writes its parameter gradients straight
        into .grad (nets.direct_param_grads: the online network is differentiated once per update, so 0 + g == g) -- autograd's
        accumulation would re-read and re-write fc4's two 6.4 MB gradients with an element-wise kernel each."""
        if self._noisy_on_kernels():
            from .nets import direct_param_grads
            with direct_param_grads(True):
                net_out.backward(grad)
        else:
            net_out.backward(grad)

    def _device_priorities(self):
        """New priorities go to the tree without visiting the host (PrioritizedReplay.commit_device): the default for noisy
        agents on csrc/noisy.hip; config.device_priorities overrides (False: the host round trip of update_priorities)."""
        want = getattr(self.config, 'device_priorities', None)
        if want is None:
            want = self._noisy_on_kernels()
        return bool(want) and hasattr(self._inner_replay(), 'commit_device')

    def _loss_grad(self, transitions, per):
        """Forward passes + the fused TD kernel.  Returns (kernel outputs, (net_output, grad))."""
        config = self.config
        states = config.state_normalizer(transitions.state)
        next_states = config.state_normalizer(transitions.next_state)
        with torch.no_grad():
            q_next = self.target_network(next_states)['q']
            q_next_online = self.network(next_states)['q'] if config.double_q else None
        action, reward, mask = self._batch_scalars(transitions)
        q = self.network(states)['q']
        per = {k: v for k, v in (per or {}).items() if k != 'beta_dev'}     # (td_loss reads a device beta behind the probabilities)
        out = ops.td_loss(q.detach(), q_next, action, reward, mask, config.discount ** config.n_step,
                          q_next_online=q_next_online, **per)
        return out, (q, out['dq'])

    def _learn(self, transitions, beta=None):
        config = self.config
        is_per = isinstance(transitions, PrioritizedTransition)
        out, (net_out, grad) = self._loss_grad(transitions, self._per_args(transitions, beta) if is_per else None)
        if is_per:
            idxs = transitions.idx
            idxs = to_np(idxs.long()) if isinstance(idxs, torch.Tensor) else np.asarray(idxs, dtype=np.int64)
            if self._device_priorities():
                self._inner_replay().commit_device(idxs, out['prio'].contiguous())
            else:
                self.replay.update_priorities(zip(idxs, to_np(out['prio'])))
        self._fused.zero_grad()
        self._backward(net_out, grad)
        with config.lock:
            self._fused.step(config.gradient_clip)
        return out

    def step(self):
        if self._learner is not None and self.optimizer.param_groups[0]['lr'] != self._learner_lr:
            raise NotImplementedError("the fused DQN learner bakes the learning rate into its captured graphs; a scheduled "
                                      "lr needs config.fused_learner = False (generic path)")
        if self._pipe is not None:
            return self._step_device()
        if self._feature is not None:   # dqn_mlp.Step: the transitions, the feed and the update without a host round trip
            return self._feature.step()
        if self._noisy_actor is not None:
            return self._step_noisy_device()
        if self._learner is not None:   # ring feeds, actor forwards and updates share the learner's stream
            with torch.cuda.stream(self._learner.stream):
                if self._host_async:
                    return self._step_host_async()
                return self._step()
        self._step()
        if not self._fused_checked and self._inner_replay().size() > 0:
            self._fused_checked = True
            if self._fused_eligible():
                self._attach_fused_learner()

    def _step(self):
        config = self.config
        transitions = self.actor.step()
        for states, actions, rewards, next_states, dones, info in transitions:
            self.record_online_return(info)
            self.total_steps += 1
            self.replay.feed(dict(
                state=np.array([s[-1] if isinstance(s, LazyFrames) else s for s in states]),
                action=actions,
                reward=[config.reward_normalizer(r) for r in rewards],
                mask=1 - np.asarray(dones, dtype=np.int32),
            ))
        self._update_and_sync()

    def _step_noisy_device(self):
        """DQN_agent.py:101-138 with the transitions produced, acted on and fed on the device (noisy_actor.NoisyActor); the
        update is the generic path's."""
        for info in self._noisy_actor.step():
            self.record_online_return(info)
            self.total_steps += 1
        self._update_and_sync()

    def _update_and_sync(self):
        """DQN_agent.py:114-138: the update of an agent step and the target synchronisation."""
        config = self.config
        if self.total_steps > config.exploration_steps:
            if self._learner is not None:
                rp = self._inner_replay()
                if hasattr(rp, 'draw'):
                    # PER (DQN_agent.py:120-127): tree descent on device with host-drawn uniforms, one D2H of the
                    # indices (validity / padding stay on the host, draw for draw); the update applies the IS
                    # weights and emits the new priorities, which the tree takes without a second host round trip
                    tree_idx, prob, data_idx = rp.draw()
                    self._learner.update(data_idx, use_graph=True, sampling_prob=prob, beta=config.replay_beta())
                    rp.commit_device(tree_idx, self._learner.prio)      # replay.py:193-196, priorities stay on the device
                else:
                    # same index draws as replay.sample() (replay.py:92-103); gather + update are one graph replay
                    self._learner.update(rp.draw_indices(), use_graph=True)
            elif self._graphed.usable(self._inner_replay()) and self._graphed.run(self._inner_replay()) is not None:
                pass
            else:
                transitions = self.replay.sample()
                if config.noisy_linear:
                    self.target_network.reset_noise()
                    self.network.reset_noise()
                self._learn(transitions)
        if self.total_steps / config.sgd_update_frequency % config.target_network_update_freq == 0:
            self.sync_target()

    def _step_host_async(self):
        """DQN_agent.py:101-138 with async_actor=True over a HOST environment.  The reference's actor process produces the
        transitions of the next agent step while the learner trains (BaseAgent.py:142-162: step() returns the cached
        transitions and immediately asks for the next ones).  Here: feed the transitions produced during the previous call,
        enqueue update t (non-blocking, update stream), then produce the transitions of step t+1 -- forward passes on the
        actor stream from the parameter copy of update t-1 (csrc/learner.hip dra_dqn_learner_q_host_async), emulator steps
        on the host -- while the update runs."""
        config = self.config
        transitions = self._ahead if self._ahead is not None else self.actor.step()
        self._ahead = None
        rp = self._inner_replay()
        for states, actions, rewards, next_states, dones, info in transitions:
            self.record_online_return(info)
            self.total_steps += 1
            self.replay.feed(dict(
                state=np.array([s[-1] if isinstance(s, LazyFrames) else s for s in states]),
                action=actions,
                reward=[config.reward_normalizer(r) for r in rewards],
                mask=1 - np.asarray(dones, dtype=np.int32),
            ))
        if self.total_steps > config.exploration_steps:
            # the reference's rejection loop (replay.py:92-103) drawn in blocks: same np.random stream, same indices
            # (learner.draw_uniform_indices; tests/test_host_utils_vs_reference.py), a fifth of the host time
            from .learner import draw_uniform_indices
            idx = draw_uniform_indices(rp.size(), rp.pos, rp.batch_size, rp.history_length, rp.n_step)
            self._learner.update_async(idx, use_graph=True)
        if self.total_steps / config.sgd_update_frequency % config.target_network_update_freq == 0:
            self.sync_target()
        self._ahead = self.actor.step()          # overlaps the update just enqueued

    def sync_target(self):
        """DQN_agent.py:136-138 as one device-to-device copy of the flat parameter buffer."""
        if self._learner is not None:
            self._learner.sync_target()
            return
        ops.copy_f32(self._target_flat.flat, self._fused.flat.flat)
        for tb, b in zip(self.target_network.buffers(), self.network.buffers()):
            tb.copy_(b)
        # (a NoisyLinear forms weight_epsilon / bias_epsilon on demand: the copies are as current as the originals were)
        for tm, m in zip(self.target_network.modules(), self.network.modules()):
            if hasattr(m, '_eps_stale'):
                tm._eps_stale = m._eps_stale


class CategoricalDQNActor(DQNActor):
    """CategoricalDQN_agent.py:14-24."""

    def _set_up(self):
        self.config.atoms = tensor(self.config.atoms)

    def compute_q(self, prediction):
        return to_np((prediction['prob'] * self.config.atoms).sum(-1))

    def q_device(self, prediction):
        return (prediction['prob'] * self.config.atoms).sum(-1)


class CategoricalDQNAgent(DQNAgent):
    """CategoricalDQN_agent.py:27-89."""
    ActorCLS = CategoricalDQNActor

    def _pre_init(self):
        config = self.config
        config.atoms = np.linspace(config.categorical_v_min, config.categorical_v_max, config.categorical_n_atoms)

    def _post_init(self):
        config = self.config
        self.batch_indices = range_tensor(config.batch_size)
        self.atoms = tensor(config.atoms)
        self.delta_atom = (config.categorical_v_max - config.categorical_v_min) / float(config.categorical_n_atoms - 1)

    def eval_step(self, state):
        self.config.state_normalizer.set_read_only()
        state = self.config.state_normalizer(state)
        if self._learner is not None:
            self._learner.synchronize()
        with torch.no_grad():
            prediction = self.network(state)
        action = to_np((prediction['prob'] * self.atoms).sum(-1).argmax(-1))
        self.config.state_normalizer.unset_read_only()
        return action

    def compute_loss(self, transitions):
        return self._loss_grad(transitions, per=None)[0]['kl']

    def reduce_loss(self, loss):
        return ops.weighted_mean(loss.contiguous())

    def _loss_grad(self, transitions, per):
        config = self.config
        states = config.state_normalizer(transitions.state)
        next_states = config.state_normalizer(transitions.next_state)
        with torch.no_grad():
            logits_t = self.target_network(next_states)['logits']
            logits_o = self.network(next_states)['logits'] if config.double_q else None
        action, reward, mask = self._batch_scalars(transitions)
        logits = self.network(states)['logits']
        weights = prio_w = None
        dev_beta = per is not None and per.get('beta_dev') is not None      # (captured update: beta lives in a device word)
        if dev_beta:
            _, weights = ops.per_weights_dev(None, per['sampling_prob'], per['beta_dev'], per['replay_eps'], per['replay_alpha'])
        elif per is not None:
            _, weights = ops.per_weights(None, per['sampling_prob'], per['beta'], per['replay_eps'], per['replay_alpha'])
        out = ops.c51_loss(logits.detach().contiguous(), logits_t.contiguous(), action, reward, mask,
                           config.discount ** config.n_step, self.atoms, config.categorical_v_min,
                           config.categorical_v_max, logits_next_online=logits_o, weights=weights)
        if dev_beta:
            out['prio'], _ = ops.per_weights_dev(out['kl'], per['sampling_prob'], per['beta_dev'], per['replay_eps'],
                                                 per['replay_alpha'])
            out['weights'] = weights
        elif per is not None:
            out['prio'], _ = ops.per_weights(out['kl'], per['sampling_prob'], per['beta'], per['replay_eps'],
                                             per['replay_alpha'])
            out['weights'] = weights
        return out, (logits, out['dlogits'])


class QuantileRegressionDQNActor(DQNActor):
    """QuantileRegressionDQN_agent.py:13-20."""

    def compute_q(self, prediction):
        return to_np(prediction['quantile'].mean(-1))

    def q_device(self, prediction):
        return prediction['quantile'].mean(-1)


class QuantileRegressionDQNAgent(DQNAgent):
    """QuantileRegressionDQN_agent.py:23-77 (UniformReplay only: the PER branch mis-shapes in the
    reference)."""
    ActorCLS = QuantileRegressionDQNActor

    def _post_init(self):
        config = self.config
        self.batch_indices = range_tensor(config.batch_size)
        self.quantile_weight = 1.0 / config.num_quantiles
        self.cumulative_density = tensor((2 * np.arange(config.num_quantiles) + 1) / (2.0 * config.num_quantiles)).view(1, -1)

    def eval_step(self, state):
        self.config.state_normalizer.set_read_only()
        state = self.config.state_normalizer(state)
        if self._learner is not None:
            self._learner.synchronize()
        with torch.no_grad():
            q = self.network(state)['quantile'].mean(-1)
        action = np.argmax(to_np(q).flatten())
        self.config.state_normalizer.unset_read_only()
        return [action]

    def compute_loss(self, transitions):
        return self._loss_grad(transitions, per=None)[0]['loss_vec']

    def reduce_loss(self, loss):
        return ops.weighted_mean(loss.contiguous())

    def _loss_grad(self, transitions, per):
        if per is not None:
            raise NotImplementedError("QR-DQN with PrioritizedReplay is not a valid reference configuration")
        config = self.config
        states = config.state_normalizer(transitions.state)
        next_states = config.state_normalizer(transitions.next_state)
        with torch.no_grad():
            theta_t = self.target_network(next_states)['quantile']
        action, reward, mask = self._batch_scalars(transitions)
        theta = self.network(states)['quantile']
        out = ops.qr_loss(theta.detach().contiguous(), theta_t.contiguous(), action, reward, mask,
                          config.discount ** config.n_step)
        return out, (theta, out['dtheta'])


# ==================================================================================================== on-policy
def _rollout_scan(storage, config, bootstrap_v):
    """PPO_agent.py:51-61 / A2C_agent.py:43-53 as one dra_gae launch.  Fills storage.advantage / .ret
    with per-step [N,1] tensors (views of the [T,N,1] results)."""
    t_len = config.rollout_length
    reward = torch.stack(storage.reward[:t_len]).contiguous()
    mask = torch.stack(storage.mask[:t_len]).contiguous()
    value = torch.stack([v.detach() for v in storage.v[:t_len]] + [bootstrap_v.detach()]).contiguous()
    adv, ret = ops.gae(reward, mask, value, config.discount, config.gae_tau, config.use_gae)
    for i in range(t_len):
        storage.advantage[i] = adv[i]
        storage.ret[i] = ret[i]
    return adv, ret


def _begin_rollout(agent, n_env):
    """Announces a rollout of rollout_length + 1 no-grad forwards over n_env environments to a categorical actor-critic
    (nets.RolloutSlots: one uniform draw for the whole rollout, results written into persistent rows) -> the slots, or None
    (another network family, or a rank-invariant sampler is installed)."""
    slots = getattr(agent.network, 'rollout_slots', None)
    if slots is None or getattr(agent.network, 'sampler', None) is not None or Config.DEVICE.type != 'cuda':
        return None
    slots.begin(int(agent.config.rollout_length) + 1, int(n_env))
    return slots


def _install_sampler(agent):
    """Data-parallel agents (and config.dp_invariant_sampling) sample actions from per-step noise that is the same
    however the environments are spread over ranks (dist.DataParallel.uniforms); everything else keeps the reference's
    dist.sample() on torch's global generator."""
    dp = agent.dp
    net = agent.network
    if not dp.invariant_sampling or not hasattr(net, 'fc_action') or not hasattr(agent.task, 'action_space'):
        return
    from .envs import Discrete
    if not isinstance(agent.task.action_space, Discrete):
        from .nets import GaussianActorCriticNet
        if not isinstance(net, GaussianActorCriticNet):
            raise NotImplementedError("rank-invariant sampling is implemented for categorical and Gaussian policies")
        from . import ppo_mlp

        def gauss(mean, scale):     # mean + scale * hashed normal of (noise seed, sampler step, GLOBAL environment, dimension)
            if dp.step_dev is None:
                dp.step_dev = torch.zeros(1, dtype=torch.int64, device=mean.device)
            return ppo_mlp.gauss_sample(mean, scale, dp.noise_seed, dp.step_dev, dp.global_workers, dp.lo)
        net.sampler = gauss
        return
    # one kernel per sample; the noise stream's position is a device counter the kernel advances: graph-capturable
    net.sampler = lambda logits: dp.sample(logits.detach())


def _dp_sync_start(dp, network, *fused):
    """Data parallel: every rank starts from rank 0's parameters, module buffers and optimizer state (only gradients are
    exchanged afterwards, so equal starts stay equal)."""
    if not dp.active:
        return
    tensors = []
    for f in fused:
        tensors += [f.flat.flat, f.state1, f.state2]
    seen = {t.data_ptr() for t in tensors}
    for t in list(network.parameters()) + list(network.buffers()):
        # parameters re-homed in a flat buffer are views of it; anything else (buffers, stray parameters) goes by itself
        if not any(f.flat.flat.data_ptr() <= t.data_ptr() < f.flat.flat.data_ptr() + 4 * f.flat.flat.numel() for f in fused) \
                and t.data_ptr() not in seen:
            tensors.append(t)
            seen.add(t.data_ptr())
    dp.sync_state(*tensors)


def _dp_plan_exchange(dp, network, fused):
    """Data parallel: the gradient exchange in two segments, [fc4 + heads] -- complete as soon as fc4's backward has run -- going
    out while the convolutions are still being differentiated (dist.DataParallel.plan_split).  NatureConvBody networks only
    (6.4 of the 6.75 MB sit behind the split); anything else keeps the single exchange."""
    if not dp.active:
        return
    fc4 = getattr(getattr(network, 'phi_body', None), 'fc4', None)
    w = getattr(fc4, 'weight', None)
    if w is None or not any(p is w for p in fused.flat.params):
        return
    start = fused.flat.offset_of(w)
    dp.plan_split(fused.flat, [p for p, o in zip(fused.flat.params, fused.flat.offsets) if o >= start])


def _device_state_fn(agent):
    """How a device-resident rollout hands observations to the network.  ImageNormalizer over NatureConvBody (a2c_pixel /
    ppo_pixel, examples.py:361-381, 525-550): conv1's kernels take the uint8 frames themselves and normalise while staging --
    f32(f64(v) * coef), the normaliser's own table values, bit for bit (tests/test_gpu_kernels.py: u8 and f32 inputs agree to the
    bit) -- so the normaliser's launch per rollout step disappears and the rollout is stored, gathered and re-read as uint8 (a
    quarter of the bytes).  Anything else goes through config.state_normalizer as the reference does."""
    from .nets import Conv2d, NatureConvBody
    from .normalizers import RescaleNormalizer
    cfg = agent.config
    norm = cfg.state_normalizer
    body = getattr(agent.network, 'phi_body', None)
    conv1 = getattr(body, 'conv1', None)
    if (Config.DEVICE.type == 'cuda' and isinstance(norm, RescaleNormalizer) and type(body) is NatureConvBody
            and isinstance(conv1, Conv2d) and k_major(conv1)
            and getattr(cfg, 'device_u8_states', True)):
        conv1.u8_coef = float(norm.coef)

        def passthrough(x):
            if isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.is_cuda:
                return x
            return norm(x)
        return passthrough
    return norm


class A2CAgent(_DeviceEpisodes, BaseAgent):
    """A2C_agent.py:12-64."""

    def __init__(self, config):
        BaseAgent.__init__(self, config)
        self.config = config
        from .dist import DataParallel
        self.dp = DataParallel(config)           # shards config.num_workers over the ranks BEFORE task_fn builds the envs
        self.task = config.task_fn()
        self.network = config.network_fn()
        self.optimizer = config.optimizer_fn(self.network.parameters())
        self._fused = FusedOptimizer.adopt(self.optimizer)
        _dp_sync_start(self.dp, self.network, self._fused)
        _dp_plan_exchange(self.dp, self.network, self._fused)
        if self.dp.active:
            self.dp.set_weight(1.0 / self.dp.world)
        self.total_steps = 0
        if DeviceAtariVec.eligible(self.task, config):      # synthetic Atari emulators: the environments live on the device
            self.task = DeviceAtariVec(self.task)
        self.states = self.task.reset()
        self.grad_hook = None  # optional extra hook on the flat gradient before the optimiser step
        self._rollout_step = 0
        self._dev_graph = _OnPolicyGraph(self)
        self._dev_state = _device_state_fn(self)
        _install_sampler(self)
        self._pixel_rollout = _PixelRollout(self)
        self.network.fuse_fc4_head = bool(getattr(config, 'fuse_fc4_head', True))
        self.network.rollout_fc4_slices = bool(getattr(config, 'rollout_fc4_slices', True))
        # action noise of the device rollout: the rank-invariant stream when one is configured, else a seed of its own
        self._noise_seed = self.dp.noise_seed
        self._episodes = EpisodeRing(self, 1, self.dp.global_workers)      # (a sampler step per rollout step and the bootstrap's)
        # one launch per rollout over device-resident environments (_step_device_rollout) -- a2c_continuous, examples.py:384-404:
        # synthetic continuous-control environments under GaussianActorCriticNet over two small MLPs (csrc/a2c_mlp.hip);
        # a2c_feature, examples.py:340-358: cart-poles under CategoricalActorCriticNet over a small FCBody (csrc/cat_mlp.hip)
        from . import a2c_mlp, cat_mlp, mlp_rollout
        self._mlp_rollout = mlp_rollout.adopt(self, a2c_mlp.Rollout)
        self._cat_rollout = mlp_rollout.adopt(self, cat_mlp.Rollout)

    def close(self):
        super().close()
        self.dp.close()

    def save(self, filename):
        """The reference's two files (BaseAgent.py:24-27); on the device rollout paths also `<filename>.sampler`: seed and position
        of the counter-hash action noise (as PPOAgent.save) and, over DeviceCartPoleVec, the environments' arrays (state, counters,
        episode steps, returns, the episode ring), so that a loaded run continues bit for bit."""
        self.drain_episodes()
        BaseAgent.save(self, filename)
        if self._device_rollout() is not None and self.dp.is_main:
            state = self.dp.sampler_state()
            if self._cat_rollout is not None:
                state.update(self._episodes.state_dict())
            _write_side(filename, '.sampler', state)

    def load(self, filename):
        BaseAgent.load(self, filename)
        state = _read_side(filename, '.sampler') if self._device_rollout() is not None else None
        if state is not None:
            self.dp.load_sampler_state(state, Config.DEVICE)
            self._noise_seed = self.dp.noise_seed
            if self._cat_rollout is not None:
                self._episodes.load_state_dict(state)

    # -- a2c_feature over device-resident cart-pole environments: device_env.EpisodeRing ------------------------------------
    _cat_steps = property(lambda self: self._episodes.steps)      # (agent steps on the device path)

    def _device_rollout(self):
        return self._mlp_rollout or self._cat_rollout

    def _step_device_rollout(self):
        """step() over device_env.DeviceContinuousVec / DeviceCartPoleVec: A2C_agent.py:22-41 is ONE launch (dra_a2c_mlp_rollout /
        dra_cat_mlp_rollout: per step the forwards, the action, the environment step), then _learn_stacked on the rollout's
        buffers -- after _OnPolicyGraph.WARMUP eager rollouts both are replayed from one captured graph (a single stream, no
        parallel branches).  Nothing comes back to the host inside a step.  What differs is the rollout's own: the episodes come
        from the host's shadow of rewards / terminals ahead of the launch (a2c_mlp.Rollout.begin_step) or from the device's
        ring, drained every config.episode_drain_interval agent steps (cat_mlp.Rollout.begin_step / end_step)."""
        from .mlp_rollout import Plan
        rollout = self._device_rollout()
        t_len = int(self.config.rollout_length)
        rollout.begin_step(t_len)
        self.total_steps += t_len * self.dp.global_workers
        sig = rollout.signature()
        if sig != rollout.sig:
            self._dev_graph.graph, rollout.sig = None, sig
        self.last_loss = self._dev_graph.run(Plan(self.task.env_counter, t_len), self._rollout_learn)
        rollout.end_step()

    def _rollout_learn(self, plan):
        rollout = self._device_rollout()
        b = rollout.run(plan.t_len)
        self._rollout_step += plan.t_len
        rows = plan.t_len * self.task.num_envs
        return self._learn_stacked(b['state'].view(rows, -1), b['action'].view(rows, *rollout.ACTION_VIEW), b['v'], b['reward'], b['mask'])

    def _step_device(self):
        """step() over device-resident environments: the host lays the rollout out (counters, rewards, terminals of every
        environment: the synthetic environment is a pure function of its frame counter), uploads it with one copy, and
        everything else -- T x [observations, forward, action sample], bootstrap forward, return scan, loss, backward, clip,
        optimizer -- is enqueued without a host round trip and, after two eager rollouts, replayed as ONE captured graph."""
        config = self.config
        plan = self.task.plan(config.rollout_length, config.reward_normalizer)
        self._account_rollout(plan.infos, self.dp.global_workers)
        if self.dp.active:      # graph = [rollout + loss + backward]; the exchange and the step behind it stay eager
            out4 = self._dev_graph.run(plan, lambda pl: self._rollout_compute(pl, apply=False), tail=self._learn_apply)
        else:
            out4 = self._dev_graph.run(plan, self._rollout_compute)
        self.last_loss = out4

    def _rollout_compute(self, plan, apply=True):
        config = self.config
        t_len = config.rollout_length
        slots = _begin_rollout(self, self.task.num_envs)
        frames = self.task.states_all(plan)        # every observation of the planned rollout, one launch
        if slots is not None and self._pixel_rollout.eligible():
            self._pixel_rollout.run(frames, slots)     # three launches per rollout step (csrc/conv_v2.hip)
            self._rollout_step += t_len + 1
            n = self.task.num_envs
            if getattr(config, 'reuse_rollout_activations', True):
                # A2C_agent.py:29-64 backpropagates through the rollout's own forwards; so does this update: the conv layers of its
                # one batched forward take the rollout's stored outputs (same inputs, same parameters) instead of recomputing them
                # -- 31 us of a 315 us agent step at 16 x 5.  (The recomputed forward runs the four-wave kernel shape, the rollout
                # the eight-wave one: the two differ in fp32 summation order, parameters agree to ~1e-6 per update, not bit for bit.)
                acts = self._pixel_rollout.bufs
                hand_over(self.network.phi_body, acts, t_len, n)
                # (and fc4's output: the folded features the rollout's head launches left -- the update's fc4 + head node runs the
                # head launch alone)
                self.network._phi_pre = acts['phi'][:t_len].reshape(t_len * n, 512)
            return self._learn_stacked(frames[:t_len].reshape((t_len * n,) + tuple(frames.shape[2:])),
                                       slots.action[:t_len].reshape(-1), slots.v[:t_len + 1].unsqueeze(-1), plan.reward,
                                       plan.mask, apply=apply)
        states, actions, values = [], [], []
        with torch.no_grad():
            for t in range(t_len):
                state_t = self._dev_state(frames[t])
                prediction = self.network(state_t)
                self._rollout_step += 1
                states.append(state_t)
                actions.append(prediction['action'])
                values.append(prediction['v'])
            values.append(self.network(self._dev_state(frames[t_len]))['v'])
        if slots is not None:
            slots.end()
            if (values[-1].data_ptr() == slots.v[t_len].data_ptr() and states[-1].data_ptr() == frames[t_len - 1].data_ptr()):
                # the forwards wrote into the slots' rows and read the frames in place: the rollout IS these buffers (no stack / cat)
                n = self.task.num_envs
                return self._learn_stacked(frames[:t_len].reshape((t_len * n,) + tuple(frames.shape[2:])),
                                           slots.action[:t_len].reshape(-1), slots.v[:t_len + 1].unsqueeze(-1), plan.reward,
                                           plan.mask, apply=apply)
        return self._learn(states, actions, values, [plan.reward[t] for t in range(t_len)],
                           [plan.mask[t] for t in range(t_len)], apply=apply)

    def _learn_apply(self, out4=None):
        """The part of an update behind the backward pass: gradient exchange (data parallel: the loss is the mean over this
        rank's T x N/G rows; equal shards -> the mean of the G gradients is the gradient of the global mean loss; ONE
        all-reduce), optional hook, clip + optimizer step identically on every rank."""
        self.dp.sum_grads(self._fused.flat.grad, 1.0 / self.dp.world if self.dp.active else 1.0)
        if self.grad_hook is not None:
            self.grad_hook(self._fused.flat.grad)
        self._fused.step(self.config.gradient_clip)
        return out4

    def _learn(self, states, actions, values, rewards, masks, apply=True):
        """A2C_agent.py:43-64 on a finished rollout.  The reference keeps the autograd graph of every rollout forward and
        backpropagates through all T of them; the parameters do not change inside a rollout, so ONE forward over the T x N
        stored observations with the stored actions gives the same log-probabilities, entropies and values and ONE
        backward the same gradient (up to fp32 summation order) -- T-fold fewer backward launches and no gradient
        accumulation passes (rocprofv3, profiles/r02z9_*: 490 launches per A2C step, 86 of them `grad += ...`)."""
        # (stored actions: [N] per step for Categorical policies, [N, action_dim] for Gaussian ones -- a2c_continuous,
        # examples.py:384-404 -- so the environment axis is concatenated and the action axis kept)
        return self._learn_stacked(torch.cat(states, dim=0), torch.cat(actions, dim=0), torch.stack(values).contiguous(),
                                   torch.stack(rewards).contiguous(), torch.stack(masks).contiguous(), apply=apply)

    def _learn_stacked(self, states, actions, value, reward, mask, apply=True):
        """_learn on a rollout that is already laid out: states [T * N, ...], actions [T * N(, A)], value [T + 1, N, 1],
        reward / mask [T, N, 1]."""
        config = self.config
        adv, ret = ops.gae(reward, mask, value, config.discount, config.gae_tau, config.use_gae)
        prediction = self.network(states, actions)
        out4, (g_lp, g_ent, g_v) = ops.a2c_loss(prediction['log_pi_a'].detach(), prediction['entropy'].detach(),
                                                prediction['v'].detach(), adv.reshape(-1, 1), ret.reshape(-1, 1),
                                                config.entropy_weight, config.value_loss_weight)
        self._fused.zero_grad(direct=not self.dp.active)
        # (one batched forward: every parameter is used once -> the layers write their gradients in place, nets.direct_param_grads;
        # data parallel keeps autograd's accumulation: its post-accumulate hooks start the early gradient exchange)
        from .nets import direct_param_grads
        # (the optimizer step follows with nothing reading the gradient in between -> the conv layers' slab folds ride in its
        # norm launch; config.defer_conv_folds = False restores one fold launch per layer)
        defer = self._fused if (apply and not self.dp.active and self.grad_hook is None
                                and getattr(config, 'defer_conv_folds', True)) else None
        with direct_param_grads(not self.dp.active, defer_folds_to=defer, covers=[self._fused]):
            torch.autograd.backward([prediction['log_pi_a'], prediction['entropy'], prediction['v']], [g_lp, g_ent, g_v])
        return self._learn_apply(out4) if apply else out4

    def step(self):
        if getattr(self.task, 'on_device', False):
            if self._device_rollout() is not None:
                return self._step_device_rollout()
            return self._step_device()
        config = self.config
        states = self.states
        seen, actions, values, rewards_l, masks_l = [], [], [], [], []
        slots = _begin_rollout(self, len(states))       # the same single draw per rollout as the device path
        for _ in range(config.rollout_length):
            with torch.no_grad():
                state_t = tensor(config.state_normalizer(states))
                prediction = self.network(state_t)
            self._rollout_step += 1
            next_states, rewards, terminals, info = self.task.step(to_np(prediction['action']))
            self.record_online_return(info)
            rewards = config.reward_normalizer(rewards)
            seen.append(state_t)
            actions.append(prediction['action'])
            values.append(prediction['v'])
            rewards_l.append(tensor(rewards).unsqueeze(-1))
            masks_l.append(tensor(1 - terminals).unsqueeze(-1))
            states = next_states
            self.total_steps += self.dp.global_workers
        self.states = states
        with torch.no_grad():
            values.append(self.network(config.state_normalizer(states))['v'])
        if slots is not None:
            slots.end()
        self.last_loss = self._learn(seen, actions, values, rewards_l, masks_l)


class _TargetRolloutAgent(_DeviceEpisodes, BaseAgent):
    """What NStepDQNAgent and OptionCriticAgent share: a target network in a flat buffer of its own, over synthetic Atari
    emulators the device path of a pixel_rollout._TargetRollout, and over device-resident cart-poles the step, episode ring and
    save / load of their feature entries (each agent brings its mlp_rollout.Rollout and its _feature_learn)."""

    def _sync_target(self):
        ops.copy_f32(self._target_flat.flat, self._fused.flat.flat)

    def _adopt_device(self, rollout):
        """Moves the task to the device when `rollout` may run this agent (conv1 then takes the uint8 frames themselves) -> whether
        it did."""
        self._dev_graph = _OnPolicyGraph(self)
        self.last_rollout = None
        if not rollout.eligible():
            return False
        self._rollout = rollout
        self.task = DeviceAtariVec(self.task)
        self.network.body.conv1.u8_coef = float(self.config.state_normalizer.coef)
        return True

    def _step_device(self):
        """step() over device-resident environments: the host lays the rollout out (DeviceAtariVec.plan) and makes the rollout's
        draws in the reference's order (the rollout's prepare()); the T head forwards with their choices, the target network's
        bootstrap, the loss, the backward over the rollout's own activations, clip and optimizer step are enqueued without a host
        round trip and, after two eager rollouts, replayed as ONE captured graph (the rollout's compute()).  The target copy of
        NStepDQN_agent.py:48-50 / OptionCritic_agent.py:83-85 runs before the rollout: the parameters do not change inside one, so
        copying then gives the bootstrap copying at step t gives."""
        config = self.config
        t_len = config.rollout_length
        plan = self.task.plan(t_len, config.reward_normalizer)
        self._rollout.prepare(t_len)
        if self._account_rollout(plan.infos, config.num_workers):
            self._sync_target()
        out = self._dev_graph.run(plan, self._rollout.compute)
        self.last_loss = out['loss']
        self.last_rollout = out

    # -- the feature entries (n_step_dqn_feature, option_critic_feature) over device-resident cart-pole environments: one
    # mlp_rollout.Rollout (`_feature`, None on every other path) and device_env.EpisodeRing (`_episodes`) --------------------
    _feature = None

    def _feature_state(self):
        """What `<filename>.envs` holds besides the environments' arrays and the device step counter."""
        return {}

    def _load_feature_state(self, state):
        return

    def save(self, filename):
        """The reference's two files (BaseAgent.py:24-27); on the cart-pole device path also `<filename>.envs`: the environments'
        arrays (state, counters, episode steps, returns, the episode ring), the device step counter and what the agent carries
        from rollout to rollout (_feature_state), so that a loaded run continues bit for bit."""
        self.drain_episodes()
        BaseAgent.save(self, filename)
        if self._feature is not None:
            torch.cuda.current_stream().synchronize()
            _write_side(filename, '.envs', dict(self._episodes.state_dict(), step=int(self._feature.step_dev.item()), **self._feature_state()))

    def load(self, filename):
        BaseAgent.load(self, filename)
        state = _read_side(filename, '.envs') if self._feature is not None else None
        if state is not None:
            self._episodes.load_state_dict(state)
            self._feature.step_dev.fill_(int(state['step']))
            self._load_feature_state(state)

    _dev_steps = property(lambda self: self._episodes.steps)      # (agent steps on the device path)
    _step_host = property(lambda self: self._episodes.stamp)      # (the host's copy of the kernel's step counter)

    def _scan_returns(self, b):
        """The module paths' returns over the buffers `b` a rollout left, by the scan kernel from the target's bootstrap -> [T * N, 1]."""
        t_len, n = b['action'].shape
        value = torch.zeros((t_len + 1, n, 1), device=b['reward'].device)
        value[t_len] = b['bootstrap'].view(n, 1)
        _, rets = ops.gae(b['reward'].view(t_len, n, 1), b['mask'].view(t_len, n, 1), value, self.config.discount, 1.0, False)
        return rets.view(t_len * n, 1)

    def _step_feature(self):
        """step() over device_env.DeviceCartPoleVec: the host makes the rollout's draws in the reference's order and stages them
        (the rollout's prepare()); the rollout is ONE launch (dra_q_mlp_rollout / dra_oc_mlp_rollout), the update with its
        backward a second one (config.fused_nstep_update / fused_oc_update False: the module path on the same buffers), then the
        fused clip + optimizer step -- after _OnPolicyGraph.WARMUP eager steps all replayed from one captured graph (a single
        stream, no parallel branches).  The target copy of NStepDQN_agent.py:48-50 / OptionCritic_agent.py:83-85 runs before the
        launch when a step of this rollout reaches target_network_update_freq: the parameters do not change inside a rollout
        (_step_device)."""
        from .mlp_rollout import Plan
        config = self.config
        t_len, n = int(config.rollout_length), config.num_workers
        self._feature.prepare(t_len)
        self._episodes.begin(t_len)
        freq, sync = config.target_network_update_freq, False
        for _ in range(t_len):
            self.total_steps += n
            if freq is not None and self.total_steps // n % freq == 0:
                sync = True
        if sync:
            self._sync_target()
        self.last_loss = self._dev_graph.run(Plan(self.task.env_counter, t_len), self._feature_learn)
        self._episodes.end()


class NStepDQNAgent(_TargetRolloutAgent):
    """NStepDQN_agent.py:12-67: on-policy n-step Q-learning; returns via the scan kernel (use_gae off)."""

    def __init__(self, config):
        BaseAgent.__init__(self, config)
        self.config = config
        self.task = config.task_fn()
        self.network = config.network_fn()
        self.target_network = config.network_fn()
        self.optimizer = config.optimizer_fn(self.network.parameters())
        self._fused = FusedOptimizer.adopt(self.optimizer)
        self._target_flat = FlatParams(list(self.target_network.parameters()),
                                       koc=nature_conv_weights(list(self.target_network.parameters())))
        self._sync_target()
        self.total_steps = 0
        self.grad_hook = None
        self._rollout_step = 0
        self._q_rollout = _QRollout(self)
        self._adopt_device(self._q_rollout)     # synthetic Atari emulators + VanillaNet(NatureConvBody): the rollout lives on the device
        # n_step_dqn_feature, examples.py:408-424 (opt-in, config.fused_nstep_feature): cart-poles under VanillaNet over a small
        # FCBody live on the device, one launch per rollout and one per update (csrc/q_mlp.hip)
        self._episodes = EpisodeRing(self, 0, config.num_workers)     # (the kernel's step counter: one stamp per rollout step)
        self.states = self.task.reset()
        self._feature = self._adopt_feature()       # (the environments move as reset() left them)

    def _adopt_feature(self):
        from . import mlp_rollout, q_mlp
        return mlp_rollout.adopt(self, q_mlp.Rollout)

    def _feature_learn(self, plan):
        config = self.config
        rollout = self._feature
        b = rollout.run(plan.t_len)
        self._rollout_step += plan.t_len
        if getattr(config, 'fused_nstep_update', True) is not False:
            loss = rollout.update(b, config.discount)
        else:       # the module path on the rollout's buffers: returns by the scan kernel, one batched forward, autograd
            t_len, n = b['action'].shape
            rets = self._scan_returns(b)
            q_a = self.network(b['state'].view(t_len * n, -1))['q'].gather(1, b['action'].view(t_len * n, 1))
            diff = q_a.detach() - rets
            loss = 0.5 * diff.pow(2).mean()
            self._fused.zero_grad()
            q_a.backward(diff / (t_len * n))
        self._fused.step(config.gradient_clip)
        return loss

    def step(self):
        if self._feature is not None:
            return self._step_feature()
        if getattr(self.task, 'on_device', False):
            return self._step_device()
        config = self.config
        storage = Storage(config.rollout_length)
        states = self.states
        for _ in range(config.rollout_length):
            q = self.network(config.state_normalizer(states))['q']
            epsilon = config.random_action_prob(config.num_workers)
            actions = epsilon_greedy(epsilon, to_np(q))
            next_states, rewards, terminals, info = self.task.step(actions)
            self.record_online_return(info)
            rewards = config.reward_normalizer(rewards)
            storage.feed({'q': q, 'action': tensor(actions).unsqueeze(-1).long(),
                          'reward': tensor(rewards).unsqueeze(-1), 'mask': tensor(1 - terminals).unsqueeze(-1)})
            states = next_states
            self.total_steps += config.num_workers
            if self.total_steps // config.num_workers % config.target_network_update_freq == 0:
                self._sync_target()
        self.states = states
        storage.placeholder()
        with torch.no_grad():
            ret = self.target_network(config.state_normalizer(states))['q']
            ret = torch.max(ret, dim=1, keepdim=True)[0]
        t_len = config.rollout_length
        reward = torch.stack(storage.reward[:t_len]).contiguous()
        mask = torch.stack(storage.mask[:t_len]).contiguous()
        zeros = torch.zeros((t_len + 1,) + tuple(ret.shape), device=ret.device)
        zeros[t_len] = ret
        _, rets = ops.gae(reward, mask, zeros, config.discount, 1.0, False)
        for i in range(t_len):
            storage.ret[i] = rets[i]
        entries = storage.extract(['q', 'action', 'ret'])
        q_a = entries.q.gather(1, entries.action)
        n = q_a.numel()
        grad = (q_a.detach() - entries.ret) / n  # d/dq of 0.5 * mean((q - ret)^2)
        self._fused.zero_grad()
        q_a.backward(grad)
        self._fused.step(config.gradient_clip)


class PPOAgent(BaseAgent):
    """PPO_agent.py:12-100."""

    def __init__(self, config):
        BaseAgent.__init__(self, config)
        self.config = config
        from .dist import DataParallel
        self.dp = DataParallel(config)
        self.task = config.task_fn()
        self.network = config.network_fn()
        if config.shared_repr:
            self.opt = config.optimizer_fn(self.network.parameters())
            self._fused = FusedOptimizer.adopt(self.opt)
        else:
            self.actor_opt = config.actor_opt_fn(self.network.actor_params)
            self.critic_opt = config.critic_opt_fn(self.network.critic_params)
            actor_ids = {id(p) for p in self.network.actor_params}
            if any(id(p) in actor_ids for p in self.network.critic_params):
                # (the reference cannot run this configuration either: PPO_agent.py:89-96 calls policy_loss.backward() and then
                # value_loss.backward() on ONE forward -- with a parameterised phi_body the first call frees the shared part of the
                # graph and steps its weights in place, and the second raises inside autograd; tests/test_nets_host_logic.py)
                raise NotImplementedError("PPO with a parameterised phi_body shared by separate actor / critic optimisers: the "
                                          "reference's own update (PPO_agent.py:89-96) raises inside autograd for it; use "
                                          "shared_repr=True (one optimiser, examples.py:525-550)")
            self._fused_actor = FusedOptimizer.adopt(self.actor_opt)
            self._fused_critic = FusedOptimizer.adopt(self.critic_opt)
        _dp_sync_start(self.dp, self.network, *([self._fused] if config.shared_repr else [self._fused_actor, self._fused_critic]))
        if config.shared_repr:
            _dp_plan_exchange(self.dp, self.network, self._fused)
        self.total_steps = 0
        from .device_env import DeviceContinuousVec
        from .ppo_mlp import MlpPPO
        self.grad_hook = None
        self._mlp = MlpPPO(self)        # csrc/ppo_mlp.hip: two small tanh MLPs + two Adam optimisers as persistent kernels
        if DeviceAtariVec.eligible(self.task, config):      # synthetic Atari emulators: the environments live on the device
            self.task = DeviceAtariVec(self.task)
            self.states = None
        else:
            self.states = self.task.reset()
            self.states = config.state_normalizer(self.states)
            if DeviceContinuousVec.eligible(self.task, config) and self._mlp.usable():
                # synthetic continuous-control environments (BASELINE configs[2]): observations, counters and the observation
                # statistics move to the device; rollouts are one launch each (_step_device_mlp)
                self.task = DeviceContinuousVec(self.task, self.states, config.state_normalizer)
                self.states = None
        self._dev_graph = _OnPolicyGraph(self, optimizer_inside=False)
        self._dev_state = _device_state_fn(self)
        if config.shared_repr:
            self.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda step: 1 - step / config.max_steps)
        self._graphed = _GraphedPPO(self)
        self._rollout_graph = _GraphedAct(self)
        self._rollout_step = 0
        _install_sampler(self)
        self._pixel_rollout = _PixelRollout(self)
        self.network.fuse_fc4_head = bool(getattr(config, 'fuse_fc4_head', True))
        self.network.rollout_fc4_slices = bool(getattr(config, 'rollout_fc4_slices', True))
        # action noise of the device rollout: the rank-invariant stream when one is configured, else a seed of its own
        self._noise_seed = self.dp.noise_seed

    def close(self):
        close_obj(self.task)
        self.dp.close()

    def save(self, filename):
        """The reference's two files (BaseAgent.py:24-27) plus `<filename>.sampler`: seed and position of the counter-hash action
        noise of the device rollout, without which a restored agent would replay the noise of its first rollouts."""
        BaseAgent.save(self, filename)
        if self.dp.is_main:
            _write_side(filename, '.sampler', self.dp.sampler_state())

    def load(self, filename):
        BaseAgent.load(self, filename)
        state = _read_side(filename, '.sampler')
        if state is not None:
            self.dp.load_sampler_state(state, Config.DEVICE)
            self._noise_seed = self.dp.noise_seed

    def _step_device(self):
        """step() over device-resident environments (see A2CAgent._step_device): the rollout -- T x [observations, image
        normalisation, no-grad forward, action sample], bootstrap forward, GAE scan, advantage normalisation -- is one
        captured graph whose outputs are the rollout entries; the optimisation phase is unchanged."""
        config = self.config
        plan = self.task.plan(config.rollout_length, config.reward_normalizer)
        self._account_rollout(plan.infos, self.dp.global_workers)
        if self.dp.active:      # PPO_agent.py:66 over the GLOBAL rollout: three all-reduced scalars, outside the captured region
            from .dist import global_advantage_normalize_

            def normalise(entries):
                global_advantage_normalize_(entries.advantage)
                return entries
            entries = self._dev_graph.run(plan, lambda pl: self._rollout_compute(pl, normalise=False), tail=normalise)
        else:
            entries = self._dev_graph.run(plan, self._rollout_compute)
        if config.shared_repr:
            self.lr_scheduler.step(self.total_steps)
        self.optimize(entries)

    def _rollout_compute(self, plan, normalise=True):
        config = self.config
        t_len = config.rollout_length
        slots = _begin_rollout(self, self.task.num_envs)
        frames = self.task.states_all(plan)        # every observation of the planned rollout, one launch
        storage = Storage(t_len)
        fused = slots is not None and self._pixel_rollout.eligible()
        if fused:
            self._pixel_rollout.run(frames, slots)     # three launches per rollout step (csrc/conv_v2.hip)
            self._rollout_step += t_len + 1
        else:
            with torch.no_grad():
                for t in range(t_len):
                    state_t = self._dev_state(frames[t])
                    prediction = self.network(state_t)
                    self._rollout_step += 1
                    storage.feed(prediction)
                    storage.feed({'reward': plan.reward[t], 'mask': plan.mask[t], 'state': state_t})
                prediction = self.network(self._dev_state(frames[t_len]))
                self._rollout_step += 1
            if slots is not None:
                slots.end()
        if fused or (slots is not None and prediction['v'].data_ptr() == slots.v[t_len].data_ptr()
                     and state_t.data_ptr() == frames[t_len - 1].data_ptr()):
            # the forwards wrote into the slots' rows and read the frames in place: the rollout IS these buffers (Storage's
            # per-key torch.cat launches and the reward / mask / value stacks of the scan disappear)
            from collections import namedtuple
            rows = t_len * self.task.num_envs
            adv, ret = ops.gae(plan.reward, plan.mask, slots.v[:t_len + 1].unsqueeze(-1), config.discount, config.gae_tau,
                               config.use_gae)
            entry_cls = namedtuple('Entry', ['state', 'action', 'log_pi_a', 'ret', 'advantage'])
            entries = entry_cls(frames[:t_len].reshape((rows,) + tuple(frames.shape[2:])), slots.action[:t_len].reshape(rows),
                                slots.log_pi_a[:t_len].reshape(rows, 1), ret.reshape(rows, 1), adv.reshape(rows, 1))
        else:
            storage.feed(prediction)
            storage.placeholder()
            _rollout_scan(storage, config, prediction['v'])
            entries = storage.extract(['state', 'action', 'log_pi_a', 'ret', 'advantage'])
            entry_cls = entries.__class__
            entries = entry_cls(*[x.detach() for x in entries])
        if not normalise:
            return entries
        if self.dp.active:
            from .dist import global_advantage_normalize_
            global_advantage_normalize_(entries.advantage)
        else:
            ops.adv_normalize_(entries.advantage)
        return entries

    def _step_device_mlp(self):
        """step() over device_env.DeviceContinuousVec: PPO_agent.py:32-49 is ONE launch (dra_ppo_mlp_rollout: per step the
        normalised observation, both forwards, action = mean + softplus(std) * noise, log-probability, environment step,
        running observation statistics), then the return scan, the advantage normalisation and optimize()."""
        import ctypes
        from collections import namedtuple
        from ._lib import lib, stream_ptr
        from .ppo_mlp import RolloutIO
        config, task, dp = self.config, self.task, self.dp
        t_len, n = int(config.rollout_length), task.num_envs
        b = task.buffers(t_len)
        events = task.shadow(t_len)
        if dp.step_dev is None:
            dp.step_dev = torch.zeros(1, dtype=torch.int64, device=Config.DEVICE)
        cfg, actor, critic = self._mlp.structs()
        self._mlp.sync_counts()
        io = RolloutIO()
        task.fill_io(io, self, t_len, config.state_normalizer.read_only)
        lib.dra_ppo_mlp_rollout(ctypes.byref(cfg), ctypes.byref(actor), ctypes.byref(critic), ctypes.byref(io), stream_ptr())
        self._rollout_step += t_len + 1
        for t, i, ret in events:        # BaseAgent.record_online_return at the step the episode ended
            self.log_train_return(ret, self.total_steps + t * dp.global_workers + i)
        self.total_steps += t_len * dp.global_workers
        adv, ret = ops.gae(b['reward'], b['mask'], b['v'], config.discount, config.gae_tau, config.use_gae)
        entry_cls = namedtuple('Entry', ['state', 'action', 'log_pi_a', 'ret', 'advantage'])
        rows = t_len * n
        entries = entry_cls(b['state'].view(rows, -1), b['action'].view(rows, -1), b['log_pi_a'].view(rows, 1),
                            ret.view(rows, 1), adv.view(rows, 1))
        ops.adv_normalize_(entries.advantage)
        self.optimize(entries)

    def step(self):
        if getattr(self.task, 'on_device', False):
            from .device_env import DeviceContinuousVec
            if isinstance(self.task, DeviceContinuousVec):
                return self._step_device_mlp()
            return self._step_device()
        config = self.config
        storage = Storage(config.rollout_length)
        states = self.states
        slots = _begin_rollout(self, len(states))       # the same single draw per rollout as the device path
        for _ in range(config.rollout_length):
            prediction, state_t = self._act(states)
            self._rollout_step += 1
            next_states, rewards, terminals, info = self.task.step(to_np(prediction['action']))
            self.record_online_return(info)
            rewards = config.reward_normalizer(rewards)
            next_states = config.state_normalizer(next_states)
            storage.feed(prediction)
            storage.feed({'reward': tensor(rewards).unsqueeze(-1), 'mask': tensor(1 - terminals).unsqueeze(-1),
                          'state': state_t})
            states = next_states
            self.total_steps += self.dp.global_workers
        self.states = states
        prediction, _ = self._act(states)
        self._rollout_step += 1
        if slots is not None:
            slots.end()
        storage.feed(prediction)
        storage.placeholder()
        _rollout_scan(storage, config, prediction['v'])

        entries = storage.extract(['state', 'action', 'log_pi_a', 'ret', 'advantage'])
        entry_cls = entries.__class__
        entries = entry_cls(*[x.detach() for x in entries])
        if self.dp.active:      # PPO_agent.py:66 over the GLOBAL rollout: three scalars all-reduced
            from .dist import global_advantage_normalize_
            global_advantage_normalize_(entries.advantage)
        else:
            ops.adv_normalize_(entries.advantage)  # PPO_agent.py:66 in place

        if config.shared_repr:
            self.lr_scheduler.step(self.total_steps)
        self.optimize(entries)

    def _act(self, states):
        """The rollout's no-grad forward (PPO_agent.py:35-36, incl. the action sample) -> (prediction dict, the
        f32 device copy of `states` that PPO_agent.py:41 stores): replayed from a captured hipGraph over a static input
        buffer (graphs._GraphedAct) once that is past its warm-up, eager until then and for device tensors."""
        graphed = self._rollout_graph(states)
        if graphed is not None:
            return graphed
        with torch.no_grad():
            prediction = self.network(states)
        return prediction, tensor(states)

    def _minibatch(self, entry, prepared=False, weight=1.0):
        """One minibatch update (PPO_agent.py:77-99) on already-gathered rows.  `prepared`: the optimisers are in
        graph mode and the caller has advanced their step scalars (FusedOptimizer.prepare_step).  `weight` (data
        parallel): rows here / rows of the GLOBAL minibatch -- the kernels' means are over the local rows, so
        weight * local gradient summed over ranks is the gradient of the global mean."""
        config = self.config
        dp = self.dp
        n_local = entry.state.size(0)
        if n_local > 0:
            prediction = self.network(entry.state, entry.action)
            out3, (g_lp, g_ent, g_v) = ops.ppo_loss(
                prediction['log_pi_a'].detach(), prediction['entropy'].detach(), prediction['v'].detach(),
                entry.log_pi_a, entry.advantage, entry.ret, config.ppo_ratio_clip, config.entropy_weight)
        else:       # this rank holds no row of the global minibatch: it still takes part in the exchange
            prediction, out3, g_lp, g_ent, g_v = None, torch.zeros(3, device=Config.DEVICE), None, None, None
        if config.shared_repr:
            self._fused.zero_grad(direct=not dp.active and prediction is not None)
            dp.set_weight(weight)       # (the fc4 segment of the exchange goes out from inside the backward pass: dist.py)
            if prediction is not None:
                from .nets import direct_param_grads
                defer = self._fused if (not dp.active and self.grad_hook is None
                                        and getattr(config, 'defer_conv_folds', True)) else None
                with direct_param_grads(not dp.active, defer_folds_to=defer, covers=[self._fused]):     # (one forward per minibatch: see A2CAgent._learn)
                    torch.autograd.backward([prediction['log_pi_a'], prediction['entropy'], prediction['v']],
                                            [g_lp, g_ent, g_v])
            dp.sum_grads(self._fused.flat.grad, weight)
            if self.grad_hook is not None:
                self.grad_hook(self._fused.flat.grad)
            self._fused.step(config.gradient_clip)
        else:
            approx_kl = out3[2].item()
            if dp.active:   # the KL gate (PPO_agent.py:88) must fall the same way on every rank: global mean KL
                approx_kl = dp.sum_scalars([approx_kl * weight])[0]
            if approx_kl <= 1.5 * config.target_kl:
                self._fused_actor.zero_grad()
                if prediction is not None:
                    torch.autograd.backward([prediction['log_pi_a'], prediction['entropy']], [g_lp, g_ent], retain_graph=True)
                dp.sum_grads(self._fused_actor.flat.grad, weight)
                self._fused_actor.step(None)
            self._fused_critic.zero_grad()
            if prediction is not None:
                prediction['v'].backward(g_v)
            dp.sum_grads(self._fused_critic.flat.grad, weight)
            self._fused_critic.step(None)
        return out3

    def optimize(self, entries):
        """PPO_agent.py:71-99: epochs of shuffled minibatches over the (detached) rollout entries."""
        config = self.config
        dp = self.dp
        if self._mlp.usable() and self._mlp.optimize(entries):      # all epochs x minibatches in one launch (csrc/ppo_mlp.hip)
            return
        self._mlp.sync_counts()
        if dp.invariant_sampling:        # G ranks, or one process asked to behave exactly like G ranks would
            return self._optimize_data_parallel(entries)
        if self._graphed.usable() and self._graphed.optimize(entries):
            return
        entry_cls = entries.__class__
        for _ in range(config.optimization_epochs):
            sampler = random_sample(np.arange(entries.state.size(0)), config.mini_batch_size)
            for batch_indices in sampler:
                batch_indices = tensor(batch_indices).long()
                entry = entry_cls(*[x[batch_indices] for x in entries])
                out3 = self._minibatch(entry)
        self.last_loss = out3

    def _optimize_data_parallel(self, entries):
        """The same epochs x minibatches over the GLOBAL rollout (T x N rows, time-major like Storage.extract): every rank
        draws the same permutation (dist.DataParallel.permutation), forms the same global minibatches as a single
        process would, and contributes the rows that belong to its environments [lo, hi)."""
        config, dp = self.config, self.dp
        entry_cls = entries.__class__
        n_glob, n_loc = dp.global_workers, dp.hi - dp.lo
        t_len = entries.state.size(0) // n_loc
        total = t_len * n_glob
        mb = config.mini_batch_size
        for _ in range(config.optimization_epochs):
            perm = np.asarray(dp.permutation(total))
            full = total // mb * mb
            batches = list(perm[:full].reshape(-1, mb)) + ([perm[full:]] if total % mb else [])
            for g_idx in batches:
                t, n = g_idx // n_glob, g_idx % n_glob
                mine = (n >= dp.lo) & (n < dp.hi)
                local = t[mine] * n_loc + (n[mine] - dp.lo)
                rows = tensor(local).long()
                entry = entry_cls(*[x[rows] for x in entries])
                out3 = self._minibatch(entry, weight=float(len(local)) / float(len(g_idx)))
        self.last_loss = out3


# ==================================================================================================== replay-based actor-critic
def _f32(x):
    """A sampled replay field as a float32 device tensor (the reference's tensor() narrows its f64 numpy batches to
    f32 BEFORE any arithmetic, torch_utils.py:20-25; the HBM ring hands back the stored dtype)."""
    return x.float() if isinstance(x, torch.Tensor) else tensor(x)


class _DeterministicPolicyAgent(_DeviceEpisodes, BaseAgent):
    """What DDPG_agent.py:13-100 and TD3_agent.py:13-108 share: one environment, a deterministic policy perturbed by a
    random process (uniform actions during warm-up), every transition fed to the uniform replay -- here the HBM ring:
    17-float states and 6-float actions are just small "frames" -- one sampled minibatch per step once warm, and a
    polyak-averaged target network.  Sub-classes provide `warm()` and `learn(batch)`.
    With config.fused_dpg_env = True (and fused_dpg_update) an envs.Pendulum / envs.SyntheticContinuous task moves to the device
    and a step is dpg_env.EnvStep's: one acting launch that writes the transition into the ring, the gather, the fused update."""

    def __init__(self, config):
        BaseAgent.__init__(self, config)
        self.config = config
        self.task = config.task_fn()
        self.network = config.network_fn()
        self.target_network = config.network_fn()
        self.target_network.load_state_dict(self.network.state_dict())
        self.replay = config.replay_fn()
        self.random_process = config.random_process_fn()
        self.total_steps = 0
        self.state = None

    def close(self):
        self.drain_episodes()
        close_obj(self.replay)
        close_obj(self.task)

    def _episode_ring(self):
        return getattr(self, '_dpg_env', None) or None

    def _fused_env(self):
        """dpg_env.EnvStep when `config.fused_dpg_env` is on and agent, task and replay allow it (decided once, ahead of the
        first step; a refusal is logged in ONE warning), else None: the host step below, unchanged."""
        env = getattr(self, '_dpg_env', False)
        if env is False:
            env = None
            if getattr(self.config, 'fused_dpg_env', False) is True:
                from . import dpg_env
                env = dpg_env.adopt(self)
            self._dpg_env = env
        return env

    def _flat_pair(self, target, src):
        """Both networks' parameters re-homed (once) into one flat fp32 buffer each, same tensor order and offsets; the
        modules and their torch optimizers keep seeing the same Parameter objects (views into the buffers)."""
        pair = getattr(self, '_soft_flat', None)
        if pair is None or pair[2] is not target or pair[3] is not src:
            tf, sf = FlatParams(list(target.parameters())), FlatParams(list(src.parameters()))
            if tf.offsets != sf.offsets or tf.numel != sf.numel:
                raise DraError("soft_update: target and source networks differ in parameter layout")
            for p in list(target.parameters()) + list(src.parameters()):
                p.grad = None        # FlatParams' gradient views are not used here (torch optimizers own the gradients)
            pair = self._soft_flat = (tf, sf, target, src)
        return pair[0].flat, pair[1].flat

    def soft_update(self, target, src):
        """target <- target * (1 - mix) + src * mix over every parameter (DDPG_agent.py:26-30): ONE launch of
        `dra_soft_update` over the two networks' flat parameter buffers."""
        t_flat, s_flat = self._flat_pair(target, src)
        ops.soft_update(t_flat, s_flat, self.config.target_network_mix)

    def _fused_dpg(self):
        """dpg_mlp.Update when `config.fused_dpg_update` is on and the agent is eligible (csrc/dpg_mlp.hip: the update as 4-5
        launches, the acting forward as one), else None: the module path below, unchanged.  Decided once, at first use; an
        agent that asked for the fused path and cannot have it says why in ONE warning."""
        fused = getattr(self, '_dpg', False)
        if fused is False:
            fused = None
            if getattr(self.config, 'fused_dpg_update', False) is True:
                from . import dpg_mlp
                why = dpg_mlp.why_not(self)
                if why is None:
                    fused = dpg_mlp.Update(self)
                else:
                    self.logger.warning('fused_dpg_update is on but this agent keeps the module path: %s' % why)
            self._dpg = fused
        return fused

    def _policy_step(self):
        """Whether this update also steps the actor and the targets (DDPG: always)."""
        return True

    def _fused_eval(self):
        """dpg_mlp.Update when config.fused_eval is on (with fused_dpg_update) and config.eval_env lives (from the first call on) on
        the device: evaluation is then ONE launch and one copy (dpg_mlp.Update.evaluate); None on every other path, and where the
        evaluation environment has to stay on the host (one warning says why)."""
        if getattr(self.config, 'fused_eval', False) is not True:
            return None
        fused = self._fused_dpg()
        if fused is None:
            return None
        return fused if fused.eval_vec() is not None else None

    def eval_episode(self):
        fused = self._fused_eval()
        if fused is None:
            return super().eval_episode()
        return float(fused.evaluate(1)[0])

    def eval_episodes(self):
        fused = self._fused_eval()
        if fused is None:
            return super().eval_episodes()
        self.drain_episodes()
        return self._report_eval(np.asarray([np.sum(r) for r in fused.evaluate(self.config.eval_episodes)]))

    def eval_step(self, state):
        norm = self.config.state_normalizer
        norm.set_read_only()
        fused = self._fused_dpg()
        with torch.no_grad():
            action = fused.act(norm(state)) if fused is not None else self.network(norm(state))
        norm.unset_read_only()
        return to_np(action)

    def _behaviour_action(self):
        space = self.task.action_space
        if self.total_steps < self.config.warm_up:
            action = [space.sample()]
        else:
            fused = self._fused_dpg()
            with torch.no_grad():
                action = to_np(fused.act(self.state) if fused is not None else self.network(self.state))
            action = action + self.random_process.sample()
        return np.clip(action, space.low, space.high)

    def step(self):
        config = self.config
        env = self._fused_env()
        if env is not None:
            env.step()
            return
        if self.state is None:
            self.random_process.reset_states()
            self.state = config.state_normalizer(self.task.reset())
        action = self._behaviour_action()
        next_state, reward, done, info = self.task.step(action)
        next_state = config.state_normalizer(next_state)
        self.record_online_return(info)
        reward = config.reward_normalizer(reward)
        self.replay.feed(dict(state=self.state, action=action, reward=reward, next_state=next_state,
                              mask=1 - np.asarray(done, dtype=np.int32)))
        if done[0]:
            self.random_process.reset_states()
        self.state = next_state
        self.total_steps += 1
        if self.warm():
            fused = self._fused_dpg()
            if fused is not None:
                # the same index draw as replay.sample(); the fields in the ring's stored dtype (the kernel narrows fp64 as it
                # loads: no cast launches), reward and mask as the gather's own fp32 outputs
                ring = getattr(self.replay, 'replay', self.replay)
                g = ring.gather(ring.draw_indices(), want_f32=True)
                # (the view: a one-dimensional action space comes back [B] from the ring and the kernels take [B, A]; no-op for A > 1)
                fused.learn(g['state'], g['action'].view(len(g['reward_f32']), -1), g['reward_f32'], g['next_state'], g['mask_f32'],
                            policy_step=self._policy_step())
                return
            tr = self.replay.sample()
            # (the view serves one-dimensional action spaces only, as above: the critic concatenates [B, S] with [B, A])
            self.learn(_f32(tr.state), _f32(tr.action).view(len(tr.reward), -1), _f32(tr.reward).unsqueeze(-1), _f32(tr.next_state),
                       _f32(tr.mask).unsqueeze(-1))


class DDPGAgent(_DeterministicPolicyAgent):
    """DDPG_agent.py:13-100."""

    def warm(self):
        return self.replay.size() >= self.config.warm_up

    def learn(self, states, actions, rewards, next_states, mask):
        net, tgt, gamma = self.network, self.target_network, self.config.discount
        with torch.no_grad():
            phi_next = tgt.feature(next_states)
            q_next = tgt.critic(phi_next, tgt.actor(phi_next))
            y = (gamma * mask * q_next).add_(rewards)
        critic_loss = (net.critic(net.feature(states), actions) - y).pow(2).mul(0.5).sum(-1).mean()
        net.zero_grad()
        critic_loss.backward()
        net.critic_opt.step()
        phi = net.feature(states)
        policy_loss = -net.critic(phi.detach(), net.actor(phi)).mean()
        net.zero_grad()
        policy_loss.backward()
        net.actor_opt.step()
        self.soft_update(tgt, net)


class TD3Agent(_DeterministicPolicyAgent):
    """TD3_agent.py:13-108: clipped double Q, target-policy smoothing, delayed policy / target updates (on the steps
    where total_steps % td3_delay is non-zero, as written at TD3_agent.py:100)."""

    def warm(self):
        return self.total_steps >= self.config.warm_up

    def _policy_step(self):
        return bool(self.total_steps % self.config.td3_delay)

    def learn(self, states, actions, rewards, next_states, mask):
        config, net, tgt = self.config, self.network, self.target_network
        space = self.task.action_space
        with torch.no_grad():
            a_next = tgt(next_states)
            noise = torch.randn_like(a_next).mul(config.td3_noise).clamp(-config.td3_noise_clip, config.td3_noise_clip)
            # (bounds as gym's Box gives them, one per dimension, or as one scalar: envs.Box of the synthetic tasks)
            low, high = (float(np.asarray(b).reshape(-1)[0]) for b in (space.low, space.high))
            a_next = (a_next + noise).clamp(low, high)
            y = rewards + config.discount * mask * torch.min(*tgt.q(next_states, a_next))
        q_1, q_2 = net.q(states, actions)
        critic_loss = F.mse_loss(q_1, y) + F.mse_loss(q_2, y)
        net.zero_grad()
        critic_loss.backward()
        net.critic_opt.step()
        if self.total_steps % config.td3_delay:
            policy_loss = -net.q(states, net(states))[0].mean()
            net.zero_grad()
            policy_loss.backward()
            net.actor_opt.step()
            self.soft_update(tgt, net)


# ==================================================================================================== option-critic
class OptionCriticAgent(_TargetRolloutAgent):
    """OptionCritic_agent.py:11-119: n-step option-critic over `num_workers` environments.  Per rollout step: one forward
    (q over options, termination beta, intra-option policies), an epsilon-soft option choice that keeps the previous
    option unless it terminates, an action from the chosen option's policy; per rollout: returns bootstrapped from the
    target network, three losses (option values, intra-option policy, termination) through ONE backward and the fused
    clip + optimizer step.  Draw order of the three Categorical samples per step is the reference's.
    option_critic_feature (examples.py:450-468) with config.fused_oc_feature = True runs on device-resident cart-poles instead
    (_step_feature over oc_mlp.Rollout: one rollout launch, one update launch); options and actions then come from uniforms
    staged per rollout by inverse CDF, not from Categorical.sample()'s own stream (oc_mlp's docstring)."""

    def __init__(self, config):
        BaseAgent.__init__(self, config)
        self.config = config
        self.task = config.task_fn()
        self.network = config.network_fn()
        self.target_network = config.network_fn()
        self.optimizer = config.optimizer_fn(self.network.parameters())
        self._fused = FusedOptimizer.adopt(self.optimizer)
        self._target_flat = FlatParams(list(self.target_network.parameters()),
                                       koc=nature_conv_weights(list(self.target_network.parameters())))
        self._sync_target()
        self.total_steps = 0
        self.worker_index = range_tensor(config.num_workers)
        self.grad_hook = None
        self._rollout_step = 0
        self._oc_rollout = _OCRollout(self)
        self._episodes = EpisodeRing(self, 0, config.num_workers)     # (the feature kernel's step counter: one stamp per rollout step)
        if self._adopt_device(self._oc_rollout):    # synthetic Atari emulators + OptionCriticNet(NatureConvBody): the rollout lives on the device
            self.states = self.task.reset()
            self.prev_options, self.is_initial_states = self._oc_rollout.state(config.num_workers)
            return
        self.states = config.state_normalizer(self.task.reset())
        # option_critic_feature, examples.py:450-468 (opt-in, config.fused_oc_feature): cart-poles under OptionCriticNet over a small
        # FCBody live on the device, one launch per rollout and one per update (csrc/oc_mlp.hip)
        self._feature = self._adopt_feature()       # (the environments move as reset() left them)
        if self._feature is not None:
            self.prev_options, self.is_initial_states = self._feature.state(config.num_workers)
            return
        self.is_initial_states = torch.ones(config.num_workers, dtype=torch.bool, device=Config.DEVICE)
        self.prev_options = torch.ones(config.num_workers, dtype=torch.int64, device=Config.DEVICE)

    def _adopt_feature(self):
        from . import mlp_rollout, oc_mlp
        return mlp_rollout.adopt(self, oc_mlp.Rollout)

    def _feature_state(self):
        return dict(prev_option=self.prev_options.cpu().numpy().copy(), is_initial=self.is_initial_states.cpu().numpy().copy())

    def _load_feature_state(self, state):
        self.prev_options.copy_(torch.from_numpy(np.asarray(state['prev_option'])))
        self.is_initial_states.copy_(torch.from_numpy(np.asarray(state['is_initial'])))

    def _feature_learn(self, plan):
        """OptionCritic_agent.py:55-116 on the device: the rollout launch, then the update launch (config.fused_oc_update False:
        the module path on the rollout's buffers -- returns by the scan kernel, the detached terms from the stored q, one batched
        forward, the three losses in torch, autograd), then the fused clip + optimizer step.  -> the total loss [1];
        `last_losses` [4] = (total, q_loss, pi_loss, beta_loss)."""
        config = self.config
        rollout = self._feature
        b = rollout.run(plan.t_len)
        self._rollout_step += plan.t_len
        if getattr(config, 'fused_oc_update', True) is not False:
            losses = rollout.update(b, config)
        else:
            t_len, n = b['action'].shape
            rows = t_len * n
            ret = self._scan_returns(b)
            q_s = b['q'].view(rows, -1)
            option, prev, action = b['option'].view(rows, 1), b['prev_option'].view(rows, 1), b['action'].view(rows, 1)
            eps = rollout.eps.view(t_len, 1).expand(t_len, n).reshape(rows, 1)
            adv = ret - q_s.gather(1, option)
            v = q_s.max(dim=-1, keepdim=True)[0] * (1 - eps) + q_s.mean(-1).unsqueeze(-1) * eps
            beta_adv = q_s.gather(1, prev) - v + config.termination_regularizer
            b['ret'].copy_(ret.view(t_len, n))
            b['adv'].copy_(adv.view(t_len, n))
            b['beta_adv'].copy_(beta_adv.view(t_len, n))
            pred = self.network(b['state'].view(rows, -1))
            rows_i = torch.arange(rows, device=option.device)
            log_pi, pi = pred['log_pi'][rows_i, option.view(-1)], pred['pi'][rows_i, option.view(-1)]
            entropy = -(pi * log_pi).sum(-1, keepdim=True)      # (Categorical.entropy without its argument checks: no sync)
            q_loss = (pred['q'].gather(1, option) - ret).pow(2).mul(0.5).mean()
            pi_loss = (-(log_pi.gather(1, action) * adv) - config.entropy_weight * entropy).mean()
            beta_loss = (pred['beta'].gather(1, prev) * beta_adv * (1 - b['init'].view(rows, 1))).mean()
            total = pi_loss + q_loss + beta_loss
            self._fused.zero_grad()
            total.backward()
            losses = torch.stack([total.detach(), q_loss.detach(), pi_loss.detach(), beta_loss.detach()])
        self._fused.step(config.gradient_clip)
        self.last_losses = losses
        return losses[:1]

    def sample_option(self, prediction, epsilon, prev_option, is_initial):
        with torch.no_grad():
            q = prediction['q']
            n_opt = q.size(1)
            pi = torch.full_like(q, epsilon / n_opt)                       # epsilon-soft over options ...
            pi.scatter_(1, q.argmax(dim=-1, keepdim=True), 1 - epsilon + epsilon / n_opt)
            keep = torch.zeros_like(q)
            keep[self.worker_index, prev_option] = 1
            beta = prediction['beta']
            pi_hat = (1 - beta) * keep + beta * pi                         # ... unless the previous option continues
            fresh = torch.distributions.Categorical(probs=pi).sample()
            continued = torch.distributions.Categorical(probs=pi_hat).sample()
            return torch.where(is_initial, fresh, continued)

    def step(self):
        if self._feature is not None:
            return self._step_feature()
        if getattr(self.task, 'on_device', False):
            return self._step_device()
        config = self.config
        n, w = config.rollout_length, self.worker_index
        storage = Storage(n, ['beta', 'option', 'beta_advantage', 'prev_option', 'init_state', 'eps'])
        for _ in range(n):
            prediction = self.network(self.states)
            epsilon = config.random_option_prob(config.num_workers)
            options = self.sample_option(prediction, epsilon, self.prev_options, self.is_initial_states)
            prediction['pi'] = prediction['pi'][w, options]
            prediction['log_pi'] = prediction['log_pi'][w, options]
            policy = torch.distributions.Categorical(probs=prediction['pi'])
            actions = policy.sample()
            next_states, rewards, terminals, info = self.task.step(to_np(actions))
            self.record_online_return(info)
            storage.feed(prediction)
            storage.feed({'reward': tensor(config.reward_normalizer(rewards)).unsqueeze(-1),
                          'mask': tensor(1 - terminals).unsqueeze(-1), 'option': options.unsqueeze(-1),
                          'prev_option': self.prev_options.unsqueeze(-1), 'entropy': policy.entropy().unsqueeze(-1),
                          'action': actions.unsqueeze(-1), 'init_state': self.is_initial_states.unsqueeze(-1).float(),
                          'eps': epsilon})
            self.is_initial_states = torch.as_tensor(np.asarray(terminals), device=Config.DEVICE).bool()
            self.prev_options = options
            self.states = config.state_normalizer(next_states)
            self.total_steps += config.num_workers
            if self.total_steps // config.num_workers % config.target_network_update_freq == 0:
                self._sync_target()
        with torch.no_grad():
            boot = self.target_network(self.states)
            storage.placeholder()
            beta = boot['beta'][w, self.prev_options]
            ret = ((1 - beta) * boot['q'][w, self.prev_options] + beta * boot['q'].max(dim=-1)[0]).unsqueeze(-1)
            for i in reversed(range(n)):
                q_i = storage.q[i].detach()
                ret = storage.reward[i] + config.discount * storage.mask[i] * ret
                storage.ret[i] = ret
                storage.advantage[i] = ret - q_i.gather(1, storage.option[i])
                v = q_i.max(dim=-1, keepdim=True)[0] * (1 - storage.eps[i]) + q_i.mean(-1).unsqueeze(-1) * storage.eps[i]
                storage.beta_advantage[i] = q_i.gather(1, storage.prev_option[i]) - v + config.termination_regularizer
        e = storage.extract(['q', 'beta', 'log_pi', 'ret', 'advantage', 'beta_advantage', 'entropy', 'option', 'action',
                             'init_state', 'prev_option'])
        q_loss = (e.q.gather(1, e.option) - e.ret).pow(2).mul(0.5).mean()
        pi_loss = (-(e.log_pi.gather(1, e.action) * e.advantage) - config.entropy_weight * e.entropy).mean()
        beta_loss = (e.beta.gather(1, e.prev_option) * e.beta_advantage * (1 - e.init_state)).mean()
        self._fused.zero_grad()
        (pi_loss + q_loss + beta_loss).backward()
        self._fused.step(config.gradient_clip)
