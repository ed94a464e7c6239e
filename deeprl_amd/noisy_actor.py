"""Rainbow's actor and environment on the device (config.device_noisy_actor).

The `sgd_update_frequency` transitions of one DQNAgent.step() (DQN_agent.py:26-45, 101-113) as ONE batched, sync-free block:

  * the synthetic Atari environment ignores actions -- frames, rewards and terminals are hashes of its frame counter -- so the
    observations of all R transitions of an agent step are known before any forward runs (learner.SyntheticEpisodeStream is
    the host shadow, as for the dqn_pixel pipeline);
  * a noisy actor's epsilon is 0 (DQN_agent.py:34-35): the action is a pure argmax and stays on the device;
  * the R transitions see the same parameters (the update follows them) and differ only in their noise draws
    (reset_noise() before each forward, DQN_agent.py:28-29): one batch-R forward whose noisy layers take one draw per row
    (csrc/noisy.hip dra_noisy_linear_fwd_rows).

Per agent step the host draws the R x 9 noise vectors (torch's CPU generator, the reference's stream: nets._NoiseBlock.draw_rows),
advances the shadow by R transitions, consumes np.random as epsilon_greedy(0, q[1, A]) does, and uploads one small plan; the
device runs synth_stacks -> normaliser table -> conv1-3 at batch R -> fc4 / value / advantage with per-row noise ->
dra_rainbow_act_rows -> dra_ring_put_rows, eagerly for the first two agent steps and as one captured graph afterwards.  No D2H
copy and no synchronisation inside the block.  The update is the agent's own (graphs._GraphedUpdate or the eager _learn).
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import ops
from ._lib import lib, stream_ptr
from .graphs import Region, _fused_noisy
from .support import Config

MAX_ROWS = 8

Block = namedtuple("Block", ["slot0", "counters", "ages", "rewards", "masks", "infos"])


def _env_of(agent):
    task = getattr(getattr(agent, 'actor', None), '_task', None)
    envs = getattr(getattr(task, 'env', None), 'envs', None)
    return envs[0] if envs and len(envs) == 1 else None


def why_not(agent):
    """None when `agent` may run its actor and environment on the device, else the first condition that fails, in words."""
    from .agents import CategoricalDQNAgent
    from .envs import SyntheticAtari
    from .nets import NatureConvBody, NoisyLinear, RainbowNet
    from .normalizers import ImageNormalizer, RescaleNormalizer, SignNormalizer
    from .replay import PrioritizedReplay, UniformReplay
    cfg = agent.config
    if getattr(cfg, 'device_noisy_actor', False) is not True:
        return "config.device_noisy_actor is off"
    if Config.DEVICE.type != 'cuda':
        return "the device is not a GPU"
    if getattr(cfg, 'device_env', True) is False:
        return "config.device_env is False"
    if not isinstance(agent, CategoricalDQNAgent):
        return "the agent is not a CategoricalDQNAgent"
    for net in (agent.network, agent.target_network):
        body = getattr(net, 'body', None)
        if type(net) is not RainbowNet or type(body) is not NatureConvBody or not net.noisy_linear or not body.noisy_linear \
                or not all(isinstance(m, NoisyLinear) for m in (net.fc_value, net.fc_advantage, body.fc4)):
            return "the network is not RainbowNet(NatureConvBody(noisy_linear=True), noisy_linear=True)"
    if not cfg.noisy_linear:
        return "config.noisy_linear is off (the actor would explore with epsilon > 0)"
    if not (_fused_noisy(cfg, agent.network) and _fused_noisy(cfg, agent.target_network)):
        return "the noisy layers are not on csrc/noisy.hip (config.fused_noisy)"
    env = _env_of(agent)
    if type(env) is not SyntheticAtari:
        return "the actor's task is not one SyntheticAtari environment"
    if env.frames is not None:
        return "the environment has already been stepped on the host"
    if env.history != 4 or env.n_actions != cfg.action_dim:
        return "the environment's history is not 4 (or its actions are not config.action_dim)"
    if type(cfg.state_normalizer) is not ImageNormalizer:
        return "the state normaliser is not ImageNormalizer"
    rn = cfg.reward_normalizer
    if not (type(rn) is SignNormalizer or (type(rn) is RescaleNormalizer and rn.coef == 1.0)):
        return "the reward normaliser is neither SignNormalizer nor RescaleNormalizer(1.0)"
    rp = getattr(agent.replay, 'replay', agent.replay)
    if type(rp) not in (UniformReplay, PrioritizedReplay) or rp.history_length != 4:
        return "the replay is not a UniformReplay / PrioritizedReplay with history_length 4"
    if not 1 <= int(cfg.sgd_update_frequency) <= MAX_ROWS:
        return "sgd_update_frequency is outside [1, %d]" % MAX_ROWS
    if rp.memory_size < int(cfg.sgd_update_frequency):
        return "the replay holds fewer slots than one agent step feeds"
    if cfg.action_dim > 64 or int(cfg.categorical_n_atoms) > 64:
        return "action_dim or categorical_n_atoms is above 64"
    return None


class ActorPlan:
    """Host side of the agent steps of one device-resident actor: per call of next() the R transitions of one agent step from
    the episode shadow -- first ring slot, per row the observation's counter and episode age, the normalised reward (f64) and
    the mask (i32), the infos -- with np.random consumed as epsilon_greedy(0, q[1, A]) consumes it per transition (torch_utils.py:
    51-58, 2-D branch: randint(A, size=1), then rand(1); the values are not used, epsilon is 0)."""

    def __init__(self, stream, reward_normalizer, n_actions, rows, capacity, slot0=0):
        self.stream, self.reward_normalizer = stream, reward_normalizer
        self.n_actions, self.rows, self.capacity = int(n_actions), int(rows), int(capacity)
        self.slot = int(slot0)
        # [slot0 i64 | counters i64 R | rewards f64 R | ages i32 R | masks i32 R]
        r = self.rows
        self.offsets = dict(slot0=0, counters=8, rewards=8 + 8 * r, ages=8 + 16 * r, masks=8 + 20 * r)
        self.nbytes = 8 + 24 * r

    def next(self):
        from .learner import actor_randomness_block
        r = self.rows
        counters, ages = np.empty(r, dtype=np.int64), np.empty(r, dtype=np.int32)
        rewards, masks = np.empty(r, dtype=np.float64), np.empty(r, dtype=np.int32)
        infos = []
        for i in range(r):
            c, _, age, reward, done, info = self.stream.transition()
            counters[i], ages[i] = c, age
            rewards[i] = self.reward_normalizer(reward)
            masks[i] = 1 - int(done)
            infos.append(info)
        if actor_randomness_block(np.random, self.n_actions, r) is None:      # (not a power of two: the scalar calls themselves)
            for _ in range(r):
                np.random.randint(self.n_actions, size=1)
                np.random.rand(1)
        slot0 = self.slot
        self.slot = (slot0 + r) % self.capacity
        return Block(slot0, counters, ages, rewards, masks, infos)

    def pack(self, block, out):
        """The block as the bytes of one upload (out: uint8 array of self.nbytes)."""
        o, r = self.offsets, self.rows
        out[0:8].view(np.int64)[0] = block.slot0
        out[o['counters']:o['counters'] + 8 * r].view(np.int64)[:] = block.counters
        out[o['rewards']:o['rewards'] + 8 * r].view(np.float64)[:] = block.rewards
        out[o['ages']:o['ages'] + 4 * r].view(np.int32)[:] = block.ages
        out[o['masks']:o['masks'] + 4 * r].view(np.int32)[:] = block.masks
        return out


class NoisyActor:
    """The actor block of a Rainbow agent whose environment lives on the device (see the module docstring)."""
    WARMUP = 2
    graph = property(lambda self: self.region.graph)

    def __init__(self, agent, env):
        from .learner import SyntheticEpisodeStream
        from .replay import _PinnedUploader
        cfg = agent.config
        self.agent = agent
        self.rows = int(cfg.sgd_update_frequency)
        self.rp = getattr(agent.replay, 'replay', agent.replay)
        ring = self.rp.device_ring()
        if ring.frame_bytes != 7056 or ring.action_bytes != 8:
            raise ops.DraError("device_noisy_actor: the replay ring does not hold 84x84 uint8 frames and int64 actions")
        env.frames = "device"           # the host emulator is retired: stepping it too would fork the streams
        self.shadow = SyntheticEpisodeStream(env.seed, env.counter, env.done_period, env.history)
        self.plan = ActorPlan(self.shadow, cfg.reward_normalizer, cfg.action_dim, self.rows, self.rp.memory_size, self.rp.pos)
        dev = Config.DEVICE
        r, o = self.rows, self.plan.offsets
        self.words = torch.zeros(self.plan.nbytes, dtype=torch.uint8, device=dev)
        self._up = _PinnedUploader(torch.uint8, self.plan.nbytes, dev)
        self._host = np.zeros(self.plan.nbytes, dtype=np.uint8)
        w = self.words
        self.slot0 = w[0:8].view(torch.int64)
        self.counters = w[o['counters']:o['counters'] + 8 * r].view(torch.int64)
        self.rewards = w[o['rewards']:o['rewards'] + 8 * r].view(torch.float64)
        self.ages = w[o['ages']:o['ages'] + 4 * r].view(torch.int32)
        self.masks = w[o['masks']:o['masks'] + 4 * r].view(torch.int32)
        self.seeds = torch.full((r,), int(env.seed), dtype=torch.int64, device=dev)
        self.stacks = torch.zeros((r, env.history, 84, 84), dtype=torch.uint8, device=dev)
        self.actions = torch.zeros(r, dtype=torch.int64, device=dev)
        self.atoms = agent.atoms.float().contiguous()
        self.region = Region("the device-resident noisy actor", cfg, self.WARMUP)
        self.noise = None               # the [R][numel] device block of the last draw_rows()

    def _layer(self, x, layer, name, act=None):
        nb = self.agent.network.noise_block()
        e = []
        for bname in layer.NOISE_NAMES:
            o, n = nb.slices[(name, bname)]
            e.append(self.noise[:, o:o + n])
        return ops.noisy_linear_fwd_rows(x, layer.weight_mu, layer.weight_sigma, layer.bias_mu, layer.bias_sigma, e[0], e[1], e[2],
                                         act=act)

    def _device_block(self):
        """Everything the device does for the R transitions: static addresses only, no host value in any argument."""
        net, r, cfg = self.agent.network, self.rows, self.agent.config
        lib.dra_synth_stacks(ctypes.c_void_p(self.counters.data_ptr()), ctypes.c_void_p(self.ages.data_ptr()),
                             ctypes.c_void_p(self.seeds.data_ptr()), r, self.stacks.shape[1], ctypes.c_void_p(self.stacks.data_ptr()),
                             stream_ptr())
        body = net.body
        y = body.conv3(body.conv2(body.conv1(cfg.state_normalizer(self.stacks))))
        phi = self._layer(y.view(r, -1), body.fc4, 'body.fc4', act=body.fc4.fused_act)
        value = self._layer(phi, net.fc_value, 'fc_value')
        adv = self._layer(phi, net.fc_advantage, 'fc_advantage')
        ops.rainbow_act_rows(value, adv.view(r, net.action_dim, net.num_atoms), self.atoms, action=self.actions)
        hist = self.stacks.shape[1]
        newest = self.stacks.view(r, hist, 7056)[:, hist - 1]
        self.rp._ring.put_rows(r, newest, hist * 7056, self.actions, self.rewards, self.masks, slot0_dev=self.slot0)

    def step(self):
        """One agent step's transitions -> their infos (episodic returns), the ring and the replay's cursor advanced."""
        agent = self.agent
        nb = agent.network.noise_block()
        block = self.plan.next()
        region = self.region
        with torch.no_grad():
            self.noise = nb.draw_rows(self.rows)
            key = self.noise.data_ptr()         # (the noise block moves when it is rebuilt: Module.to())
            self._up.upload_into(self.words, self.plan.pack(block, self._host))
            if region.due(key) and (region.graph is not None or region.capture(self._device_block, key)):
                region.replay()
            else:
                self._device_block()
        self.rp.advance(self.rows)
        agent.actor._total_steps += self.rows
        return block.infos
