"""Host side of dra_dqn_replay_mlp_update (csrc/dqn_mlp.hip): dqn_feature (examples.py:11-52) with the replay options its keyword
arguments take -- an n-step window (`n_step`) and / or a PrioritizedReplay (`replay_cls`) -- over dqn_mlp's device-resident cart-pole
and HBM replay ring.  Opt-in under a switch of its own, config.fused_dqn_replay_feature: config.fused_dqn_feature keeps refusing both
options.

Acting and evaluation are dqn_mlp's launches as they are (dra_dqn_mlp_act writes 1-step rows into the ring); the update launch is
dqn_mlp's kernel over a window with optional priorities.  Two kinds over it, picked by the replay's type (`adopt`):

  WindowKind   a UniformReplay with n_step 1..8: dqn_mlp.Step's draws (draw_indices honours the window), no weights, no priorities.
  PerKind      a PrioritizedReplay with n_step 1..8: the host makes the step's draws in the host path's order --
               plan_actor_epsilon_greedy, the tree's adds (`PrioritizedReplay.advance`), past exploration_steps the prioritised draw
               (python `random`, the descent on the device, ONE host wait) and ONE config.replay_beta() call -- and stages the
               probabilities with beta directly behind them; the priorities' commit runs eagerly behind the learn region
               (rainbow_mlp.Step: DESIGN.md 4.17).

config.fused_dqn_replay_update False: ring.gather (its n-step fold) on the staged indices and the agent's own _loss_grad
(ops.td_loss with the device beta behind the probabilities).  There is no CPU / eager-PyTorch implementation here: without the HIP
library every call raises.
"""
import ctypes

import numpy as np
import torch

from . import dqn_mlp
from .mlp_rollout import shape_table
from .support import plan_actor_epsilon_greedy

SWITCH = 'fused_dqn_replay_feature'
UPDATE_SWITCH = 'fused_dqn_replay_update'
MAX_B, MAX_N_STEP = dqn_mlp.MAX_B, 8


class UpdateIO(ctypes.Structure):
    """Mirror of dra_dqn_replay_mlp_update_io (include/deeprl_amd.h)."""
    _fields_ = [("ring_frames", ctypes.c_void_p), ("ring_actions", ctypes.c_void_p), ("ring_rewards", ctypes.c_void_p),
                ("ring_masks", ctypes.c_void_p), ("idx", ctypes.c_void_p), ("prob", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("grad", ctypes.c_void_p), ("out_q_target", ctypes.c_void_p), ("out_td", ctypes.c_void_p),
                ("out_loss", ctypes.c_void_p), ("out_prio", ctypes.c_void_p), ("out_weights", ctypes.c_void_p),
                ("err", ctypes.c_void_p), ("capacity", ctypes.c_int64), ("discount", ctypes.c_double),
                ("step_discount", ctypes.c_double), ("replay_eps", ctypes.c_double), ("replay_alpha", ctypes.c_double),
                ("batch", ctypes.c_int32), ("double_q", ctypes.c_int32), ("n_step", ctypes.c_int32), ("reserved", ctypes.c_int32)]


update_supported = shape_table('dra_dqn_replay_mlp_update_supported')     # (state_dim, n_actions, hidden, batch, gate, n_step)


class WindowKind(dqn_mlp.Kind):
    """dqn_mlp.Kind for dqn_feature over a UniformReplay with an n-step window."""
    SWITCH, UPDATE_SWITCH = SWITCH, UPDATE_SWITCH
    UPDATE = 'dra_dqn_replay_mlp_update'
    PRIORITIZED, MAX_N_STEP = False, MAX_N_STEP
    # (dqn_mlp.why_not knows no window: extra() asks the table again with the replay's n_step)
    update_supported = staticmethod(lambda *dims: update_supported(*dims, 1))

    @classmethod
    def extra(cls, agent, shp):
        cfg, rp = agent.config, agent._inner_replay()
        if int(rp.memory_size) < int(cfg.sgd_update_frequency) + int(rp.n_step) + 1:
            return "the replay holds fewer slots than an agent step and an n-step window need"
        if float(rp.discount) != float(cfg.discount):
            return "the replay's discount is not the configuration's"
        b, n_step = int(rp.batch_size), int(rp.n_step)
        if cls.fused_update(cfg, shp) and not update_supported(shp[0], shp[1], shp[2], b, shp[3], n_step):
            return "%s is not built for minibatches of %d over an n-step window of %d" % (cls.UPDATE, b, n_step)
        return None


class PerKind(WindowKind):
    """dqn_mlp.Kind for dqn_feature over a PrioritizedReplay with an n-step window."""
    PRIORITIZED = True


def kind_of(agent):
    """The kind the agent's replay asks for."""
    from .replay import PrioritizedReplay
    return PerKind if isinstance(agent._inner_replay(), PrioritizedReplay) else WindowKind


def why_not(agent, supported_fn=None, update_supported_fn=None):
    """None when `agent` (a DQNAgent on dqn_feature's kind of configuration) may run on the kernels under this module's switch,
    else the first reason it may not: dqn_mlp.why_not's list for the kind of the agent's replay."""
    return dqn_mlp.why_not(agent, supported_fn, update_supported_fn, kind=kind_of(agent))


class Step(dqn_mlp.Step):
    """dqn_mlp.Step over the window's update launch: the update's io is this class's; everything else is the parent's."""
    KIND = WindowKind

    def replay_io(self):
        """dra_dqn_replay_mlp_update_io with the outputs, the window and (a subclass: the priorities) set."""
        rp = self.agent._inner_replay()
        io = UpdateIO()
        io.out_q_target, io.out_td, io.out_loss = self.q_target.data_ptr(), self.td.data_ptr(), self.loss.data_ptr()
        io.step_discount, io.n_step = float(rp.discount), int(rp.n_step)
        return io

    def update(self):
        """dra_dqn_replay_mlp_update on the staged indices: the gradient lands in the optimiser's flat gradient buffer."""
        return self.launch_update(self.replay_io())


class PerStep(Step):
    """Step over a PrioritizedReplay: the staged probabilities and beta, the prioritised draw in prepare, the priority and weight
    buffers and the commit behind the learn region are this class's."""
    KIND = PerKind

    def __init__(self, agent, shp):
        Step.__init__(self, agent, shp)
        d, b = self._up.dev, self.batch
        self.prob = d[self._o_prob:self._o_prob + 4 * b].view(torch.float32)
        self.beta = d[self._o_beta:self._o_beta + 4].view(torch.float32)
        self.tree_idx = None            # the last draw's leaves: what the commit behind the learn region gates on

    def staged_tail(self):
        """The sampling probabilities (f32 [B]) behind the parent's block and beta (f32) DIRECTLY behind the last of them: where
        ops.td_loss reads a device beta (beta < 0: sampling_prob[B])."""
        self._o_prob = self._o_tail
        self._o_beta = self._o_prob + 4 * self.batch
        return (4 * self.batch + 4 + 7) // 8 * 8

    def make_outputs(self, dev):
        Step.make_outputs(self, dev)
        self.prio = torch.zeros(self.batch, dtype=torch.float32, device=dev)
        self.weights = torch.zeros(self.batch, dtype=torch.float32, device=dev)

    def replay_io(self):
        cfg = self.agent.config
        io = Step.replay_io(self)
        io.prob, io.beta = self.prob.data_ptr(), self.beta.data_ptr()
        io.replay_eps, io.replay_alpha = float(cfg.replay_eps), float(cfg.replay_alpha)
        io.out_prio, io.out_weights = self.prio.data_ptr(), self.weights.data_ptr()
        return io

    def module_update(self):
        """config.fused_dqn_replay_update False: ring.gather on the staged indices (its n-step fold), then the agent's own
        _loss_grad (the modules' forwards, ops.td_loss on the staged probabilities with the device beta behind them, autograd);
        the priorities land in self.prio, where the commit reads them."""
        agent = self.agent
        cfg, rp = agent.config, agent._inner_replay()
        self.static = g = rp.gather(self.idx, out=self.static)
        tr = rp.TransitionCLS(state=g['state'], action=g['action'], reward=g['reward'], next_state=g['next_state'], mask=g['mask'],
                              sampling_prob=self.prob, idx=None)
        per = dict(sampling_prob=self.prob, beta=-1.0, replay_eps=cfg.replay_eps, replay_alpha=cfg.replay_alpha)
        out, (net_out, grad) = agent._loss_grad(tr, per)
        self.prio.copy_(out['prio'])
        agent._fused.zero_grad()
        agent._backward(net_out, grad)
        return out['loss']

    def prepare(self):
        """The step's draws in the host path's order: per transition the epsilon of DQN_agent.py:34-39 and epsilon_greedy's two
        draws, the feed's bookkeeping with the tree's adds, then (total_steps > exploration_steps) the prioritised draw and ONE
        replay_beta() call -- staged with one copy.  -> whether the step updates."""
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
        raw = self._up.stage().numpy()
        raw[:8].view(np.int64)[0] = slot0
        raw[self._o_rand:self._o_flag].view(np.int64)[...] = rand
        raw[self._o_flag:self._o_flag + k] = explore
        idx = None
        if learn:
            self.tree_idx, prob, idx = rp.draw()
            raw[self._o_idx:self._o_rand].view(np.int64)[...] = idx
            raw[self._o_prob:self._o_beta].view(np.float32)[...] = prob
            raw[self._o_beta:self._o_beta + 4].view(np.float32)[0] = cfg.replay_beta()
        self._up.send()
        self.last_draws = (explore, rand, slot0, idx)
        return learn

    def after_learn(self):
        """replay.py:193-196 with the priorities still on the device: the pending marks and first-writer-wins are gated on the
        host, so the commit runs eagerly behind the replayed region, as the target copy does."""
        self.agent._inner_replay().commit_device(self.tree_idx, self.prio)


def adopt(agent):
    """A Step of the kind the agent's replay asks for, with the actor's environment on the device, when configuration, agent and
    task allow it; else None (the host path; with the switch on the reason is logged once)."""
    return dqn_mlp.adopt(agent, PerStep if kind_of(agent) is PerKind else Step)
