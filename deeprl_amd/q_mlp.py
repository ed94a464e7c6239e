"""Host side of csrc/q_mlp.hip: n_step_dqn_feature (examples.py:408-424) over device-resident cart-pole environments.

`shape(network)` says whether a network is one the kernels walk (VanillaNet over a two-layer FCBody of one width with a relu or
tanh gate and a plain biased fc_head); `why_not(agent)` adds the agent-side conditions and names the first one that fails;
`Rollout(agent)` builds the kernels' structs over the agent's flat parameter buffer and the TARGET network's flat buffer of the
same layout, stages the rollout's exploration draws (support.plan_epsilon_greedy: the reference's draw order) and launches a
rollout (NStepDQN_agent.py:31-57: one launch instead of T x [forward, download q, 5 environment steps, upload]); `update(...)`
is NStepDQN_agent.py:58-65 with the whole backward as one more launch.  There is no CPU / eager implementation here: without the
HIP library every call raises.
"""
import ctypes

import numpy as np
import torch

from . import mlp_rollout
from ._lib import lib, stream_ptr
from .device_env import DeviceCartPoleVec
from .mlp_rollout import GATES, body_params, fc_body, head_out, shape_table      # noqa: F401  (GATES: this module's public name)
from .support import Config, StagedUpload, plan_epsilon_greedy


class Net(ctypes.Structure):
    """Mirror of dra_q_mlp_net (include/deeprl_amd.h)."""
    _fields_ = [("param", ctypes.c_void_p), ("target", ctypes.c_void_p),
                ("w1", ctypes.c_int32), ("b1", ctypes.c_int32), ("w2", ctypes.c_int32), ("b2", ctypes.c_int32),
                ("wq", ctypes.c_int32), ("bq", ctypes.c_int32),
                ("gate", ctypes.c_int32), ("state_dim", ctypes.c_int32), ("n_actions", ctypes.c_int32),
                ("hidden", ctypes.c_int32)]


class RolloutIO(ctypes.Structure):
    """Mirror of dra_q_mlp_rollout_io."""
    _fields_ = [("env_state", ctypes.c_void_p), ("env_counter", ctypes.c_void_p), ("ep_steps", ctypes.c_void_p),
                ("ep_return", ctypes.c_void_p), ("env_seed", ctypes.c_void_p), ("step_counter", ctypes.c_void_p),
                ("ep_count", ctypes.c_void_p), ("ep_ring", ctypes.c_void_p),
                ("explore", ctypes.c_void_p), ("random_action", ctypes.c_void_p),
                ("out_state", ctypes.c_void_p), ("out_q", ctypes.c_void_p), ("out_action", ctypes.c_void_p),
                ("out_reward", ctypes.c_void_p), ("out_mask", ctypes.c_void_p), ("bootstrap", ctypes.c_void_p),
                ("horizon", ctypes.c_int64), ("ring_cap", ctypes.c_int64), ("reward_coef", ctypes.c_double),
                ("t_len", ctypes.c_int32), ("n_env", ctypes.c_int32)]


class UpdateIO(ctypes.Structure):
    """Mirror of dra_q_mlp_update_io."""
    _fields_ = [("state", ctypes.c_void_p), ("action", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("bootstrap", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("out_ret", ctypes.c_void_p),
                ("out_loss", ctypes.c_void_p), ("discount", ctypes.c_double), ("t_len", ctypes.c_int32), ("n_env", ctypes.c_int32)]


def shape(network):
    """(state_dim, n_actions, hidden, gate code) when `network` is a VanillaNet whose body is a two-layer FCBody of one width with
    a relu or tanh gate and whose fc_head is a plain Linear layer with a bias; else None."""
    from .nets import VanillaNet
    if type(network) is not VanillaNet:
        return None
    body = fc_body(network.body)
    if body is None or body[1] != body[2]:
        return None
    s_dim, hidden, _, gate = body
    n_actions = head_out(network.fc_head, hidden)
    if n_actions is None or network.fc_head.fused_act is not None:
        return None
    return s_dim, n_actions, hidden, gate


supported = shape_table('dra_q_mlp_supported')                    # (state_dim, n_actions, hidden, n_env, gate): the rollout kernel
update_supported = shape_table('dra_q_mlp_update_supported')      # (.., rows = rollout length x environments, gate): the update kernel


def _fields(net):
    return list(zip(("w1", "b1", "w2", "b2", "wq", "bq"), body_params(net.body) + [net.fc_head.weight, net.fc_head.bias]))


def why_not(agent, supported_fn=supported):
    """None when NStepDQNAgent may run `agent` on the kernels, else the first reason it may not (all but the task itself, which
    DeviceCartPoleVec.eligible decides): mlp_rollout.why_not's -- opt-in: config.fused_nstep_feature must be True --, then the target's."""
    why = mlp_rollout.why_not(Rollout, agent, supported_fn)
    if why is not None:
        return why
    return Rollout.target_why_not(agent, shape(agent.network))


def update(net, state, action, reward, mask, bootstrap, discount, grad, out_ret, out_loss):
    """dra_q_mlp_update on the current stream: returns, loss and the gradient of 0.5 mean (q_a - ret)^2 with respect to the six
    tensors `net` (a Net struct) names, written into the flat buffer `grad` at the parameters' offsets.  state [T, N, 4], action
    int64 [T, N], reward / mask [T, N], bootstrap [N]; out_ret [T, N], out_loss [1]."""
    io = UpdateIO()
    io.state, io.action, io.reward, io.mask = state.data_ptr(), action.data_ptr(), reward.data_ptr(), mask.data_ptr()
    io.bootstrap, io.grad, io.out_ret, io.out_loss = bootstrap.data_ptr(), grad.data_ptr(), out_ret.data_ptr(), out_loss.data_ptr()
    io.discount, io.t_len, io.n_env = float(discount), int(action.shape[0]), int(action.shape[1])
    lib.dra_q_mlp_update(ctypes.byref(net), ctypes.byref(io), stream_ptr())


class Rollout(mlp_rollout.TargetRollout):
    """dra_q_mlp_rollout over a DeviceCartPoleVec, the agent's flat parameter buffer and its target network's."""
    SWITCH, ENTRY, VEC, OPT_IN = 'fused_nstep_feature', 'dra_q_mlp_rollout', DeviceCartPoleVec, True
    NETWORK = "VanillaNet over a two-layer relu / tanh FCBody with a plain head"
    NOT_TASK = "the task is not a vector of at most 64 envs.CartPole environments under RescaleNormalizer(1.0), or there is no device"
    Net, IO, DIMS, ACTION_VIEW = Net, RolloutIO, ("state_dim", "n_actions", "hidden", "gate"), ()
    UPDATE, UPDATE_SWITCH, update_supported = 'dra_q_mlp_update', 'fused_nstep_update', staticmethod(update_supported)
    network_shape, fields, supported, why_not = staticmethod(shape), staticmethod(_fields), staticmethod(supported), staticmethod(why_not)

    def __init__(self, agent, shp):
        mlp_rollout.TargetRollout.__init__(self, agent, shp)
        self._up = None
        self.explore = self.random_action = None

    def attach(self):
        """The environments move to the device with the buffers these kernels leave (and the update's two outputs)."""
        self.agent.task = DeviceCartPoleVec(self.agent.task, buffers=lambda t_len, n, f: dict(
            q=f(t_len, n, 2), reward=f(t_len, n), mask=f(t_len, n), bootstrap=f(n), ret=f(t_len, n), loss=f(1)))

    def prepare(self, t_len):
        """Draws the rollout's exploration (support.plan_epsilon_greedy: NStepDQN_agent.py:34-35's calls in their order, so that
        np.random and the schedule end where the step-by-step loop leaves them) and stages it into the persistent device buffers
        the kernel reads (fixed addresses: graph replays see the new values).  -> (explore, random_action) as drawn."""
        cfg = self.agent.config
        n = self.agent.task.num_envs
        explore, rand = plan_epsilon_greedy(cfg.random_action_prob, t_len, n, self.shape[1], cfg.num_workers)
        o = t_len * n * 8       # one block, one copy: int64 random actions | uint8 explore flags
        if self._up is None or self.explore.shape[0] != t_len:
            self._up = StagedUpload(o + t_len * n, torch.uint8, Config.DEVICE)
            self.random_action = self._up.dev[:o].view(torch.int64).view(t_len, n)
            self.explore = self._up.dev[o:].view(t_len, n)
        raw = self._up.stage().numpy()
        raw[:o].view(np.int64).reshape(t_len, n)[...] = rand
        raw[o:].reshape(t_len, n)[...] = explore
        self._up.send()
        return explore, rand

    def fill_own(self, io):
        io.explore, io.random_action = self.explore.data_ptr(), self.random_action.data_ptr()

    def update(self, b, discount):
        """dra_q_mlp_update on the buffers run() left: the gradient lands in the optimiser's flat gradient buffer."""
        net = self.net_struct()
        update(net, b['state'], b['action'], b['reward'], b['mask'], b['bootstrap'], discount, self.agent._fused.flat.grad,
               b['ret'], b['loss'])
        return b['loss']
