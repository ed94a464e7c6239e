"""Host side of csrc/a2c_mlp.hip: a2c_continuous (examples.py:384-404) over device-resident synthetic environments.

`shape(network)` says whether a network is one the rollout kernel walks (GaussianActorCriticNet, identity phi_body, two
two-layer FCBody stacks of one width and one gate -- relu or tanh); `eligible(agent)` adds the agent-side conditions;
`Rollout(agent)` builds the kernel's two structs over the agent's ONE flat parameter buffer and launches a rollout
(A2C_agent.py:22-41: one launch instead of T x [normalise, forward, sample, 16 environment steps, upload]).
There is no CPU / eager implementation here: without the HIP library every call raises.
"""
import ctypes

import torch

from . import mlp_rollout
from .device_env import DeviceContinuousVec
from .mlp_rollout import GATES, body_params, fc_body, head_out, shape_table      # noqa: F401  (GATES: this module's public name)
from .support import Config


class Net(ctypes.Structure):
    """Mirror of dra_a2c_mlp_net (include/deeprl_amd.h)."""
    _fields_ = [("param", ctypes.c_void_p),
                ("a_w1", ctypes.c_int32), ("a_b1", ctypes.c_int32), ("a_w2", ctypes.c_int32), ("a_b2", ctypes.c_int32),
                ("a_w3", ctypes.c_int32), ("a_b3", ctypes.c_int32),
                ("c_w1", ctypes.c_int32), ("c_b1", ctypes.c_int32), ("c_w2", ctypes.c_int32), ("c_b2", ctypes.c_int32),
                ("c_w3", ctypes.c_int32), ("c_b3", ctypes.c_int32),
                ("off_std", ctypes.c_int32), ("gate", ctypes.c_int32),
                ("state_dim", ctypes.c_int32), ("action_dim", ctypes.c_int32), ("hidden", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class RolloutIO(ctypes.Structure):
    """Mirror of dra_a2c_mlp_rollout_io."""
    _fields_ = [("env_state", ctypes.c_void_p), ("env_counter", ctypes.c_void_p), ("env_seed", ctypes.c_void_p),
                ("rms", ctypes.c_void_p), ("cur_state", ctypes.c_void_p), ("sampler_step", ctypes.c_void_p),
                ("out_state", ctypes.c_void_p), ("out_action", ctypes.c_void_p), ("out_v", ctypes.c_void_p),
                ("out_reward", ctypes.c_void_p), ("out_mask", ctypes.c_void_p),
                ("env0", ctypes.c_int64), ("n_global", ctypes.c_int64), ("noise_seed", ctypes.c_uint64),
                ("horizon", ctypes.c_int64), ("reward_coef", ctypes.c_double), ("rms_epsilon", ctypes.c_double),
                ("rms_clip", ctypes.c_double), ("rms_update", ctypes.c_int32), ("t_len", ctypes.c_int32),
                ("n_env", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def shape(network):
    """(state_dim, action_dim, hidden, gate code) when `network` is a GaussianActorCriticNet whose phi_body is the identity and
    whose actor / critic bodies are two-layer FCBody stacks of one width with the same relu or tanh gate, plain Linear layers
    with biases; else None."""
    from .nets import DummyBody, GaussianActorCriticNet
    if type(network) is not GaussianActorCriticNet or type(network.phi_body) is not DummyBody:
        return None
    actor, critic = fc_body(network.actor_body), fc_body(network.critic_body)
    if actor is None or actor != critic or actor[1] != actor[2]:
        return None
    s_dim, hidden, _, gate = actor
    a_dim = head_out(network.fc_action, hidden)
    if a_dim is None or head_out(network.fc_critic, hidden) != 1:
        return None
    return s_dim, a_dim, hidden, gate


supported = shape_table('dra_a2c_mlp_supported')      # (state_dim, action_dim, hidden, n_env, gate): the rollout kernel


def _fields(net):
    a, c = body_params(net.actor_body), body_params(net.critic_body)
    return list(zip(("a_w1", "a_b1", "a_w2", "a_b2", "a_w3", "a_b3", "c_w1", "c_b1", "c_w2", "c_b2", "c_w3", "c_b3", "off_std"),
                    a + [net.fc_action.weight, net.fc_action.bias] + c + [net.fc_critic.weight, net.fc_critic.bias, net.std]))


def eligible(agent, supported_fn=supported):
    """The network shape when A2CAgent may move `agent.task` to the device (None: it keeps the host path, silently).  Everything
    but the task itself (device_env.DeviceContinuousVec.eligible) is decided here."""
    return shape(agent.network) if mlp_rollout.why_not(Rollout, agent, supported_fn) is None else None


class Rollout(mlp_rollout.Rollout):
    """dra_a2c_mlp_rollout over a DeviceContinuousVec and the agent's flat parameter buffer."""
    SWITCH, ENTRY, VEC = 'fused_a2c_mlp', 'dra_a2c_mlp_rollout', DeviceContinuousVec
    NETWORK = "GaussianActorCriticNet over two two-layer relu / tanh FCBody stacks of one width with plain heads"
    Net, IO, DIMS, ACTION_VIEW = Net, RolloutIO, ("state_dim", "action_dim", "hidden", "gate"), (-1,)
    network_shape, fields, supported = staticmethod(shape), staticmethod(_fields), staticmethod(supported)

    def attach(self):
        """Observations, counters and the observation statistics move to the device; the update's Gaussian head becomes one
        kernel each way."""
        a = self.agent
        a.task = DeviceContinuousVec(a.task, a.states, a.config.state_normalizer)
        a.network.fused_gauss_head = True

    def begin_step(self, t_len):
        """Episode reporting: rewards and terminals are hashes of the counters, so the host's shadow of them knows the episodes
        that end inside this rollout before it is launched (BaseAgent.record_online_return at the step the episode ended)."""
        a = self.agent
        events = a.task.shadow(t_len)
        if a.dp.step_dev is None:
            a.dp.step_dev = torch.zeros(1, dtype=torch.int64, device=Config.DEVICE)
        for t, i, ret in events:
            a.log_train_return(ret, a.total_steps + t * a.dp.global_workers + i)

    def signature(self):
        """What the captured launch has baked in besides the optimizer's hyper-parameters (graphs._OnPolicyGraph's own key): whether the
        normaliser's statistics are left alone (fill_io's read_only), and the seed of the noise stream."""
        return bool(getattr(self.agent.config.state_normalizer, 'read_only', False)), int(self.agent._noise_seed)
