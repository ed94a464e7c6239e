"""Host side of csrc/cat_mlp.hip: a2c_feature (examples.py:340-358) over device-resident cart-pole environments.

`shape(network)` says whether a network is one the rollout kernel walks (CategoricalActorCriticNet, a two-layer FCBody phi_body of
one width with a relu or tanh gate, identity actor / critic bodies, biased Linear heads); `why_not(agent)` adds the agent-side
conditions and names the first one that fails; `Rollout(agent)` builds the kernel's two structs over the agent's ONE flat
parameter buffer and launches a rollout (A2C_agent.py:22-41: one launch instead of T x [forward, sample, download the actions,
5 environment steps, upload]).  There is no CPU / eager implementation here: without the HIP library every call raises.
"""
import ctypes

import torch

from . import mlp_rollout
from .device_env import DeviceCartPoleVec
from .mlp_rollout import GATES, body_params, fc_body, head_out, shape_table      # noqa: F401  (GATES: this module's public name)
from .support import Config


class Net(ctypes.Structure):
    """Mirror of dra_cat_mlp_net (include/deeprl_amd.h)."""
    _fields_ = [("param", ctypes.c_void_p),
                ("w1", ctypes.c_int32), ("b1", ctypes.c_int32), ("w2", ctypes.c_int32), ("b2", ctypes.c_int32),
                ("wa", ctypes.c_int32), ("ba", ctypes.c_int32), ("wc", ctypes.c_int32), ("bc", ctypes.c_int32),
                ("gate", ctypes.c_int32), ("state_dim", ctypes.c_int32), ("n_actions", ctypes.c_int32),
                ("hidden", ctypes.c_int32)]


class RolloutIO(ctypes.Structure):
    """Mirror of dra_cat_mlp_rollout_io."""
    _fields_ = [("env_state", ctypes.c_void_p), ("env_counter", ctypes.c_void_p), ("ep_steps", ctypes.c_void_p),
                ("ep_return", ctypes.c_void_p), ("env_seed", ctypes.c_void_p), ("sampler_step", ctypes.c_void_p),
                ("ep_count", ctypes.c_void_p), ("ep_ring", ctypes.c_void_p),
                ("out_state", ctypes.c_void_p), ("out_action", ctypes.c_void_p), ("out_v", ctypes.c_void_p),
                ("out_reward", ctypes.c_void_p), ("out_mask", ctypes.c_void_p),
                ("env0", ctypes.c_int64), ("n_global", ctypes.c_int64), ("noise_seed", ctypes.c_uint64),
                ("horizon", ctypes.c_int64), ("ring_cap", ctypes.c_int64), ("reward_coef", ctypes.c_double),
                ("t_len", ctypes.c_int32), ("n_env", ctypes.c_int32)]


def shape(network):
    """(state_dim, n_actions, hidden, gate code) when `network` is a CategoricalActorCriticNet whose phi_body is a two-layer FCBody
    of one width with a relu or tanh gate, whose actor / critic bodies are identities and whose heads are plain Linear layers
    with biases; else None."""
    from .nets import CategoricalActorCriticNet, DummyBody
    if type(network) is not CategoricalActorCriticNet:
        return None
    if type(network.actor_body) is not DummyBody or type(network.critic_body) is not DummyBody:
        return None
    body = fc_body(network.phi_body)
    if body is None or body[1] != body[2]:
        return None
    s_dim, hidden, _, gate = body
    n_actions = head_out(network.fc_action, hidden)
    if n_actions is None or head_out(network.fc_critic, hidden) != 1:
        return None
    if network.fc_action.fused_act is not None or network.fc_critic.fused_act is not None:
        return None
    return s_dim, n_actions, hidden, gate


supported = shape_table('dra_cat_mlp_supported')      # (state_dim, n_actions, hidden, n_env, gate): the rollout kernel


def _fields(net):
    return list(zip(("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc"),
                    body_params(net.phi_body) + [net.fc_action.weight, net.fc_action.bias, net.fc_critic.weight, net.fc_critic.bias]))


def why_not(agent, supported_fn=supported):
    """None when A2CAgent may run `agent` on the rollout kernel, else the first reason it may not (everything but the task
    itself, which device_env.DeviceCartPoleVec.eligible decides)."""
    return mlp_rollout.why_not(Rollout, agent, supported_fn)


def eligible(agent, supported_fn=supported):
    """The network shape when A2CAgent may move `agent.task` to the device (None: it keeps the host path)."""
    return shape(agent.network) if why_not(agent, supported_fn) is None else None


class Rollout(mlp_rollout.Rollout):
    """dra_cat_mlp_rollout over a DeviceCartPoleVec and the agent's flat parameter buffer."""
    SWITCH, ENTRY, VEC = 'fused_a2c_cat', 'dra_cat_mlp_rollout', DeviceCartPoleVec
    NETWORK = "CategoricalActorCriticNet over a two-layer relu / tanh FCBody with plain heads"
    Net, IO, DIMS, ACTION_VIEW = Net, RolloutIO, ("state_dim", "n_actions", "hidden", "gate"), ()
    network_shape, fields, supported = staticmethod(shape), staticmethod(_fields), staticmethod(supported)

    def attach(self):
        """The environments move to the device; episode ends come back through the device's episode ring."""
        mlp_rollout.Rollout.attach(self)
        a = self.agent
        if a.dp.step_dev is None:      # the rank-invariant sampler's position: the kernel reads and advances it
            a.dp.step_dev = torch.zeros(1, dtype=torch.int64, device=Config.DEVICE)
        a._episodes.stamp = int(a.dp.step_dev.item())

    def begin_step(self, t_len):
        """Episode reporting: the terminals depend on the actions, so episode ends come back through the device's ring (EpisodeRing)."""
        self.agent._episodes.begin(t_len)

    def signature(self):
        """What the captured launch has baked in besides the optimizer's hyper-parameters: the seed of the noise stream."""
        return (int(self.agent._noise_seed),)

    def end_step(self):
        self.agent._episodes.end()
