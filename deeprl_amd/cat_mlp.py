"""Host side of csrc/cat_mlp.hip: a2c_feature (examples.py:340-358) over device-resident cart-pole environments.

`shape(network)` says whether a network is one the rollout kernel walks (CategoricalActorCriticNet, a two-layer FCBody phi_body of
one width with a relu or tanh gate, identity actor / critic bodies, biased Linear heads); `why_not(agent)` adds the agent-side
conditions and names the first one that fails; `Rollout(agent)` builds the kernel's two structs over the agent's ONE flat
parameter buffer and launches a rollout (A2C_agent.py:22-41: one launch instead of T x [forward, sample, download the actions,
5 environment steps, upload]).  There is no CPU / eager implementation here: without the HIP library every call raises.
"""
import ctypes

import torch
import torch.nn.functional as F

from ._lib import lib, stream_ptr

GATES = {F.relu: 1, torch.relu: 1, torch.tanh: 2, F.tanh: 2}      # ops.ACT codes


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
    from .nets import CategoricalActorCriticNet, DummyBody, FCBody, Linear
    if type(network) is not CategoricalActorCriticNet:
        return None
    if type(network.actor_body) is not DummyBody or type(network.critic_body) is not DummyBody:
        return None
    b = network.phi_body
    if type(b) is not FCBody or b.noisy_linear or b.gate not in GATES or len(b.layers) != 2:
        return None
    if any(type(layer) is not Linear or layer.bias is None for layer in b.layers):
        return None
    hidden, s_dim = b.layers[0].weight.shape
    if tuple(b.layers[1].weight.shape) != (hidden, hidden):
        return None
    heads = (network.fc_action, network.fc_critic)
    if any(type(h) is not Linear or h.bias is None or h.fused_act is not None for h in heads):
        return None
    if network.fc_action.weight.shape[1] != hidden or tuple(network.fc_critic.weight.shape) != (1, hidden):
        return None
    return int(s_dim), int(network.fc_action.weight.shape[0]), int(hidden), GATES[b.gate]


def supported(state_dim, n_actions, hidden, n_env, gate):
    """dra_cat_mlp_supported: the shapes the rollout kernel is built for."""
    return lib.dra_cat_mlp_supported.raw(int(state_dim), int(n_actions), int(hidden), int(n_env), int(gate)) == 0


def _params(net):
    b = net.phi_body.layers
    return [b[0].weight, b[0].bias, b[1].weight, b[1].bias, net.fc_action.weight, net.fc_action.bias, net.fc_critic.weight,
            net.fc_critic.bias]


def why_not(agent, supported_fn=supported):
    """None when A2CAgent may run `agent` on the rollout kernel, else the first reason it may not (everything but the task
    itself, which device_env.DeviceCartPoleVec.eligible decides)."""
    cfg = agent.config
    if getattr(cfg, 'fused_a2c_cat', True) is False:
        return "config.fused_a2c_cat is off"
    if agent.dp.active:
        return "the agent is data parallel"
    if agent.grad_hook is not None:
        return "a grad_hook is installed"
    shp = shape(agent.network)
    if shp is None:
        return "the network is not CategoricalActorCriticNet over a two-layer relu / tanh FCBody with plain heads"
    flat = agent._fused.flat
    if any(all(p is not q for q in flat.params) for p in _params(agent.network)):
        return "one optimiser does not own every parameter the kernel reads"
    if not supported_fn(shp[0], shp[1], shp[2], int(cfg.num_workers), shp[3]):
        return "dra_cat_mlp_rollout is not built for state_dim %d, %d actions, hidden %d, %d environments" % (
            shp[0], shp[1], shp[2], int(cfg.num_workers))
    return None


def eligible(agent, supported_fn=supported):
    """The network shape when A2CAgent may move `agent.task` to the device (None: it keeps the host path)."""
    return shape(agent.network) if why_not(agent, supported_fn) is None else None


class Rollout:
    """dra_cat_mlp_rollout over a DeviceCartPoleVec and the agent's flat parameter buffer."""

    def __init__(self, agent, shp):
        self.agent = agent
        self.shape = shp
        self.launches = 0

    def net_struct(self):
        a = self.agent
        flat = a._fused.flat
        n = Net()
        n.param = flat.flat.data_ptr()
        n.w1, n.b1, n.w2, n.b2, n.wa, n.ba, n.wc, n.bc = [flat.offset_of(p) for p in _params(a.network)]
        n.state_dim, n.n_actions, n.hidden, n.gate = self.shape
        return n

    def run(self, t_len):
        """One rollout launch on the current stream; returns the task's buffers (state, action, v, reward, mask)."""
        a = self.agent
        task, dp = a.task, a.dp
        b = task.buffers(t_len)
        io = RolloutIO()
        io.env_state, io.env_counter, io.ep_steps = task.env_state.data_ptr(), task.env_counter.data_ptr(), task.ep_steps.data_ptr()
        io.ep_return, io.env_seed, io.sampler_step = task.ep_return.data_ptr(), task.env_seed.data_ptr(), dp.step_dev.data_ptr()
        io.ep_count, io.ep_ring = task.ep_count.data_ptr(), task.ep_ring.data_ptr()
        io.out_state, io.out_action, io.out_v = b['state'].data_ptr(), b['action'].data_ptr(), b['v'].data_ptr()
        io.out_reward, io.out_mask = b['reward'].data_ptr(), b['mask'].data_ptr()
        io.env0, io.n_global, io.noise_seed, io.horizon = dp.lo, dp.global_workers, a._noise_seed, task.horizon
        io.ring_cap, io.reward_coef = task.ring_cap, float(a.config.reward_normalizer.coef)
        io.t_len, io.n_env = int(t_len), task.num_envs
        net = self.net_struct()
        lib.dra_cat_mlp_rollout(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        self.launches += 1
        return b
