"""Host side of csrc/a2c_mlp.hip: a2c_continuous (examples.py:384-404) over device-resident synthetic environments.

`shape(network)` says whether a network is one the rollout kernel walks (GaussianActorCriticNet, identity phi_body, two
two-layer FCBody stacks of one width and one gate -- relu or tanh); `eligible(agent)` adds the agent-side conditions;
`Rollout(agent)` builds the kernel's two structs over the agent's ONE flat parameter buffer and launches a rollout
(A2C_agent.py:22-41: one launch instead of T x [normalise, forward, sample, 16 environment steps, upload]).
There is no CPU / eager implementation here: without the HIP library every call raises.
"""
import ctypes

import torch
import torch.nn.functional as F

from ._lib import lib, stream_ptr

GATES = {F.relu: 1, torch.relu: 1, torch.tanh: 2, F.tanh: 2}      # ops.ACT codes


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
    from .nets import DummyBody, FCBody, GaussianActorCriticNet, Linear
    if type(network) is not GaussianActorCriticNet or type(network.phi_body) is not DummyBody:
        return None
    bodies = (network.actor_body, network.critic_body)
    for b in bodies:
        if type(b) is not FCBody or b.noisy_linear or b.gate not in GATES or len(b.layers) != 2:
            return None
        if any(type(layer) is not Linear or layer.bias is None for layer in b.layers):
            return None
    a, c = bodies
    if GATES[a.gate] != GATES[c.gate]:
        return None
    s_dim, hidden = a.layers[0].weight.shape[1], a.layers[0].weight.shape[0]
    if not all(tuple(b.layers[0].weight.shape) == (hidden, s_dim) and tuple(b.layers[1].weight.shape) == (hidden, hidden)
               for b in bodies):
        return None
    heads = (network.fc_action, network.fc_critic)
    if any(type(h) is not Linear or h.bias is None for h in heads):
        return None
    if network.fc_action.weight.shape[1] != hidden or tuple(network.fc_critic.weight.shape) != (1, hidden):
        return None
    return int(s_dim), int(network.fc_action.weight.shape[0]), int(hidden), GATES[a.gate]


def supported(state_dim, action_dim, hidden, n_env, gate):
    """dra_a2c_mlp_supported: the shapes the rollout kernel is built for."""
    return lib.dra_a2c_mlp_supported.raw(int(state_dim), int(action_dim), int(hidden), int(n_env), int(gate)) == 0


def eligible(agent, supported_fn=supported):
    """The network shape when A2CAgent may move `agent.task` to the device (None: it keeps the host path).  Everything but
    the task itself (device_env.DeviceContinuousVec.eligible) is decided here."""
    cfg = agent.config
    if getattr(cfg, 'fused_a2c_mlp', True) is False or agent.dp.active or agent.grad_hook is not None:
        return None
    shp = shape(agent.network)
    if shp is None:
        return None
    flat = agent._fused.flat
    net = agent.network
    need = [l.weight for b in (net.actor_body, net.critic_body) for l in b.layers] + \
           [l.bias for b in (net.actor_body, net.critic_body) for l in b.layers] + \
           [net.fc_action.weight, net.fc_action.bias, net.fc_critic.weight, net.fc_critic.bias, net.std]
    if any(all(p is not q for q in flat.params) for p in need):      # one optimiser over every parameter the kernel reads
        return None
    if not supported_fn(shp[0], shp[1], shp[2], int(cfg.num_workers), shp[3]):
        return None
    return shp


class Rollout:
    """dra_a2c_mlp_rollout over a DeviceContinuousVec and the agent's flat parameter buffer."""

    def __init__(self, agent, shp):
        self.agent = agent
        self.shape = shp
        self.launches = 0

    def net_struct(self):
        a = self.agent
        net, flat = a.network, a._fused.flat
        n = Net()
        n.param = flat.flat.data_ptr()
        ab, cb = net.actor_body.layers, net.critic_body.layers
        off = flat.offset_of
        n.a_w1, n.a_b1, n.a_w2, n.a_b2 = off(ab[0].weight), off(ab[0].bias), off(ab[1].weight), off(ab[1].bias)
        n.a_w3, n.a_b3 = off(net.fc_action.weight), off(net.fc_action.bias)
        n.c_w1, n.c_b1, n.c_w2, n.c_b2 = off(cb[0].weight), off(cb[0].bias), off(cb[1].weight), off(cb[1].bias)
        n.c_w3, n.c_b3 = off(net.fc_critic.weight), off(net.fc_critic.bias)
        n.off_std = off(net.std)
        n.state_dim, n.action_dim, n.hidden, n.gate = self.shape
        return n

    def run(self, t_len, read_only):
        """One rollout launch on the current stream; returns the task's buffers (state, action, v, reward, mask)."""
        a = self.agent
        task, dp, config = a.task, a.dp, a.config
        b = task.buffers(t_len)
        io = RolloutIO()
        io.env_state, io.env_counter, io.env_seed = task.env_state.data_ptr(), task.env_counter.data_ptr(), task.env_seed.data_ptr()
        io.rms, io.cur_state, io.sampler_step = task.rms.data_ptr(), task.cur_state.data_ptr(), dp.step_dev.data_ptr()
        io.out_state, io.out_action, io.out_v = b['state'].data_ptr(), b['action'].data_ptr(), b['v'].data_ptr()
        io.out_reward, io.out_mask = b['reward'].data_ptr(), b['mask'].data_ptr()
        io.env0, io.n_global, io.noise_seed, io.horizon = dp.lo, dp.global_workers, a._noise_seed, task.horizon
        io.reward_coef, io.rms_epsilon, io.rms_clip = float(config.reward_normalizer.coef), task.rms_epsilon, task.rms_clip
        io.rms_update = 1 if (task.rms_kind == 'meanstd' and not read_only) else 0
        io.t_len, io.n_env = int(t_len), task.num_envs
        net = self.net_struct()
        lib.dra_a2c_mlp_rollout(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        self.launches += 1
        return b

