"""Host side of csrc/oc_mlp.hip: option_critic_feature (examples.py:450-468) over device-resident cart-pole environments.

`shape(network)` says whether a network is one the kernels walk (OptionCriticNet over a two-layer FCBody of one width with a relu
or tanh gate and three plain biased heads of the right shapes); `why_not(agent)` adds the agent-side conditions and names the
first one that fails; `Rollout(agent)` builds the kernels' structs over the agent's flat parameter buffer and the TARGET network's
flat buffer of the same layout, stages the rollout's option epsilons (config.random_option_prob once per step, the reference's
calls in its order) and uniforms and launches a rollout (OptionCritic_agent.py:55-93: one launch instead of T x [forward, three
Categorical draws with their syncs, download, 5 environment steps, upload]); `update(...)` is OptionCritic_agent.py:95-116 with
the whole backward as one more launch.  The carried option state (prev_option, is_initial) lives in persistent device buffers the
rollout launch reads and replaces.

Random draws: one uniform_() [T, N, 3] per rollout on torch's device generator (before the captured region), turned into options
and actions by inverse CDF -- the documented deviation of pixel_rollout._OCRollout: inverse CDF of staged uniforms, not
Categorical.sample()'s own stream.

There is no CPU / eager implementation here: without the HIP library every call raises.
"""
import ctypes

import numpy as np
import torch

from . import mlp_rollout
from ._lib import lib, stream_ptr
from .device_env import DeviceCartPoleVec
from .mlp_rollout import GATES, body_params, fc_body, head_out, shape_table      # noqa: F401  (GATES: this module's public name)
from .support import Config, StagedUpload

_OFFSETS = ("w1", "b1", "w2", "b2", "wq", "bq", "wp", "bp", "wb", "bb")


class Net(ctypes.Structure):
    """Mirror of dra_oc_mlp_net (include/deeprl_amd.h)."""
    _fields_ = ([("param", ctypes.c_void_p), ("target", ctypes.c_void_p)] + [(k, ctypes.c_int32) for k in _OFFSETS] +
                [("gate", ctypes.c_int32), ("state_dim", ctypes.c_int32), ("n_actions", ctypes.c_int32),
                 ("hidden", ctypes.c_int32), ("n_options", ctypes.c_int32)])


class RolloutIO(ctypes.Structure):
    """Mirror of dra_oc_mlp_rollout_io."""
    _fields_ = ([(k, ctypes.c_void_p) for k in (
        "env_state", "env_counter", "ep_steps", "ep_return", "env_seed", "step_counter", "ep_count", "ep_ring", "eps", "uniform",
        "prev_option", "is_initial", "out_state", "out_q", "out_beta", "out_logits", "out_option", "out_prev_option", "out_action",
        "out_init", "out_log_pi_a", "out_entropy", "out_reward", "out_mask", "bootstrap")] +
        [("horizon", ctypes.c_int64), ("ring_cap", ctypes.c_int64), ("reward_coef", ctypes.c_double),
         ("t_len", ctypes.c_int32), ("n_env", ctypes.c_int32)])


class UpdateIO(ctypes.Structure):
    """Mirror of dra_oc_mlp_update_io."""
    _fields_ = ([(k, ctypes.c_void_p) for k in (
        "state", "q", "beta", "logits", "option", "prev_option", "action", "init", "log_pi_a", "entropy", "reward", "mask",
        "bootstrap", "eps", "grad", "out_ret", "out_adv", "out_beta_adv", "out_loss")] +
        [("discount", ctypes.c_double), ("termination_regularizer", ctypes.c_double), ("entropy_weight", ctypes.c_double),
         ("t_len", ctypes.c_int32), ("n_env", ctypes.c_int32)])


def shape(network):
    """(state_dim, n_actions, hidden, gate code, n_options) when `network` is an OptionCriticNet whose body is a two-layer FCBody
    of one width with a relu or tanh gate and whose fc_q [O, hidden], fc_pi [O * A, hidden] and fc_beta [O, hidden] are plain
    Linear layers with biases; else None."""
    from .nets import OptionCriticNet
    if type(network) is not OptionCriticNet:
        return None
    body = fc_body(network.body)
    if body is None or body[1] != body[2]:
        return None
    s_dim, hidden, _, gate = body
    n_opt, n_act = int(network.num_options), int(network.action_dim)
    heads = (network.fc_q, network.fc_pi, network.fc_beta)
    if any(getattr(h, 'fused_act', None) is not None for h in heads):
        return None
    if [head_out(h, hidden) for h in heads] != [n_opt, n_opt * n_act, n_opt]:
        return None
    return s_dim, n_act, hidden, gate, n_opt


supported = shape_table('dra_oc_mlp_supported')       # (state_dim, n_actions, hidden, n_env, gate, n_options): the rollout kernel
update_supported = shape_table('dra_oc_mlp_update_supported')     # (.., rows = rollout length x environments, gate, n_options)


def _fields(net):
    return list(zip(_OFFSETS, body_params(net.body) + [net.fc_q.weight, net.fc_q.bias, net.fc_pi.weight, net.fc_pi.bias,
                                                        net.fc_beta.weight, net.fc_beta.bias]))


def why_not(agent, supported_fn=supported):
    """None when OptionCriticAgent may run `agent` on the kernels, else the first reason it may not (all but the task itself,
    which DeviceCartPoleVec.eligible decides): mlp_rollout.why_not's -- opt-in: config.fused_oc_feature must be True --, the
    option count, then the target's shape and layout, then the update's rows."""
    shp = shape(agent.network)
    if shp is not None and Rollout.switched_on(agent.config) and not 2 <= shp[4] <= 8:
        return "%s is not built for %d option%s (2 to 8: the initial prev_options = ones must name one)" % (
            Rollout.ENTRY, shp[4], "" if shp[4] == 1 else "s")
    why = mlp_rollout.why_not(Rollout, agent, lambda s, a, h, n, g: supported_fn(s, a, h, n, g, shp[4]))
    if why is not None:
        return why
    return Rollout.target_why_not(agent, shp)


def update(net, b, eps, discount, termination_regularizer, entropy_weight, grad):
    """dra_oc_mlp_update on the current stream over the buffers `b` a rollout left (state [T, N, 4], q / beta [T, N, O], logits
    [T, N, 2], option / prev_option / action int64 [T, N], init / log_pi_a / entropy / reward / mask [T, N], bootstrap [N]) and eps
    [T]: ret / adv / beta_adv [T, N], loss [4] = (total, q_loss, pi_loss, beta_loss) and the gradient of pi_loss + q_loss +
    beta_loss with respect to the ten tensors `net` (a Net struct) names, written into the flat buffer `grad` at their offsets."""
    io = UpdateIO()
    for k in ("state", "q", "beta", "logits", "option", "prev_option", "action", "init", "log_pi_a", "entropy", "reward", "mask",
              "bootstrap"):
        setattr(io, k, b[k].data_ptr())
    io.eps, io.grad = eps.data_ptr(), grad.data_ptr()
    io.out_ret, io.out_adv, io.out_beta_adv, io.out_loss = (b[k].data_ptr() for k in ("ret", "adv", "beta_adv", "loss"))
    io.discount, io.termination_regularizer, io.entropy_weight = float(discount), float(termination_regularizer), float(entropy_weight)
    io.t_len, io.n_env = int(b['action'].shape[0]), int(b['action'].shape[1])
    lib.dra_oc_mlp_update(ctypes.byref(net), ctypes.byref(io), stream_ptr())


class Rollout(mlp_rollout.TargetRollout):
    """dra_oc_mlp_rollout over a DeviceCartPoleVec, the agent's flat parameter buffer and its target network's.  Random draws: one
    uniform_() [T, N, 3] per rollout on torch's device generator, turned into options and actions by inverse CDF -- the
    documented deviation of pixel_rollout._OCRollout: inverse CDF of staged uniforms, not Categorical.sample()'s own stream."""
    SWITCH, ENTRY, VEC, OPT_IN = 'fused_oc_feature', 'dra_oc_mlp_rollout', DeviceCartPoleVec, True
    NETWORK = "OptionCriticNet over a two-layer relu / tanh FCBody with three plain heads"
    NOT_TASK = "the task is not a vector of at most 64 envs.CartPole environments under RescaleNormalizer(1.0), or there is no device"
    Net, IO, DIMS, ACTION_VIEW = Net, RolloutIO, ("state_dim", "n_actions", "hidden", "gate", "n_options"), ()
    UPDATE, UPDATE_SWITCH, update_supported = 'dra_oc_mlp_update', 'fused_oc_update', staticmethod(update_supported)
    network_shape, fields, supported, why_not = staticmethod(shape), staticmethod(_fields), staticmethod(supported), staticmethod(why_not)

    def __init__(self, agent, shp):
        mlp_rollout.TargetRollout.__init__(self, agent, shp)
        self._eps_up = None
        self.eps = self.uniform = self.prev_option = self.is_initial = None

    def attach(self):
        """The environments move to the device with the buffers these kernels leave (and the update's outputs)."""
        n_opt = self.shape[4]
        i = lambda *s: torch.zeros(s, dtype=torch.int64, device=Config.DEVICE)
        self.agent.task = DeviceCartPoleVec(self.agent.task, buffers=lambda t_len, n, f: dict(
            q=f(t_len, n, n_opt), beta=f(t_len, n, n_opt), logits=f(t_len, n, 2), option=i(t_len, n), prev_option=i(t_len, n),
            init=f(t_len, n), log_pi_a=f(t_len, n), entropy=f(t_len, n), reward=f(t_len, n), mask=f(t_len, n), bootstrap=f(n),
            ret=f(t_len, n), adv=f(t_len, n), beta_adv=f(t_len, n), loss=f(4)))

    def state(self, n):
        """The carried option state (OptionCritic_agent.py:26-27: ones at the start): persistent device buffers."""
        dev = Config.DEVICE
        self.prev_option = torch.ones(n, dtype=torch.int64, device=dev)
        self.is_initial = torch.ones(n, dtype=torch.bool, device=dev)
        return self.prev_option, self.is_initial

    def prepare(self, t_len):
        """config.random_option_prob(num_workers) once per rollout step -- the reference's calls in its order -- staged into the
        persistent [T] buffer the kernel reads, and one uniform_() [T, N, 3] on torch's device generator into a persistent buffer
        (columns: fresh option, continued option, action).  Both run before the captured region and keep their addresses: graph
        replays see the new values.  -> the epsilons as drawn."""
        a = self.agent
        eps = np.asarray([a.config.random_option_prob(a.config.num_workers) for _ in range(t_len)], dtype=np.float64)
        if self._eps_up is None or self._eps_up.dev.shape[0] != t_len:
            self._eps_up = StagedUpload(t_len, torch.float32, Config.DEVICE)
            self.uniform = torch.empty((t_len, a.task.num_envs, 3), dtype=torch.float32, device=Config.DEVICE)
        self.eps = self._eps_up.put(eps)
        self.uniform.uniform_()
        return eps

    def fill_own(self, io):
        io.eps, io.uniform = self.eps.data_ptr(), self.uniform.data_ptr()
        io.prev_option, io.is_initial = self.prev_option.data_ptr(), self.is_initial.data_ptr()

    def update(self, b, cfg):
        """dra_oc_mlp_update on the buffers run() left: the gradient lands in the optimiser's flat gradient buffer.  -> loss [4]."""
        net = self.net_struct()
        update(net, b, self.eps, cfg.discount, cfg.termination_regularizer, cfg.entropy_weight, self.agent._fused.flat.grad)
        return b['loss']
