"""Host side of csrc/dist_mlp.hip: categorical_dqn_feature (examples.py:164-193) and quantile_regression_dqn_feature
(examples.py:101-127) over ONE device-resident cart-pole environment and the HBM replay ring.

The agent step is dqn_mlp.Step's, as it is (the draws in the reference's order staged in one block, one acting launch, one update
launch, the fused clip + optimizer step, both replayed from captured graphs, the target copy between replays); this module brings
what tells the two distributional entries from dqn_feature: `shape(network)` (CategoricalNet / QuantileNet over a two-layer FCBody
of one width with a relu or tanh gate and a plain biased head), `why_not(agent)` (dqn_mlp.why_not's list for the two agent classes
under config.fused_dist_feature), the structs and the two launches.  config.fused_dist_update False keeps the device acting and
ring and runs ring.gather plus the agent's own _loss_grad (the modules, ops.c51_loss / ops.qr_loss, autograd) on the same
indices; True runs dra_dist_mlp_update; unset, each head kind takes the form that measured faster (Kind.fused_update: the kernel
for quantiles, the module form for the categorical head).  There is no CPU / eager-PyTorch implementation here: without the HIP library every call raises.
"""
import ctypes

import torch

from . import dqn_mlp
from .mlp_rollout import body_params, fc_body, head_out, shape_table

SWITCH = 'fused_dist_feature'
NETWORK = "CategoricalNet / QuantileNet over a two-layer relu / tanh FCBody with a plain head"
CATEGORICAL, QUANTILE = 1, 2
MAX_K, MAX_B, MAX_ATOMS = 8, 256, 51


class Net(ctypes.Structure):
    """Mirror of dra_dist_mlp_net (include/deeprl_amd.h)."""
    _fields_ = [("param", ctypes.c_void_p), ("target", ctypes.c_void_p),
                ("w1", ctypes.c_int32), ("b1", ctypes.c_int32), ("w2", ctypes.c_int32), ("b2", ctypes.c_int32),
                ("wq", ctypes.c_int32), ("bq", ctypes.c_int32),
                ("gate", ctypes.c_int32), ("state_dim", ctypes.c_int32), ("n_actions", ctypes.c_int32),
                ("hidden", ctypes.c_int32), ("head", ctypes.c_int32), ("n_atoms", ctypes.c_int32),
                ("v_min", ctypes.c_double), ("v_max", ctypes.c_double)]


ActIO = dqn_mlp.ActIO       # the acting launch's io is dra_dqn_mlp_act_io as it is


class UpdateIO(ctypes.Structure):
    """Mirror of dra_dist_mlp_update_io."""
    _fields_ = [("ring_frames", ctypes.c_void_p), ("ring_actions", ctypes.c_void_p), ("ring_rewards", ctypes.c_void_p),
                ("ring_masks", ctypes.c_void_p), ("idx", ctypes.c_void_p), ("grad", ctypes.c_void_p),
                ("out_loss", ctypes.c_void_p), ("out_loss_vec", ctypes.c_void_p), ("out_q_next", ctypes.c_void_p),
                ("out_target", ctypes.c_void_p), ("err", ctypes.c_void_p), ("capacity", ctypes.c_int64),
                ("discount", ctypes.c_double), ("batch", ctypes.c_int32), ("double_q", ctypes.c_int32)]


def _head_layer(network):
    from .nets import CategoricalNet, QuantileNet
    if type(network) is CategoricalNet:
        return CATEGORICAL, network.fc_categorical, int(network.num_atoms)
    if type(network) is QuantileNet:
        return QUANTILE, network.fc_quantiles, int(network.num_quantiles)
    return None


def shape(network):
    """(state_dim, n_actions, hidden, gate code, head kind, atoms per action) when `network` is a CategoricalNet or a QuantileNet
    whose body is a two-layer FCBody of one width with a relu or tanh gate and whose head is a plain Linear layer with a bias of
    n_actions x atoms outputs; else None."""
    found = _head_layer(network)
    if found is None:
        return None
    kind, layer, n = found
    body = fc_body(network.body)
    if body is None or body[1] != body[2]:
        return None
    s_dim, hidden, _, gate = body
    out = head_out(layer, hidden)
    n_actions = int(network.action_dim)
    if out is None or layer.fused_act is not None or n < 1 or out != n_actions * n:
        return None
    return s_dim, n_actions, hidden, gate, kind, n


def _fields(net):
    layer = _head_layer(net)[1]
    return list(zip(("w1", "b1", "w2", "b2", "wq", "bq"), body_params(net.body) + [layer.weight, layer.bias]))


# (state_dim, n_actions, hidden, t_len = transitions per launch | batch, gate, head, n_atoms); the update's: what fits its workgroup's LDS
supported = shape_table('dra_dist_mlp_supported')
update_supported = shape_table('dra_dist_mlp_update_supported')


def support(config, head):
    """(v_min, v_max) the kernels are told: the categorical support, (0, 0) for quantiles."""
    if head == CATEGORICAL:
        return float(config.categorical_v_min), float(config.categorical_v_max)
    return 0.0, 0.0


class Kind(dqn_mlp.Kind):
    """dqn_mlp.Kind for the two distributional entries."""
    ENTRY, SWITCH, UPDATE_SWITCH = 'dist_feature', SWITCH, 'fused_dist_update'
    AGENTS = ('CategoricalDQNAgent', 'QuantileRegressionDQNAgent')
    NOT_AGENT = "the agent is a %s, not a CategoricalDQNAgent or a QuantileRegressionDQNAgent"
    NETWORK, ACT, UPDATE, N_SUPPORTED = NETWORK, 'dra_dist_mlp_act', 'dra_dist_mlp_update', 6
    EVAL = 'dra_dist_mlp_eval'
    # examples.py leaves config.async_actor at the Config's default (True) in both entries, and for these two agents it is a no-op on
    # the host path (agents.py's module docstring): the Step keeps that path's order, so the field does not decide anything here
    ASYNC_ACTOR = True
    Net, DIMS = Net, ("state_dim", "n_actions", "hidden", "gate", "head", "n_atoms")
    shape, fields = staticmethod(shape), staticmethod(_fields)
    supported, update_supported = staticmethod(supported), staticmethod(update_supported)

    @classmethod
    def fused_update(cls, cfg, shp):
        """config.fused_dist_update when it is set; unset, the measured faster form per head kind: the update
        kernel for quantiles, ring.gather plus the modules and ops.c51_loss for the categorical head."""
        want = getattr(cfg, cls.UPDATE_SWITCH, None)
        return shp[4] == QUANTILE if want is None else want is not False

    @staticmethod
    def extra(agent, shp):
        cfg = agent.config
        categorical = type(agent).__name__ == 'CategoricalDQNAgent'
        if (shp[4] == CATEGORICAL) != categorical:
            return "the network's head is not the agent's (%s)" % ("categorical" if categorical else "quantiles")
        n = int(cfg.categorical_n_atoms if categorical else cfg.num_quantiles)
        if n != shp[5]:
            return "the network has %d atoms per action, the configuration %d" % (shp[5], n)
        if categorical and not float(cfg.categorical_v_max) > float(cfg.categorical_v_min):
            return "categorical_v_max is not above categorical_v_min"
        return None


def why_not(agent, supported_fn=None, update_supported_fn=None):
    """None when `agent` (a CategoricalDQNAgent or a QuantileRegressionDQNAgent) may run on the kernels, else the first reason
    it may not: dqn_mlp.why_not's list under this module's switch, agent classes and shapes, without its
    async_actor condition (Kind.ASYNC_ACTOR says why) (a PrioritizedReplay is refused for
    both: QR-DQN has no valid PER configuration in the reference, and the categorical kernel applies no importance weights)."""
    return dqn_mlp.why_not(agent, supported_fn, update_supported_fn, kind=Kind)


class Step(dqn_mlp.Step):
    """dqn_mlp.Step over the distributional kernels: the net struct's support, the update's io and its output buffers are this
    class's; the two launches (by Kind.ACT / Kind.UPDATE), the module-path update, prepare, step, the captured regions, check,
    drain and the state dict are the parent's."""
    KIND = Kind

    def make_outputs(self, dev):
        n, head = self.shape[5], self.shape[4]
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.loss, self.loss_vec = f(1), f(self.batch if head == CATEGORICAL else n)
        self.q_next, self.target = f(self.batch, 2), f(self.batch, n)

    def net_struct(self):
        n = dqn_mlp.Step.net_struct(self)
        n.v_min, n.v_max = support(self.agent.config, n.head)
        return n

    def update(self):
        """dra_dist_mlp_update on the staged indices: the gradient lands in the optimiser's flat gradient buffer."""
        io = UpdateIO()
        io.out_loss, io.out_loss_vec = self.loss.data_ptr(), self.loss_vec.data_ptr()
        io.out_q_next, io.out_target = self.q_next.data_ptr(), self.target.data_ptr()
        return self.launch_update(io)


def adopt(agent):
    """A Step with the actor's environment on the device when configuration, agent and task allow it; else None (the host path;
    with the switch on the reason is logged once)."""
    return dqn_mlp.adopt(agent, Step)
