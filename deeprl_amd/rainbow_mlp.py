"""Host side of csrc/rainbow_mlp.hip: the two launches of rainbow_feature (examples.py:231-280) over ONE device-resident cart-pole
environment and the HBM replay ring -- dra_rainbow_mlp_act (sgd_update_frequency transitions, transition k under noise row k of a
`_NoiseBlock.draw_rows` block) and dra_rainbow_mlp_update (the n-step gather, the target network under its noise, the online
network under one draw, double_q, the projection, the KL, priorities and importance weights, the gradient of all sixteen tensors
into the optimiser's flat gradient buffer).

This module brings the struct mirrors, the shape tables, `shape(network)` (RainbowNet over a two-layer noisy FCBody of one width
with a relu or tanh gate and two NoisyLinear heads), `fill_layers` (the sixteen parameter offsets and the twelve noise offsets of a
net struct), `why_not(agent)` (dqn_mlp.why_not's list under config.fused_rainbow_feature for a CategoricalDQNAgent over a
PrioritizedReplay with an n-step window and noisy layers) and `Step`, dqn_mlp.Step over the two launches: the host makes the step's
draws in the host path's order -- np.random as epsilon_greedy(0, q) consumes it per transition, the K noise rows
(`_NoiseBlock.draw_rows`), the tree's adds (`PrioritizedReplay.advance`), and past exploration_steps the prioritised draw (python
`random`, the descent on the device, ONE host wait, validity / padding / pending marks on the host), the target's and the online
network's reset_noise() and beta -- and stages them in one block; the acting launch, the update launch
(config.fused_rainbow_update False: ring.gather and the agent's own _loss_grad on the same staged words) and the fused clip +
optimizer step replay from captured graphs; the priorities' commit (its leaf list is gated on the host) and the target copy run
eagerly between replays.  There is no CPU / eager-PyTorch implementation here: without the HIP library every call
raises.
"""
import ctypes

import numpy as np
import torch

from . import dqn_mlp
from ._lib import lib, stream_ptr
from .mlp_rollout import GATES, shape_table

SWITCH = 'fused_rainbow_feature'

NETWORK = "RainbowNet over a two-layer relu / tanh FCBody(noisy_linear=True) with NoisyLinear heads"
MAX_K, MAX_B, MAX_ATOMS, MAX_N_STEP = 8, 64, 51, 8
LAYERS = ("l1", "l2", "value", "advantage")                                       # the net struct's layer fields, in its order
PARAMS = ("weight_mu", "weight_sigma", "bias_mu", "bias_sigma")                   # NoisyLinear's parameters, in Layer's order
NOISE = ("noise_in", "noise_out_weight", "noise_out_bias")                        # its raw noise vectors, in Layer's order


class Layer(ctypes.Structure):
    """Mirror of dra_rainbow_mlp_layer (include/deeprl_amd.h)."""
    _fields_ = [("w_mu", ctypes.c_int32), ("w_sigma", ctypes.c_int32), ("b_mu", ctypes.c_int32), ("b_sigma", ctypes.c_int32),
                ("e_in", ctypes.c_int32), ("e_out", ctypes.c_int32), ("e_b", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Net(ctypes.Structure):
    """Mirror of dra_rainbow_mlp_net."""
    _fields_ = [("param", ctypes.c_void_p), ("target", ctypes.c_void_p), ("noise", ctypes.c_void_p),
                ("target_noise", ctypes.c_void_p),
                ("l1", Layer), ("l2", Layer), ("value", Layer), ("advantage", Layer),
                ("noise_stride", ctypes.c_int32), ("gate", ctypes.c_int32), ("state_dim", ctypes.c_int32),
                ("n_actions", ctypes.c_int32), ("hidden", ctypes.c_int32), ("n_atoms", ctypes.c_int32),
                ("v_min", ctypes.c_double), ("v_max", ctypes.c_double)]


ActIO = dqn_mlp.ActIO       # the acting launch's io is dra_dqn_mlp_act_io as it is


class UpdateIO(ctypes.Structure):
    """Mirror of dra_rainbow_mlp_update_io."""
    _fields_ = [("ring_frames", ctypes.c_void_p), ("ring_actions", ctypes.c_void_p), ("ring_rewards", ctypes.c_void_p),
                ("ring_masks", ctypes.c_void_p), ("idx", ctypes.c_void_p), ("prob", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("grad", ctypes.c_void_p), ("out_loss", ctypes.c_void_p), ("out_loss_vec", ctypes.c_void_p),
                ("out_prio", ctypes.c_void_p), ("out_weights", ctypes.c_void_p), ("out_q_next", ctypes.c_void_p),
                ("out_target", ctypes.c_void_p), ("err", ctypes.c_void_p), ("capacity", ctypes.c_int64),
                ("discount", ctypes.c_double), ("step_discount", ctypes.c_double), ("replay_eps", ctypes.c_double),
                ("replay_alpha", ctypes.c_double), ("batch", ctypes.c_int32), ("double_q", ctypes.c_int32),
                ("n_step", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# (state_dim, n_actions, hidden, t_len = transitions per launch, gate, n_atoms) / (..., batch, gate, n_atoms, n_step): the update's is
# what fits its workgroup's LDS -- batches of at most MAX_B rows
supported = shape_table('dra_rainbow_mlp_supported')
update_supported = shape_table('dra_rainbow_mlp_update_supported')


def noisy_layers(network):
    """[(struct field, NoisyLinear)] in the net struct's order (NOT the draw order, which is RainbowNet.noisy_layers()'s), or None
    when `network` is not a RainbowNet whose two body layers and two heads are NoisyLinear."""
    from .nets import FCBody, NoisyLinear, RainbowNet
    if type(network) is not RainbowNet or not network.noisy_linear:
        return None
    body = network.body
    if type(body) is not FCBody or not body.noisy_linear or len(body.layers) != 2:
        return None
    found = list(zip(LAYERS, (body.layers[0], body.layers[1], network.fc_value, network.fc_advantage)))
    return found if all(type(m) is NoisyLinear for _, m in found) else None


def shape(network):
    """(state_dim, n_actions, hidden, gate code, atoms per action) when `network` is a RainbowNet over a two-layer noisy FCBody of
    one width with a relu or tanh gate whose heads have num_atoms and action_dim x num_atoms outputs over that width; else None."""
    found = noisy_layers(network)
    if found is None or network.body.gate not in GATES:
        return None
    l1, l2, value, adv = (m for _, m in found)
    hidden, n, n_actions = int(l1.out_features), int(network.num_atoms), int(network.action_dim)
    if (l2.in_features, l2.out_features, value.in_features, adv.in_features) != (hidden,) * 4:
        return None
    if n < 1 or int(value.out_features) != n or int(adv.out_features) != n_actions * n:
        return None
    return int(l1.in_features), n_actions, hidden, GATES[network.body.gate], n


def noise_names(network):
    """{struct field: the layer's name in RainbowNet.noisy_layers() / _NoiseBlock.slices}."""
    return dict(zip(LAYERS, ('body.layers.0', 'body.layers.1', 'fc_value', 'fc_advantage')))


def fill_layers(net, network, offset_of, noise_slices):
    """Fills the four Layer structs of `net`: offset_of(parameter) -> its float offset in the flat parameter buffer,
    noise_slices[(layer name, buffer name)] -> (offset, length) in a noise row (_NoiseBlock.slices).  -> net"""
    names = noise_names(network)
    for field, m in noisy_layers(network):
        layer = getattr(net, field)
        for dst, p in zip(("w_mu", "w_sigma", "b_mu", "b_sigma"), PARAMS):
            setattr(layer, dst, int(offset_of(getattr(m, p))))
        for dst, b in zip(("e_in", "e_out", "e_b"), NOISE):
            setattr(layer, dst, int(noise_slices[(names[field], b)][0]))
    return net


def _fields(network):
    """[(name, parameter)] of the sixteen tensors (the names serve the ownership and layout checks; fill_layers fills the struct)."""
    return [("%s.%s" % (field, p), getattr(m, p)) for field, m in noisy_layers(network) for p in PARAMS]


class Kind(dqn_mlp.Kind):
    """dqn_mlp.Kind for rainbow_feature."""
    ENTRY, SWITCH, UPDATE_SWITCH = 'rainbow_feature', SWITCH, 'fused_rainbow_update'
    AGENTS, NOT_AGENT = ('CategoricalDQNAgent',), "the agent is a %s, not a CategoricalDQNAgent"
    NETWORK, ACT, UPDATE, N_SUPPORTED = NETWORK, 'dra_rainbow_mlp_act', 'dra_rainbow_mlp_update', 5
    EVAL = 'dra_rainbow_mlp_eval'
    ASYNC_ACTOR = True       # (the entry sets it; for this agent class it is a no-op on the host path: dist_mlp.Kind)
    PRIORITIZED, MAX_N_STEP, NOISY = True, MAX_N_STEP, True
    Net, DIMS = Net, ("state_dim", "n_actions", "hidden", "gate", "n_atoms")
    shape, fields = staticmethod(shape), staticmethod(_fields)
    supported = staticmethod(supported)
    # (dqn_mlp.why_not knows no window: extra() asks the table again with the replay's n_step)
    update_supported = staticmethod(lambda *dims: update_supported(*dims, 1))

    @staticmethod
    def eval_net(agent, net):
        """Evaluation runs under the ONLINE network's own noise buffers (its last reset_noise()), as ONE row: what the host's
        eval_step sees through self.network(state), and what the update launch reads."""
        net.noise = agent.network.noise_block().flat.data_ptr()
        return net

    @staticmethod
    def extra(agent, shp):
        cfg, rp = agent.config, agent._inner_replay()
        if int(cfg.categorical_n_atoms) != shp[4]:
            return "the network has %d atoms per action, the configuration %d" % (shp[4], int(cfg.categorical_n_atoms))
        if not float(cfg.categorical_v_max) > float(cfg.categorical_v_min):
            return "categorical_v_max is not above categorical_v_min"
        if int(rp.memory_size) < int(cfg.sgd_update_frequency) + int(rp.n_step) + 1:
            return "the replay holds fewer slots than an agent step and an n-step window need"
        if float(rp.discount) != float(cfg.discount):
            return "the replay's discount is not the configuration's"
        for net in (agent.network, agent.target_network):
            if not net.fused_noisy or not net.noise_block().intact():
                return "a network's noise vectors are not the views of its noise block"
        # the kernel's own table on the real window (dqn_mlp.why_not asks it with a window of 1)
        b, n_step = int(rp.batch_size), int(rp.n_step)
        if Kind.fused_update(cfg, shp) and not update_supported(shp[0], shp[1], shp[2], b, shp[3], shp[4], n_step):
            return "%s is not built for minibatches of %d over an n-step window of %d" % (Kind.UPDATE, b, n_step)
        return None


def why_not(agent, supported_fn=None, update_supported_fn=None):
    """None when `agent` (a CategoricalDQNAgent on rainbow_feature's kind of configuration) may run on the kernels, else the first
    reason it may not: dqn_mlp.why_not's list under this module's switch with a PrioritizedReplay, an n-step window of at most
    MAX_N_STEP and noisy layers REQUIRED where the siblings refuse them."""
    return dqn_mlp.why_not(agent, supported_fn, update_supported_fn, kind=Kind)


class Step(dqn_mlp.Step):
    """dqn_mlp.Step over the rainbow kernels: see the module's docstring.  The staged block, prepare, the net struct, the update's
    io and outputs and the commit behind the learn region are this class's; act, step, the captured regions, check, drain and the
    state dict are the parent's."""
    KIND = Kind

    def __init__(self, agent, shp):
        dqn_mlp.Step.__init__(self, agent, shp)
        d, b = self._up.dev, self.batch
        self.prob = d[self._o_prob:self._o_prob + 4 * b].view(torch.float32)
        self.beta = d[self._o_beta:self._o_beta + 4].view(torch.float32)
        # the static [K][numel] block draw_rows(k) fills, taken up without a draw
        self.noise_rows = agent.network.noise_block().rows_block(self.k)
        self.tree_idx = None            # the last draw's leaves: what the commit behind the learn region gates on

    def staged_tail(self):
        """The sampling probabilities (f32 [B]) and beta (f32) behind the parent's block."""
        self._o_prob = self._o_tail
        self._o_beta = self._o_prob + (4 * self.batch + 7) // 8 * 8
        return self._o_beta + 8 - self._o_tail

    def make_outputs(self, dev):
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        b, n = self.batch, self.shape[4]
        self.loss, self.loss_vec, self.prio, self.weights = f(1), f(b), f(b), f(b)
        self.q_next, self.target = f(b, 2), f(b, n)

    def net_struct(self):
        a, cfg = self.agent, self.agent.config
        flat, block, tblock = a._fused.flat, a.network.noise_block(), a.target_network.noise_block()
        n = fill_layers(Net(), a.network, flat.offset_of, block.slices)
        n.param, n.target = flat.flat.data_ptr(), a._target_flat.flat.data_ptr()
        # acting reads row k of the rows block, the update the networks' own buffers (their last reset_noise())
        n.noise, n.noise_stride = self.noise_rows.data_ptr(), block.numel
        n.target_noise = tblock.flat.data_ptr()
        for field, v in zip(Kind.DIMS, self.shape):
            setattr(n, field, v)
        n.v_min, n.v_max = float(cfg.categorical_v_min), float(cfg.categorical_v_max)
        return n

    def update(self):
        """dra_rainbow_mlp_update on the staged indices, probabilities and beta: the gradient lands in the optimiser's flat
        gradient buffer, the new priorities in self.prio."""
        a = self.agent
        cfg, rp = a.config, a._inner_replay()
        io = UpdateIO()
        io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = self.ring.pointers()
        io.idx, io.prob, io.beta = self.idx.data_ptr(), self.prob.data_ptr(), self.beta.data_ptr()
        io.grad = a._fused.flat.grad.data_ptr()
        io.out_loss, io.out_loss_vec, io.out_prio = self.loss.data_ptr(), self.loss_vec.data_ptr(), self.prio.data_ptr()
        io.out_weights, io.out_q_next, io.out_target = self.weights.data_ptr(), self.q_next.data_ptr(), self.target.data_ptr()
        io.err, io.capacity = self.err.data_ptr(), self.capacity
        io.discount, io.step_discount = float(cfg.discount) ** int(cfg.n_step), float(rp.discount)
        io.replay_eps, io.replay_alpha = float(cfg.replay_eps), float(cfg.replay_alpha)
        io.batch, io.double_q, io.n_step = self.batch, int(bool(cfg.double_q)), int(rp.n_step)
        net = self.net_struct()
        net.noise = a.network.noise_block().flat.data_ptr()
        lib.dra_rainbow_mlp_update(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        return self.loss

    def module_update(self):
        """config.fused_rainbow_update False: ring.gather on the staged indices (its n-step fold), then the agent's own
        _loss_grad under the modules' current noise (the four NoisyLinear forwards per pass, ops.per_weights_dev on the staged
        probabilities and beta, ops.c51_loss, autograd); the priorities land in self.prio, where the commit reads them."""
        agent = self.agent
        cfg, rp = agent.config, agent._inner_replay()
        self.static = g = rp.gather(self.idx, out=self.static)
        tr = rp.TransitionCLS(state=g['state'], action=g['action'], reward=g['reward'], next_state=g['next_state'], mask=g['mask'],
                              sampling_prob=self.prob, idx=None)
        per = dict(sampling_prob=self.prob, beta=-1.0, beta_dev=self.beta, replay_eps=cfg.replay_eps, replay_alpha=cfg.replay_alpha)
        out, (net_out, grad) = agent._loss_grad(tr, per)
        self.prio.copy_(out['prio'])
        agent._fused.zero_grad()
        agent._backward(net_out, grad)
        return out['loss']

    def prepare(self):
        """The step's draws in the host path's order: per transition np.random as epsilon_greedy(0, q) consumes it
        (torch_utils.py:51-58: randint(A, size=1), rand(1); the values are not used) and one reset_noise() (row k of the rows
        block), the feed's bookkeeping with the tree's adds, then (total_steps > exploration_steps) the prioritised draw, the
        target's and the online network's reset_noise() and beta -- staged with one copy.  -> whether the step updates."""
        agent = self.agent
        cfg, actor, rp = agent.config, agent.actor, agent._inner_replay()
        k = self.k
        for _ in range(k):
            np.random.randint(self.shape[1], size=1)
            np.random.rand(1)
        actor._total_steps += k
        rows = agent.network.noise_block().draw_rows(k)
        assert rows.data_ptr() == self.noise_rows.data_ptr()
        slot0 = int(rp.pos)
        rp.advance(k)
        self.episodes.begin(k)
        agent.total_steps += k
        learn = agent.total_steps > cfg.exploration_steps
        raw = self._up.stage().numpy()
        raw[:8].view(np.int64)[0] = slot0
        raw[self._o_rand:self._o_flag].view(np.int64)[...] = 0
        raw[self._o_flag:self._o_flag + k] = 0
        idx = None
        if learn:
            self.tree_idx, prob, idx = rp.draw()
            agent.target_network.reset_noise()
            agent.network.reset_noise()
            raw[self._o_idx:self._o_rand].view(np.int64)[...] = idx
            raw[self._o_prob:self._o_prob + 4 * self.batch].view(np.float32)[...] = prob
            raw[self._o_beta:self._o_beta + 4].view(np.float32)[0] = cfg.replay_beta()
        self._up.send()
        self.last_draws = (np.zeros(k, dtype=bool), np.zeros(k, dtype=np.int64), slot0, idx)
        return learn

    def after_learn(self):
        """replay.py:193-196 with the priorities still on the device: the pending marks and first-writer-wins are gated on the
        host, so the commit runs eagerly behind the replayed region, as the target copy does."""
        self.agent._inner_replay().commit_device(self.tree_idx, self.prio)


def adopt(agent):
    """A Step with the actor's environment on the device when configuration, agent and task allow it; else None (the host path;
    with the switch on the reason is logged once)."""
    return dqn_mlp.adopt(agent, Step)
