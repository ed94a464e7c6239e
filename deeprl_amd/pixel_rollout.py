"""What the device rollouts over NatureConvBody share (A2C / PPO, n-step DQN, option-critic on pixels): the checks that a body
and a head are ones the rollout kernels can walk and that an agent's task may run on the device, the activation buffers with
their pre-built launch arguments, the trunk's three launches per rollout step -- a step is [conv1 | head of step t - 1] (the
rollout's own entry), then conv2, conv3 and fc4's 28 K-slice partial sums -- and the update over the activations a rollout
stored.  The three rollouts keep what differs: the conv1 + head entry and its arguments, the final stand-alone head call, which
network runs step T, their extra buffers, the loss call and what compute() returns.
There is no CPU / eager implementation here: without the HIP library every launch raises.
"""
import ctypes

import numpy as np
import torch

from . import ops
from ._lib import lib, stream_ptr
from .device_env import DeviceAtariVec
from .nets import (CategoricalActorCriticNet, Conv2d, DummyBody, Linear, NatureConvBody, OptionCriticNet, VanillaNet, _claim_direct,
                   direct_param_grads, fc4_from_rollout)
from .support import Config, StagedUpload, plan_epsilon_greedy

RELU = ops.ACT["relu"]


# ------------------------------------------------------------------------------------------------------------ checks
def k_major(conv):
    """The conv weight is stored [(c, kh, kw)][oc] (optim.FlatParams(koc=...)): the layout the rollout's conv kernels read."""
    return conv.weight.permute(1, 2, 3, 0).is_contiguous()


def plain_linear(m, fused_act=None):
    """`m` is a plain contiguous Linear layer with a bias and the given fused activation (a head: none)."""
    return type(m) is Linear and m.bias is not None and m.weight.is_contiguous() and m.fused_act == fused_act


def walkable_trunk(body):
    """`body` is a NatureConvBody the rollout kernels can walk: not noisy, three biased K-major Conv2d layers, fc4 a plain
    contiguous biased Linear of shape (512, 3136) with its fused ReLU."""
    if type(body) is not NatureConvBody or getattr(body, 'noisy_linear', False):
        return False
    if not all(type(c) is Conv2d and c.bias is not None and k_major(c) for c in (body.conv1, body.conv2, body.conv3)):
        return False
    return plain_linear(body.fc4, "relu") and tuple(body.fc4.weight.shape) == (512, 3136)


def rollout_switch(cfg):
    return getattr(cfg, 'fused_rollout', True) is not False


def fits(history, n):
    """What the rollout launches are built for: stacks of four frames, at most 32 environments."""
    return history == 4 and n <= 32


def task_may_move(task, cfg):
    """The agent's host task may run on the device under a rollout that also runs the update: the switch is on, the task is one
    DeviceAtariVec adopts, the run is not distributed (data-parallel agents keep the host path), and the rollout fits the kernels
    (history 4, n <= 32, T * n <= 2048 rows, every worker an environment)."""
    if not rollout_switch(cfg) or not DeviceAtariVec.eligible(task, cfg):
        return False
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        return False
    envs = task.env.envs
    n = len(envs)
    return fits(envs[0].history, n) and int(cfg.rollout_length) * n <= 2048 and int(cfg.num_workers) == n


# ------------------------------------------------------------------------------------------- buffers and trunk launches
def _one(t):
    return (ctypes.c_void_p * 1)(t.data_ptr())


def activation_buffers(rows, phi_rows, n, **extra):
    """The activations of `rows` trunk steps over n environments (every step is kept: the update backpropagates through them, as
    the reference does through the rollout's own forward graph), fc4's 28 K-slice slabs, `phi_rows` rows of folded features and
    the per-step pointer arguments of the launches, built once (a rollout loop is host-side eager code)."""
    dev = Config.DEVICE
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    b = dict(extra, y1=f(rows, n, 32, 20, 20), y2=f(rows, n, 64, 9, 9), y3=f(rows, n, 64, 7, 7), slabs=f(28, n, 512),
             phi=f(phi_rows, n, 512))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    b['args'] = [(_one(b['y1'][t]), _one(b['y2'][t]), _one(b['y3'][t])) for t in range(rows)]
    b['y1_p'], b['phi_p'], b['slabs_p'] = [p(y) for y in b['y1']], [p(y) for y in b['phi']], p(b['slabs'])
    return b


def trunk_args(body):
    """The pointer arguments of trunk_step for `body`'s conv2, conv3 and fc4 ([(c, kh, kw)][oc] conv storage)."""
    return (_one(body.conv2.weight), _one(body.conv2.bias), _one(body.conv3.weight), _one(body.conv3.bias), _one(body.fc4.weight))


def trunk_step(b, t, n, body_args, st):
    """Step t behind its conv1 launch: conv2, conv3, fc4's 28 K-slice partial sums (the next head launch folds them)."""
    y1, y2, y3 = b['args'][t]
    w2, b2, w3, b3, w4 = body_args
    lib.dra_conv_fwd_koc(2, 1, y1, w2, b2, y2, n, 0, 1.0, RELU, st)
    lib.dra_conv_fwd_koc(3, 1, y2, w3, b3, y3, n, 0, 1.0, RELU, st)
    lib.dra_linear_fwd_slabs_one(1, y3, w4, n, 3136, 512, 28, b['slabs_p'], st)


# ------------------------------------------------------------------------------------------------------------ update
def hand_over(body, b, t_len, n):
    """The conv layers' next forward -- ONE call each, over the T x N stored observations -- takes the rollout's stored outputs
    (same inputs, same parameters) instead of recomputing them (Conv2d._y_pre)."""
    for conv, key in ((body.conv1, 'y1'), (body.conv2, 'y2'), (body.conv3, 'y3')):
        y = b[key][:t_len]
        conv._y_pre = y.reshape((t_len * n,) + tuple(y.shape[2:]))


def update(agent, t_len, n, frames, b, body, heads, loss):
    """The update over the rollout's own activations: one batched conv forward over the stored outputs, fc4 from its stored
    features, then `loss(phi [T * N, 512])` -- the launch that writes the gradients of `heads` in place and returns its outputs,
    'dphi' among them -- the backward through fc4 and the convolutions and the fused clip + optimizer step.  -> loss's outputs."""
    cfg = agent.config
    rows = t_len * n
    hand_over(body, b, t_len, n)
    y3 = body.conv3(body.conv2(body.conv1(frames[:t_len].reshape((rows,) + tuple(frames.shape[2:])))))
    phi_pre = b['phi'].view(rows, 512)
    phi = fc4_from_rollout(body, y3.view(rows, -1), phi_pre)
    agent._fused.zero_grad(direct=True)
    defer = agent._fused if getattr(cfg, 'defer_conv_folds', True) else None
    with direct_param_grads(True, defer_folds_to=defer, covers=[agent._fused]):
        _claim_direct(heads)
        out = loss(phi_pre)
        torch.autograd.backward([phi], [out['dphi']])
    agent._fused.step(cfg.gradient_clip)
    return out


# ------------------------------------------------------------------------------------------------------------ rollouts
class _PixelRollout:
    """The no-grad forwards of one A2C / PPO rollout over CategoricalActorCriticNet(NatureConvBody) and device-resident synthetic
    Atari environments as FOUR launches per step instead of five (csrc/conv_v2.hip: rollout_conv1_heads_kernel): [conv1 of step t
    | fc4's finish + policy head of step t - 1], conv2, conv3, fc4's 28 K-slice partial sums -- every launch of such a step is a few dozen workgroups at its latency floor,
    so the step costs what its launches cost.  The head of step t - 1 can share conv1's launch because the planned observations
    do not depend on the actions (DeviceAtariVec.states_all).  Same device functions as the module path: the rollout's actions,
    log-probabilities, entropies and values are bit-identical (tests/test_gpu_agents.py).  a2c_pixel 209 k -> 224 k, ppo_pixel
    109 k -> 118 k env-steps/s (profiles/r05x_bench_agents_c3fc4_ab.jsonl; conv3 + fc4 as one launch was measured too and lost)."""

    def __init__(self, agent):
        self.agent = agent
        self.bufs = None

    def eligible(self):
        """The task is already on the device (the agent adopts it for its module path too) and may be any size the plan allows:
        the update is not this rollout's, so no row cap; a rank-invariant sampler or rollout_fc4_slices off keep the module path."""
        a = self.agent
        net, cfg = a.network, a.config
        if not rollout_switch(cfg) or Config.DEVICE.type != 'cuda' or not isinstance(a.task, DeviceAtariVec):
            return False
        if type(net) is not CategoricalActorCriticNet or getattr(net, 'sampler', None) is not None or not getattr(net, 'rollout_fc4_slices', True):
            return False
        if type(net.actor_body) is not DummyBody or type(net.critic_body) is not DummyBody or not walkable_trunk(net.phi_body):
            return False
        if getattr(net.phi_body.conv1, 'u8_coef', None) is None or not fits(a.task.history, a.task.num_envs):
            return False
        return (plain_linear(net.fc_action) and plain_linear(net.fc_critic) and net.fc_action.weight.shape[0] <= 64
                and net.fc_critic.weight.shape[0] == 1)

    def run(self, frames, slots):
        """frames: uint8 [T + 1, N, 4, 84, 84]; fills rows 0..T of `slots` (action, log_pi_a, entropy, v) from slots.uniform."""
        net = self.agent.network
        body = net.phi_body
        rows, n = int(frames.shape[0]), int(frames.shape[1])
        if self.bufs is None or self.bufs['n'] != n or self.bufs['rows'] < rows:
            self.bufs = activation_buffers(rows, rows, n)
            self.bufs.update(n=n, rows=rows)
        b = self.bufs
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        st = stream_ptr()
        wa, ba, wv, bv = net.fc_action.weight, net.fc_action.bias, net.fc_critic.weight, net.fc_critic.bias
        n_act = int(wa.shape[0])
        coef = float(body.conv1.u8_coef)
        w1, b1, b4, slabs = p(body.conv1.weight), p(body.conv1.bias), p(body.fc4.bias), b['slabs_p']
        heads = (p(wa), p(ba), p(wv), p(bv))
        args = trunk_args(body)
        for t in range(rows):
            # fc4 of step t - 1 left its 28 K-slice partial sums: the head that rides in this launch folds them (bias, ReLU) first
            # (and leaves the folded features of step t - 1 in phi[t - 1]: fc4's forward output, for A2C's update)
            if t > 0:
                s = t - 1
                lib.dra_rollout_conv1_heads_phi(p(frames[t]), w1, b1, b['y1_p'][t], n, coef, slabs, b4, *heads, p(slots.uniform[s]),
                                                n_act, p(slots.action[s]), p(slots.log_pi_a[s]), p(slots.entropy[s]), p(slots.v[s]),
                                                b['phi_p'][s], st)
            else:
                lib.dra_rollout_conv1_heads_phi(p(frames[t]), w1, b1, b['y1_p'][t], n, coef, None, None, *heads, None, n_act, None,
                                                None, None, None, None, st)
            trunk_step(b, t, n, args, st)
        t = rows - 1
        lib.dra_policy_heads_sample_fold28(slabs, b4, *heads, p(slots.uniform[t]), n, n_act, p(slots.action[t]), p(slots.log_pi_a[t]),
                                           p(slots.entropy[t]), p(slots.v[t]), st)
        slots.end()


class _TargetRollout:
    """What _QRollout and _OCRollout share: the agent's task may move to the device (`eligible`: task_may_move, a walkable trunk,
    the subclass's `heads_fit`), and compute(plan) is T + 1 trunk steps -- steps 0..T-1 on the online body, step T on the TARGET
    network's (its conv1 launch carries the online head of step T - 1) -- the subclass's bootstrap head, then `update` over the
    rollout's own activations (the reference keeps the rollout's own forward graph).  A subclass names its network class (NET),
    `heads_fit(net)`, `prepare(t_len)` (the host's draws and uploads ahead of the captured region), `buffers`, `conv1_head(b, frames,
    t, body, plan)`, `bootstrap(b)`, `head_params()`, `loss(b, plan, phi)` and `result(b, out)`."""
    NET = None

    def __init__(self, agent):
        self.agent = agent
        self.bufs = None

    def eligible(self):
        a = self.agent
        net = a.network
        return (task_may_move(a.task, a.config) and type(net) is self.NET and walkable_trunk(net.body) and self.heads_fit(net))

    def compute(self, plan):
        a = self.agent
        online, target = a.network.body, a.target_network.body
        t_len, n = plan.t_len, a.task.num_envs
        b = self.buffers(t_len, n)
        frames = a.task.states_all(plan)           # every observation of the planned rollout, one launch
        st = stream_ptr()
        args = trunk_args(online)
        for t in range(t_len):
            self.conv1_head(b, frames, t, online, plan)
            trunk_step(b, t, n, args, st)
        self.conv1_head(b, frames, t_len, target, plan)
        trunk_step(b, t_len, n, trunk_args(target), st)
        self.bootstrap(b)
        a._rollout_step += t_len
        out = update(a, t_len, n, frames, b, online, self.head_params(), lambda phi: self.loss(b, plan, phi))
        return self.result(b, out)


class _QRollout(_TargetRollout):
    """NStepDQNAgent's device path over VanillaNet(NatureConvBody) and device-resident synthetic Atari environments.  Per rollout
    step the four launches of _PixelRollout with the Q head in conv1's launch (dra_rollout_conv1_qheads: [conv1 of step t | fc4's
    fold + Q head + epsilon-greedy selection of step t - 1], conv2, conv3, fc4's 28 K-slice partial sums); step T is the TARGET
    network's forward of the last observation (its conv1 launch carries the online head of step T - 1), then its max head
    (dra_q_heads_fold28, NStepDQN_agent.py:56-57).  The update: returns, loss and the Q head's backward in one launch
    (dra_nstep_q_loss_bwd), fc4 and the convolutions backpropagate through the activations the rollout stored (the reference keeps
    the rollout's own forward graph, NStepDQN_agent.py:33-67), then the fused clip + optimizer step."""
    NET = VanillaNet
    _up = None

    @staticmethod
    def heads_fit(net):
        return plain_linear(net.fc_head) and 1 <= net.fc_head.weight.shape[0] <= 64

    def prepare(self, t_len):
        """Draws the rollout's exploration (support.plan_epsilon_greedy) and stages it into the persistent device buffers the
        Q-head launches read (fixed addresses: graph replays see the new values)."""
        a = self.agent
        n, n_act = a.task.num_envs, int(a.network.fc_head.weight.shape[0])
        explore, rand = plan_epsilon_greedy(a.config.random_action_prob, t_len, n, n_act, a.config.num_workers)
        o = t_len * n * 8       # one block, one copy: int64 random actions | uint8 explore flags
        if self._up is None or self.explore.shape[0] != t_len:
            self._up = StagedUpload(o + t_len * n, torch.uint8, Config.DEVICE)
            self.random_action = self._up.dev[:o].view(torch.int64).view(t_len, n)
            self.explore = self._up.dev[o:].view(t_len, n)
        raw = self._up.stage().numpy()
        raw[:o].view(np.int64).reshape(t_len, n)[...] = rand
        raw[o:].reshape(t_len, n)[...] = explore
        self._up.send()

    def buffers(self, t_len, n):
        n_act = int(self.agent.network.fc_head.weight.shape[0])
        if self.bufs is None or self.bufs['key'] != (t_len, n, n_act):
            dev = Config.DEVICE
            self.bufs = activation_buffers(t_len + 1, t_len, n, key=(t_len, n, n_act),
                                           q=torch.empty((t_len, n, n_act), dtype=torch.float32, device=dev),
                                           action=torch.empty((t_len, n), dtype=torch.int64, device=dev),
                                           bootstrap=torch.empty(n, dtype=torch.float32, device=dev))
        return self.bufs

    def conv1_head(self, b, frames, t, body, plan):
        net = self.agent.network
        head, s = net.fc_head, t - 1
        ops.rollout_conv1_qheads(frames[t], body.conv1.weight, body.conv1.bias, b['y1'][t], float(net.body.conv1.u8_coef),
                                 *((b['slabs'], net.body.fc4.bias, head.weight, head.bias, self.explore[s], self.random_action[s],
                                    b['q'][s], b['action'][s], b['phi'][s]) if t > 0 else ()))

    def bootstrap(self, b):
        tgt = self.agent.target_network
        ops.q_heads_fold28(b['slabs'], tgt.body.fc4.bias, tgt.fc_head.weight, tgt.fc_head.bias, out_max=b['bootstrap'])

    def head_params(self):
        head = self.agent.network.fc_head
        return (head.weight, head.bias)       # the loss launch writes the Q head's gradient in place

    def loss(self, b, plan, phi):
        head = self.agent.network.fc_head
        t_len, n = b['action'].shape
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=phi.device)
        return ops.nstep_q_loss_bwd(b['q'], b['action'], plan.reward, plan.mask, b['bootstrap'], self.agent.config.discount, phi,
                                    head.weight, out=dict(ret=f(t_len, n), loss=f(1), dw=head.weight.grad, db=head.bias.grad,
                                                          dphi=f(t_len * n, 512)))

    @staticmethod
    def result(b, out):
        return dict(loss=out['loss'], ret=out['ret'], q=b['q'], action=b['action'], bootstrap=b['bootstrap'])


class _OCRollout(_TargetRollout):
    """OptionCriticAgent's device path over OptionCriticNet(NatureConvBody) and device-resident synthetic Atari environments.  Per
    rollout step the four launches of _PixelRollout with the option-critic head in conv1's launch (dra_rollout_conv1_ocheads:
    [conv1 of step t | fc4's fold + q / beta / intra-option logits + option and action choice of step t - 1], conv2, conv3, fc4's
    28 K-slice partial sums); step T is the TARGET network's forward of the last observation (its conv1 launch carries the online
    head of step T - 1), then its bootstrap head (dra_oc_heads_fold28, OptionCritic_agent.py:87-93).  The update: returns,
    advantages, the three losses and the heads' backward in one launch (dra_oc_loss_bwd), fc4 and the convolutions backpropagate
    through the activations the rollout stored, then the fused clip + optimizer step.  The carried option state (prev_option,
    is_initial) lives in persistent device buffers the head launches read and replace.  Random draws: one uniform_() [T, N, 3] per
    rollout on torch's device generator (draw_uniforms, before the captured region), turned into options and actions by inverse
    CDF -- the documented deviation of A2C's RolloutSlots: Categorical.sample()'s own stream is not reproduced."""
    NET = OptionCriticNet
    KEYS = ("q", "beta", "logits", "option", "action", "log_pi_a", "entropy", "prev_option", "init", "phi")
    _eps_up = uniform = eps = None

    @staticmethod
    def heads_fit(net):
        n_opt, n_act = int(net.num_options), int(net.action_dim)
        return (all(plain_linear(m) for m in (net.fc_q, net.fc_pi, net.fc_beta)) and 1 <= n_opt <= 8 and 1 <= n_act <= 18
                and tuple(net.fc_q.weight.shape) == (n_opt, 512) and tuple(net.fc_beta.weight.shape) == (n_opt, 512)
                and tuple(net.fc_pi.weight.shape) == (n_opt * n_act, 512))

    def state(self, n):
        """The carried option state (OptionCritic_agent.py:26-27: ones at the start): persistent device buffers."""
        dev = Config.DEVICE
        self.prev_option = torch.ones(n, dtype=torch.int64, device=dev)
        self.is_initial = torch.ones(n, dtype=torch.bool, device=dev)
        return self.prev_option, self.is_initial

    def prepare(self, t_len):
        self.upload_exploration(t_len)
        self.draw_uniforms(t_len)

    def upload_exploration(self, t_len):
        """config.random_option_prob(num_workers) once per rollout step -- the reference's calls in its order -- staged into the
        persistent [T] buffer the head launches read (a fixed address: graph replays see the new values).  -> the host values."""
        a = self.agent
        eps = np.asarray([a.config.random_option_prob(a.config.num_workers) for _ in range(t_len)], dtype=np.float64)
        if self._eps_up is None or self._eps_up.dev.shape[0] != t_len:
            self._eps_up = StagedUpload(t_len, torch.float32, Config.DEVICE)
        self.eps = self._eps_up.put(eps)
        return eps

    def draw_uniforms(self, t_len):
        """One uniform_() [T, N, 3] on torch's device generator into a persistent buffer (columns: fresh option, continued option,
        action).  Runs before the captured region, so replays read the new draw at the same address."""
        n = self.agent.task.num_envs
        if self.uniform is None or self.uniform.shape[0] != t_len:
            self.uniform = torch.empty((t_len, n, 3), dtype=torch.float32, device=Config.DEVICE)
        self.uniform.uniform_()

    def buffers(self, t_len, n):
        net = self.agent.network
        n_opt, n_act = int(net.num_options), int(net.action_dim)
        if self.bufs is None or self.bufs['key'] != (t_len, n, n_opt, n_act):
            dev = Config.DEVICE
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            i = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
            self.bufs = activation_buffers(t_len + 1, t_len, n, key=(t_len, n, n_opt, n_act), q=f(t_len, n, n_opt),
                                           beta=f(t_len, n, n_opt), logits=f(t_len, n, n_act), option=i(t_len, n), action=i(t_len, n),
                                           log_pi_a=f(t_len, n), entropy=f(t_len, n), prev_option=i(t_len, n), init=f(t_len, n),
                                           boot=f(n))
        return self.bufs

    def head_params(self):
        net = self.agent.network
        return (net.fc_q.weight, net.fc_q.bias, net.fc_beta.weight, net.fc_beta.bias, net.fc_pi.weight, net.fc_pi.bias)

    def conv1_head(self, b, frames, t, body, plan):
        online = self.agent.network.body
        coef = float(online.conv1.u8_coef)
        if t > 0:
            s = t - 1
            ops.rollout_conv1_ocheads(frames[t], body.conv1.weight, body.conv1.bias, b['y1'][t], coef, b['slabs'], online.fc4.bias,
                                      self.head_params(), self.uniform[s], self.eps[s:s + 1], plan.mask[s], self.prev_option,
                                      self.is_initial, out={k: b[k][s] for k in self.KEYS})
        else:
            ops.rollout_conv1_ocheads(frames[t], body.conv1.weight, body.conv1.bias, b['y1'][t], coef)

    def bootstrap(self, b):
        tgt = self.agent.target_network
        ops.oc_heads_fold28(b['slabs'], tgt.body.fc4.bias, tgt.fc_q.weight, tgt.fc_q.bias, tgt.fc_beta.weight, tgt.fc_beta.bias,
                            prev_option=self.prev_option, boot=b['boot'])

    def loss(self, b, plan, phi):
        net, cfg = self.agent.network, self.agent.config
        t_len, n = b['action'].shape
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=phi.device)
        # (the loss launch writes the three heads' gradients in place)
        return ops.oc_loss_bwd(b, plan.reward, plan.mask, b['boot'], self.eps, cfg.discount, cfg.termination_regularizer,
                               cfg.entropy_weight, phi, net.fc_q.weight, net.fc_pi.weight, net.fc_beta.weight,
                               out=dict(ret=f(t_len, n), adv=f(t_len, n), beta_adv=f(t_len, n), loss=f(4),
                                        dw_q=net.fc_q.weight.grad, db_q=net.fc_q.bias.grad, dw_pi=net.fc_pi.weight.grad,
                                        db_pi=net.fc_pi.bias.grad, dw_beta=net.fc_beta.weight.grad,
                                        db_beta=net.fc_beta.bias.grad, dphi=f(t_len * n, 512)))

    @staticmethod
    def result(b, out):
        return dict(q=b['q'], beta=b['beta'], logits=b['logits'], option=b['option'], prev_option=b['prev_option'], init=b['init'],
                    action=b['action'], log_pi_a=b['log_pi_a'], entropy=b['entropy'], boot=b['boot'], ret=out['ret'],
                    advantage=out['adv'], beta_advantage=out['beta_adv'], loss=out['loss'][:1], losses=out['loss'])
