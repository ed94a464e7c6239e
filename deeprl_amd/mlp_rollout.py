"""What the host sides of the small-MLP kernels share (a2c_mlp.py, cat_mlp.py, q_mlp.py, oc_mlp.py, dqn_mlp.py, dist_mlp.py,
ppo_mlp.py, dpg_mlp.py): the gate codes, the ONE check that a body is a two-layer FCBody the kernels walk and that a head is a
plain Linear, the shape tables (`shape_table`), the ONE filler of a net struct (`fill_net`), the conditions on the optimiser's
ownership (`unowned`) and on a target network (`target_why_not`), the agent-side conditions of a device rollout (`why_not`), the
ONE way an agent takes such a rollout up (`adopt`), the `Rollout` base of a2c_mlp.Rollout / cat_mlp.Rollout -- the kernel's two
structs over the agent's ONE flat parameter buffer and its device-resident environments, one launch per rollout -- and
`TargetRollout`, the base of q_mlp.Rollout / oc_mlp.Rollout, which adds the target network's flat buffer, the kernel's own step
counter and the update kernel's row condition.
There is no CPU / eager implementation here: without the HIP library every call raises.
"""
import ctypes
from collections import namedtuple

import torch
import torch.nn.functional as F

from ._lib import lib, stream_ptr
from .support import Config

GATES = {F.relu: 1, torch.relu: 1, torch.tanh: 2, F.tanh: 2}      # ops.ACT codes

Plan = namedtuple('Plan', ['counters', 't_len'])      # what graphs._OnPolicyGraph.run reads of a rollout plan


def fc_body(body):
    """(in, h1, h2, gate code) when `body` is a two-layer FCBody of plain Linear layers with biases under a relu or tanh gate, not
    noisy; else None."""
    from .nets import FCBody, Linear
    if type(body) is not FCBody or body.noisy_linear or body.gate not in GATES or len(body.layers) != 2:
        return None
    if any(type(layer) is not Linear or layer.bias is None for layer in body.layers):
        return None
    w1, w2 = body.layers[0].weight, body.layers[1].weight
    if w2.shape[1] != w1.shape[0]:
        return None
    return int(w1.shape[1]), int(w1.shape[0]), int(w2.shape[0]), GATES[body.gate]


def head_out(head, in_features):
    """The output width when `head` is a plain Linear layer with a bias over `in_features` inputs; else None."""
    from .nets import Linear
    if type(head) is not Linear or head.bias is None or head.weight.shape[1] != in_features:
        return None
    return int(head.weight.shape[0])


def body_params(body):
    a, b = body.layers
    return [a.weight, a.bias, b.weight, b.bias]


def shape_table(entry):
    """The `(dims...) -> bool` of the library's `entry` (a `*_supported` function): whether a kernel is built for the shape."""
    def table(*dims):
        return getattr(lib, entry).raw(*map(int, dims)) == 0
    return table


def fill_net(n, flat, fields, dims, shp, target=None):
    """Fills the net struct `n`: the flat buffer of the online FlatParams `flat` (and of `target`, where the struct has one),
    the offset of every (field, parameter) pair of `fields` into it, and the shape `shp` under the names `dims`.  -> n"""
    n.param = flat.flat.data_ptr()
    if target is not None:
        n.target = target.flat.data_ptr()
    for field, p in fields:
        setattr(n, field, flat.offset_of(p))
    for field, v in zip(dims, shp):
        setattr(n, field, v)
    return n


def unowned(agent, fields):
    """The reason when agent._fused, the ONE optimiser, does not own every parameter of `fields(agent.network)`; else None."""
    owned = agent._fused.flat.params
    if any(all(p is not q for q in owned) for _, p in fields(agent.network)):
        return "one optimiser does not own every parameter the kernel reads"
    return None


def target_why_not(agent, shape, fields, shp, other_shape):
    """The target network's conditions: `other_shape` (the caller's words) when it has not the online network's shape `shp`, a
    reason of this function's own when its parameters lie elsewhere in their flat buffer than the online ones in theirs; else
    None."""
    if shape(agent.target_network) != shp:
        return other_shape
    flat, target = agent._fused.flat, agent._target_flat
    if ([flat.offset_of(p) for _, p in fields(agent.network)] != [target.offset_of(p) for _, p in fields(agent.target_network)]):
        return "the online and the target parameters are laid out differently in their flat buffers"
    return None


def why_not(kind, agent, supported_fn=None):
    """None when `agent` may run on the rollout kernel of `kind` (a Rollout subclass), else the first reason it may not
    (everything but the task itself, which the device_env class decides).  An agent without a `dp` is not data parallel."""
    cfg = agent.config
    if not kind.switched_on(cfg):
        return "config.%s is %s" % (kind.SWITCH, "not on" if kind.OPT_IN else "off")
    if getattr(agent, 'dp', None) is not None and agent.dp.active:
        return "the agent is data parallel"
    if agent.grad_hook is not None:
        return "a grad_hook is installed"
    shp = kind.network_shape(agent.network)
    if shp is None:
        return "the network is not %s" % kind.NETWORK
    why = unowned(agent, kind.fields)
    if why is not None:
        return why
    if not (supported_fn or kind.supported)(shp[0], shp[1], shp[2], int(cfg.num_workers), shp[3]):
        return "%s is not built for state_dim %d, %d actions, hidden %d, %d environments" % (
            kind.ENTRY, shp[0], shp[1], shp[2], int(cfg.num_workers))
    return None


def adopt(agent, kind):
    """A `kind` rollout with agent.task on the device when task, configuration and agent allow it; else None (the host path)."""
    able = kind.VEC.eligible(agent.task, agent.config)
    why = kind.why_not(agent) if able else kind.NOT_TASK
    if why is not None:
        kind.stays_on_host(agent, why)
    if why is not None or not able:
        return None
    rollout = kind(agent, kind.network_shape(agent.network))
    rollout.attach()
    agent.states = None
    return rollout


class Rollout:
    """One launch per rollout over the agent's device-resident environments (agent.task: a device_env class with fill_io) and its
    flat parameter buffer.  A subclass names its kernel: the config switch, the library entry, the two struct mirrors, the
    struct's four shape fields, `network_shape(network)`, `fields(network)` -- the (offset field, parameter) pairs -- and
    `supported(...)`; whether the switch must be set to turn the path on (`OPT_IN`) and what is said of a task that cannot move
    (`NOT_TASK`, None: nothing); how the task moves to the device (`VEC`, `attach`); and where A2CAgent's device step
    differs between them: `begin_step` / `end_step` (episode reporting), `signature()` (what a captured launch has baked in: the
    arguments fill_io takes behind t_len, then the noise seed; kept in `sig`) and `ACTION_VIEW` (the stored actions' shape
    behind the row axis)."""
    SWITCH = ENTRY = VEC = NETWORK = Net = IO = DIMS = ACTION_VIEW = NOT_TASK = None
    OPT_IN = False

    def __init__(self, agent, shp):
        self.agent = agent
        self.shape = shp
        self.launches = 0
        self.sig = None         # signature() of the captured launch

    def net_struct(self):
        return fill_net(self.Net(), self.agent._fused.flat, self.fields(self.agent.network), self.DIMS, self.shape)

    def run(self, t_len):
        """One rollout launch on the current stream; returns the task's buffers (state, action, v, reward, mask)."""
        io = self.IO()
        b = self.agent.task.fill_io(io, self.agent, t_len, *self.sig[:-1])
        net = self.net_struct()
        getattr(lib, self.ENTRY)(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        self.launches += 1
        return b

    @classmethod
    def switched_on(cls, cfg):
        return getattr(cfg, cls.SWITCH, False) is True if cls.OPT_IN else getattr(cfg, cls.SWITCH, True) is not False

    why_not = classmethod(lambda cls, agent: why_not(cls, agent))      # (a kind with conditions of its own adds them)

    def attach(self):
        self.agent.task = self.VEC(self.agent.task)

    @classmethod
    def stays_on_host(cls, agent, why):
        # (logged where the VEC has a line for it, HOST_NOTE, unless the switch itself is off)
        note = getattr(cls.VEC, 'HOST_NOTE', None)
        if note and cls.switched_on(agent.config):
            getattr(agent.logger, 'warning', agent.logger.info)(note % why)

    def end_step(self):
        return


class TargetRollout(Rollout):
    """A Rollout whose kernels also read the agent's TARGET network (a flat buffer of the online one's layout), stamp the episode
    ring's rows with a step counter of their own and leave the rollout's buffers to an update kernel (`UPDATE`, under the config
    switch `UPDATE_SWITCH`, its shapes in `update_supported`): q_mlp.Rollout, oc_mlp.Rollout.  A subclass fills what its rollout
    io has of its own in `fill_own(io)`."""
    UPDATE = UPDATE_SWITCH = update_supported = None

    def __init__(self, agent, shp):
        Rollout.__init__(self, agent, shp)
        # the kernel's own step counter: the ring rows carry it (device_env.EpisodeRing turns it into a step number)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=Config.DEVICE)

    @classmethod
    def target_why_not(cls, agent, shp):
        """Behind why_not(cls, agent): the target's shape and layout, then the update kernel's rows."""
        why = target_why_not(agent, cls.network_shape, cls.fields, shp, "the network is not %s" % cls.NETWORK)
        if why is not None:
            return why
        cfg = agent.config
        n, t_len = int(cfg.num_workers), int(cfg.rollout_length)
        if getattr(cfg, cls.UPDATE_SWITCH, True) is not False and not cls.update_supported(shp[0], shp[1], shp[2], t_len * n, *shp[3:]):
            return "%s is not built for %d rows (rollout length %d x %d environments)" % (cls.UPDATE, t_len * n, t_len, n)
        return None

    def net_struct(self):
        a = self.agent
        return fill_net(self.Net(), a._fused.flat, self.fields(a.network), self.DIMS, self.shape, a._target_flat)

    def buffers(self, t_len):
        return self.agent.task.buffers(t_len)

    def run(self, t_len):
        """One rollout launch on the current stream (after prepare(t_len)); returns the task's buffers of t_len."""
        io = self.IO()
        b = self.agent.task.fill_io(io, self.agent, t_len)
        io.step_counter, io.bootstrap = self.step_dev.data_ptr(), b['bootstrap'].data_ptr()
        self.fill_own(io)
        net = self.net_struct()
        getattr(lib, self.ENTRY)(ctypes.byref(net), ctypes.byref(io), stream_ptr())
        self.launches += 1
        return b
