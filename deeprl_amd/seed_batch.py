"""Many seeds of a cart-pole replay entry as lanes of the same device launches (csrc/seed_lanes.h, csrc/dqn_mlp.hip,
csrc/dist_mlp.hip and csrc/optim.hip: seed lanes): dqn_feature (DQNFeatureSeeds; with an n-step window: DQNReplayFeatureSeeds),
categorical_dqn_feature (CategoricalDQNFeatureSeeds) and quantile_regression_dqn_feature (QuantileRegressionDQNFeatureSeeds).

`DQNFeatureSeeds(make_config, seeds)` builds, per seed, an ordinary DQNAgent on the config.fused_dqn_feature path exactly as a user
would -- random_seed(seed), torch.manual_seed(seed), make_config(seed) -- so lane k's network, target, optimiser state,
environment, replay ring and np.random state ARE the single run's; the np.random state moves into a RandomState of the lane's
own.  `step()` is then one agent step of every lane: the schedule's epsilons, the learn / no-learn decision and the target-sync
cadence are common and computed once; each lane's draws come from its RandomState in the reference's order
(support.plan_actor_epsilon_greedy, then UniformReplay.advance / draw_indices) and all of them are staged in ONE block of per-lane
blocks (lane_layout) sent with one copy; dra_dqn_mlp_act_lanes, dra_dqn_mlp_update_lanes and dra_clip_rmsprop_step_lanes run lane
k as workgroup (x, k) on lane k's own structs -- the single launches' arithmetic, hence the single run's bits -- from two
graphs.Regions as dqn_mlp.Step has them (acting alone; acting + update + step); the target copy of every lane is one eager
launch between replays; the episode rings of all lanes are one tensor and drain with one copy.  Nothing here has a CPU or
eager-PyTorch form.

All of that but the head is FeatureSeeds, the base class: construction per seed, the RandomState hand-over, first_mismatch, the
staged block, rings and error words, prepare, step, the regions, the optimiser and copy tables, drain, check and close.  A
subclass names the agent class, the switch it sets, the module of its Step (dqn_mlp / dist_mlp: the Step type, why_not, the net,
act-io and update-io structs), how the update io's outputs are filled, the three library entries and what its lane_signature
holds beyond the common fields.  The two distributional classes run CategoricalDQNAgent / QuantileRegressionDQNAgent over
dist_mlp.Step on dra_dist_mlp_act_lanes / dra_dist_mlp_update_lanes (DistFeatureSeeds).

dqn_feature with an n-step window (n_step 1..8 over a UniformReplay) is DQNReplayFeatureSeeds, opt-in under the single path's own
switch as there: DQNFeatureSeeds keeps refusing n_step > 1, and zoo.run_seeds picks the new class (REPLAY_SEED_CLASSES) only with
fused_dqn_replay_feature=True among its keyword arguments.  Its lanes are DQNAgents over dqn_replay_mlp.Step
(config.fused_dqn_replay_feature, set here); acting and evaluation are dqn_mlp's lane launches as they are, the update is
dra_dqn_replay_mlp_update_lanes over the lane Steps' own replay_io(); the lanes share n_step and the replay's discount.  The host
draws honour the window already (UniformReplay.draw_indices); the device draws go through dra_np_mt_draw_window_lanes with the
batch's n_step.  A PrioritizedReplay stays refused by name: the prioritised draw (python's `random` per lane, the tree's launches)
and the priorities' commit (per-lane pending sets) have no lane form.

What the lanes cannot be is named in a ValueError: an agent that stayed on the host path (the module's why_not's reason: n_step >
1, a PrioritizedReplay, another network, ...), the module-path update, fused_eval on a lane's own config (below), an optimiser
other than RMSprop, lanes that differ in anything the launches share (first_mismatch), more than MAX_LANES seeds.

Evaluation is a property of the BATCH, not of one lane: `eval_lanes=True` (off by default; every head has it) moves each lane's
config.eval_env onto the device through the lane Step's own eval_vec(config.eval_episodes) -- a lane whose evaluation environment
cannot move is refused with a ValueError, lanes have no host evaluation to fall back to -- and `evaluate(n)` runs n greedy episodes
of every lane as ONE launch of dra_dqn_mlp_eval_lanes / dra_dist_mlp_eval_lanes (workgroup (0, lane) is the single evaluation
launch on the lane's row of the acting lanes' net table and of an io table; lanes end at different steps and wait for nobody) and
ONE copy back of one block [n_lanes][n + 1 + (n + 1) // 2], whatever the lane count, eagerly between the graph replays.
`eval_episodes()` is BaseAgent.eval_episodes of every lane: drain_episodes(), evaluate(config.eval_episodes) and each lane agent's
own _report_eval.  config.eval_episodes and the evaluation horizon join the lanes' signature.  Evaluation draws nothing from
np.random, so it composes with device_draws unchanged.  A lane config that sets config.fused_eval itself stays refused: that switch
asks for the single launch per agent.  On an eval_lanes batch `lane(k).eval_episodes()` and `lane(k).eval_episode()` raise a
RuntimeError that points to the batch's eval_episodes(): the lane's evaluation environment has retired from the host, and the
host loop must not step it.  (On a batch without eval_lanes they are the agent's own host evaluation, as before.)

`device_draws=True` (off by default; every head has it, it lives in FeatureSeeds) takes the lanes' draws on the device WITHOUT
changing the stream: each lane's RandomState.get_state() (key, pos; a cached Gaussian is refused) is uploaded once, and
dra_np_mt_draw_lanes (csrc/np_mt.hip), first launch of both regions, draws lane k's step from lane k's state in numpy's own
arithmetic -- randint's masked rejection, rand's two words, the twist when pos reaches 624 -- and fills the very blocks the act and
update lane kernels read (lane_layout stays the one source of the offsets).  prepare() then evaluates the schedule once, sends one
small common block (first slot, the ring's pos / size after the step's appends, the k epsilons: dra_np_mt_common) and keeps the
per-lane counters; it makes no numpy draw and stages nothing per lane, and last_draws is None -- fetch_draws(k) copies the last
step's values back from the lane's block.  rng_tail(k) and close() copy the lane's state back into rngs[k] first, so the generator
handed out stands where the single run's np.random stands.  A ring state without a valid index (over the batch's n-step
window) is refused with a ValueError before the step; shapes dra_np_mt_lanes_supported (a window class:
dra_np_mt_window_lanes_supported) rejects are refused at construction."""
import ctypes

import numpy as np
import torch

from . import dist_mlp, dqn_mlp, dqn_replay_mlp
from ._lib import lib, stream_ptr
from .graphs import Region
from .support import Config, StagedUpload, plan_actor_epsilon_greedy, random_seed

MAX_LANES = 64


class OptimLane(ctypes.Structure):
    """Mirror of dra_optim_lane (include/deeprl_amd.h)."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("square_avg", ctypes.c_void_p),
                ("grad_avg", ctypes.c_void_p), ("out_norm", ctypes.c_void_p), ("n", ctypes.c_int64)]


class CopyLane(ctypes.Structure):
    """Mirror of dra_copy_lane."""
    _fields_ = [("dst", ctypes.c_void_p), ("src", ctypes.c_void_p), ("n", ctypes.c_int64)]


class NpMtCommon(ctypes.Structure):
    """Mirror of dra_np_mt_common: what a step of the device draws shares among the lanes."""
    _fields_ = [("slot0", ctypes.c_int64), ("ring_pos", ctypes.c_int64), ("ring_size", ctypes.c_int64), ("eps", ctypes.c_double * 8)]


class NpMtState(ctypes.Structure):
    """Mirror of dra_np_mt_state: a lane's RandomState.get_state() as the draw kernel keeps it."""
    _fields_ = [("key", ctypes.c_uint32 * 624), ("pos", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


NP_MT_STATE_WORDS = ctypes.sizeof(NpMtState) // 4      # DRA_NP_MT_STATE_WORDS
NP_MT_ERR_BUDGET = 1 << 30                             # DRA_NP_MT_ERR_BUDGET


def np_mt_words(rs):
    """The get_state() of RandomState `rs` as the uint32 [NP_MT_STATE_WORDS] words of a dra_np_mt_state.  A state that holds a
    cached Gaussian is refused: the device draws have no Gaussian, and dropping the cached value would change the stream."""
    kind, key, pos, has_gauss, _ = rs.get_state()
    if kind != 'MT19937' or has_gauss != 0:
        raise ValueError("device_draws: the lane's np.random state %s, which the draw kernel cannot carry"
                         % ("is a %s's" % kind if kind != 'MT19937' else "holds a cached Gaussian (has_gauss != 0)"))
    words = np.zeros(NP_MT_STATE_WORDS, dtype=np.uint32)
    words[:624], words[624] = key, pos
    return words


def np_mt_restore(rs, words):
    """set_state of `rs` from the words of a dra_np_mt_state."""
    rs.set_state(('MT19937', np.array(words[:624], dtype=np.uint32), int(words[624]), 0, 0.0))
    return rs


def ring_after(pos, size, memory_size, k):
    """(pos, size) of a UniformReplay after advance(k)."""
    for _ in range(k):
        if pos >= size:
            size += 1
        pos = (pos + 1) % memory_size
    return pos, size


def valid_index_count(pos, size, n_step=1):
    """How many slots UniformReplay.valid_index accepts at history_length = 1 over a window of `n_step`."""
    return max(pos - n_step, 0) + max(size - n_step - pos, 0)


class LaneTable:
    """`n` structs of `cls` in pinned host memory, which the device maps at the same address: the lane entries check the rows on
    the host and their workgroups read them from where they are (`ptr`).  `rows[k] = struct` fills row k."""

    def __init__(self, cls, n):
        self.buf = torch.zeros(n * ctypes.sizeof(cls), dtype=torch.uint8).pin_memory()
        self.rows = (cls * n).from_address(self.buf.data_ptr())
        self.ptr = ctypes.c_void_p(self.buf.data_ptr())


def lane_layout(k, batch):
    """The staged block of ONE lane, dqn_mlp.Step's: int64 first slot | int64 indices [batch] | int64 random actions [k] | uint8
    flags [k] -> dict(idx, rand, flag: byte offsets inside the lane's block; size: its bytes; stride: from one lane's block to the
    next, `size` rounded up to 16 bytes)."""
    idx, rand = 8, 8 + 8 * batch
    flag = rand + 8 * k
    size = flag + (k + 7) // 8 * 8
    return dict(idx=idx, rand=rand, flag=flag, size=size, stride=(size + 15) // 16 * 16)


def _schedule_signature(s):
    return (type(s).__name__,) + tuple(sorted((k, v) for k, v in vars(s).items() if not callable(v)))


def lane_signature(agent, shape=None, **extra):
    """What the lanes' launches and the host's common decisions share, in the order first_mismatch names it.  `shape`: the
    network's shape where it is not dqn_mlp.shape's; `extra`: a head's own fields, named behind the common ones."""
    cfg, rp, opt = agent.config, agent._inner_replay(), agent.optimizer
    g = opt.param_groups[0]
    return dict(shape=tuple(dqn_mlp.shape(agent.network) if shape is None else shape), sgd_update_frequency=int(cfg.sgd_update_frequency),
                batch=int(rp.batch_size), memory_size=int(rp.memory_size), schedule=_schedule_signature(cfg.random_action_prob),
                exploration_steps=cfg.exploration_steps, target_network_update_freq=cfg.target_network_update_freq,
                gradient_clip=cfg.gradient_clip, discount=float(cfg.discount),
                optimizer=(type(opt).__name__, g['lr'], g.get('alpha'), g.get('eps'), bool(g.get('centered', False))),
                double_q=bool(cfg.double_q), graph_update=getattr(cfg, 'graph_update', True) is not False, **extra)


def first_mismatch(signatures):
    """None when every lane's signature is lane 0's, else 'lane K differs from lane 0 in FIELD (A, lane 0: B)' of the first."""
    for k, sig in enumerate(signatures[1:], 1):
        for field, want in signatures[0].items():
            if sig.get(field) != want:
                return "lane %d differs from lane 0 in %s (%r, lane 0: %r)" % (k, field, sig.get(field), want)
    return None


def eval_signature(agent):
    """What an eval_lanes batch asks its lanes to share on top of lane_signature: config.eval_episodes and the evaluation
    environment's horizon (read from the host environment, ahead of its move onto the device).  The kernels take both per lane;
    one configuration is what a sweep over seeds means, and first_mismatch names the lane that differs."""
    from .device_env import _RolloutVec
    cfg = agent.config
    return dict(eval_episodes=int(cfg.eval_episodes), eval_horizon=int(_RolloutVec._host_envs(cfg.eval_env, cfg)[0].horizon))


def lane_why_not(agent, module=dqn_mlp):
    """None when `agent`, built with the switch of `module`'s kind on (dqn_mlp: config.fused_dqn_feature; dist_mlp:
    config.fused_dist_feature; ReplayModule: config.fused_dqn_replay_feature), can be a lane; else the first reason.  config.fused_eval on a LANE's config is refused: it asks
    for the single evaluation launch, per agent.  Evaluation of lanes is a property of the batch -- FeatureSeeds(...,
    eval_lanes=True) evaluates every lane in one launch -- not of one lane's config."""
    cfg, kind = agent.config, module.Kind
    step = getattr(agent, '_feature', None)
    if type(step) is not module.Step:
        return module.why_not(agent) or "the agent runs on %s, not on the %s path" % (type(step).__name__, kind.SWITCH)
    if not kind.fused_update(cfg, step.shape):
        return "config.%s is off: the module-path update has no lane form" % kind.UPDATE_SWITCH
    if getattr(cfg, dqn_mlp.EVAL_SWITCH, False) is True:
        return "config.fused_eval is on: the evaluation launch has no lane form"
    if agent._fused.kind != 'rmsprop':
        return "the optimizer is not RMSprop: the lanes' clip + step launch is dra_clip_rmsprop_step_lanes"
    return None


class FeatureSeeds:
    """What the seed lanes of every head share: see the module's docstring.  `make_config(seed)` -> a Config for the subclass's
    agent class; its switch is set here; `device_draws`, `eval_lanes`: the module's docstring.  Surface: step(), evaluate(n),
    eval_episodes(), eval_returns, eval_lengths, eval_steps, eval_launches, eval_copies (eval_lanes), total_steps (of every lane:
    they advance together), episodes(k), drain_episodes(), lane(k) -- the underlying agent, whose network, _target_flat, replay ring and save() see the lane's live
    buffers --, rng_tail(k) -- the lane's RandomState --, fetch_draws(k), close().

    A subclass supplies ENTRY (the name in region labels and errors), MODULE (dqn_mlp or dist_mlp, or a namespace of the same
    names: Step, why_not, Kind, Net, ActIO, UpdateIO), the library entries ACT_LANES / UPDATE_LANES / LANES_SUPPORTED / EVAL_LANES,
    agent_class(), switch_on(config), signature(agent), update_outputs(io, step) and, where LANES_SUPPORTED takes more than the
    shape, lanes_supported_args(shape, n).  WINDOW: the lanes' replay has an n-step window, and the device draws go through the
    np_mt window entries with it (else: the 1-step entries, which are the window entries at n_step 1)."""
    WARMUP = dqn_mlp.Step.WARMUP
    ENTRY = MODULE = ACT_LANES = UPDATE_LANES = LANES_SUPPORTED = EVAL_LANES = None
    WINDOW = False

    # -- what a subclass supplies ------------------------------------------------------------------------------------------
    def agent_class(self):
        raise NotImplementedError

    def switch_on(self, cfg):
        """Sets the switches of the device path on a lane's Config, ahead of the agent's construction."""
        setattr(cfg, self.MODULE.Kind.SWITCH, True)

    def why_not(self, agent):
        return lane_why_not(agent, self.MODULE)

    def signature(self, agent):
        return lane_signature(agent)

    def update_outputs(self, io, st):
        """The update io's output pointers from lane Step `st`, as the Step's own update() sets them."""
        raise NotImplementedError

    def lanes_supported_args(self, shape, n):
        """LANES_SUPPORTED's arguments for `n` lanes of network shape `shape`."""
        return (*shape[:3], self.k, self.batch, *shape[3:self.MODULE.Kind.N_SUPPORTED], n)

    # -- construction ------------------------------------------------------------------------------------------------------
    def __init__(self, make_config, seeds, device_draws=False, eval_lanes=False):
        seeds = [int(s) for s in seeds]
        self.device_draws, self.eval_lanes = bool(device_draws), bool(eval_lanes)
        if not 1 <= len(seeds) <= MAX_LANES:
            raise ValueError("%s runs 1 to %d seeds as lanes, not %d" % (type(self).__name__, MAX_LANES, len(seeds)))
        agent_cls = self.agent_class()
        self.seeds, self.agents, self.rngs = seeds, [], []
        try:
            for seed in seeds:
                random_seed(seed)
                torch.manual_seed(seed)
                cfg = make_config(seed)
                self.switch_on(cfg)
                agent = agent_cls(cfg)
                self.agents.append(agent)
                why = self.why_not(agent)
                if why is not None:
                    raise ValueError("seed %d cannot run as a lane: %s" % (seed, why))
                why = agent._feature._eval_why_not(int(cfg.eval_episodes)) if self.eval_lanes else None
                if why is not None:      # (lanes have no host evaluation to fall back to)
                    raise ValueError("seed %d cannot run as a lane: fused evaluation: %s" % (seed, why))
                rs = np.random.RandomState()
                rs.set_state(np.random.get_state())      # where the single run's draws would start
                self.rngs.append(rs)
            why = first_mismatch([dict(self.signature(a), **(eval_signature(a) if self.eval_lanes else {})) for a in self.agents])
            if why is not None:
                raise ValueError("the lanes do not share one configuration: %s" % why)
            self._wire()
            if self.eval_lanes:
                self._wire_eval()
        except Exception:
            for a in self.agents:
                a.close()
            raise

    # -- the lanes' buffers that become one, the tables ----------------------------------------------------------------------
    def _wire(self):
        dev, n, m = Config.DEVICE, len(self.agents), self.MODULE
        steps = self.steps_ = [a._feature for a in self.agents]
        s0, cfg = steps[0], self.agents[0].config
        self.k, self.batch, self.cfg = s0.k, s0.batch, cfg
        self.n_step = int(self.agents[0]._inner_replay().n_step)      # (the lanes share it: the signature, or the 1-step kinds' why_not)
        if getattr(lib, self.LANES_SUPPORTED).raw(*self.lanes_supported_args(s0.shape, n)):
            raise ValueError("%s are not built for %d lanes of shape %r" % (self.ACT_LANES.replace("_act_", "_*_"), n, (s0.shape, self.k, self.batch)))
        # ONE staged block of [n] per-lane blocks; every lane's Step sees its block through the views it had of its own
        lay = self.layout = lane_layout(self.k, self.batch)
        if self.device_draws:
            # the draw kernel fills the lanes' blocks: a plain device tensor, the lanes' generators beside it, and the little the
            # lanes share in a step as the one staged upload
            dims = (n, self.k, self.batch, s0.shape[1], s0.capacity)
            if self.WINDOW and lib.dra_np_mt_window_lanes_supported.raw(*dims, self.n_step):
                raise ValueError("device_draws: dra_np_mt_draw_window_lanes is not built for %d lanes of k %d, batch %d, %d actions and a "
                                 "ring of %d slots over an n-step window of %d" % (dims + (self.n_step,)))
            if not self.WINDOW and lib.dra_np_mt_lanes_supported.raw(*dims):
                raise ValueError("device_draws: dra_np_mt_draw_lanes is not built for %d lanes of k %d, batch %d, %d actions and a ring "
                                 "of %d slots" % dims)
            self._up = None
            self._blocks = torch.zeros(n * lay['stride'], dtype=torch.uint8, device=dev)
            self._uploaded = np.stack([np_mt_words(rs) for rs in self.rngs])
            self._mt = torch.from_numpy(self._uploaded.view(np.int32)).to(dev)
            self._mt_stale = [False] * n      # whether rngs[k] lags behind the device's state of lane k
            self._learned = False             # whether the last prepared step updates
            self._common = StagedUpload(ctypes.sizeof(NpMtCommon), torch.uint8, dev)
        else:
            self._up = StagedUpload(n * lay['stride'], torch.uint8, dev)
        blocks = self._blocks if self.device_draws else self._up.dev
        # the episode rings [n][3 cap + 1] and the error words [n] as one tensor each, and the rings' pinned twin
        cap3 = 3 * s0.vec.ring_cap + 1
        self._rings = torch.zeros((n, cap3), dtype=torch.float64, device=dev)
        self._rings_host = torch.zeros((n, cap3), dtype=torch.float64).pin_memory()
        self.err = torch.zeros(n, dtype=torch.int32, device=dev)
        self._draining = False
        for k, st in enumerate(steps):
            d = blocks[k * lay['stride']:(k + 1) * lay['stride']]
            st.slot0 = d[:8].view(torch.int64)
            st.idx = d[lay['idx']:lay['rand']].view(torch.int64)
            st.random_action = d[lay['rand']:lay['flag']].view(torch.int64)
            st.explore = d[lay['flag']:lay['flag'] + self.k]
            st.err = self.err[k:k + 1]
            v = st.vec
            self._rings[k].copy_(v._ring_buf)
            v._ring_buf = self._rings[k]
            v.ep_ring = v._ring_buf[:cap3 - 1].view(v.ring_cap, 3)
            v.ep_count = v._ring_buf[cap3 - 1:].view(torch.int64)
            v.drain = lambda k=k: self._lane_rows(k)
        self.nets, self.act_ios = LaneTable(m.Net, n), LaneTable(m.ActIO, n)
        self.update_ios, self.opt_lanes, self.copy_lanes = LaneTable(m.UpdateIO, n), LaneTable(OptimLane, n), LaneTable(CopyLane, n)
        for k, (a, st) in enumerate(zip(self.agents, steps)):
            self.nets.rows[k] = st.net_struct()
            self.act_ios.rows[k] = st.act_io()
            io = m.UpdateIO()
            self.update_outputs(io, st)
            io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = st.ring.pointers()
            io.idx, io.grad, io.err, io.capacity = st.idx.data_ptr(), a._fused.flat.grad.data_ptr(), st.err.data_ptr(), st.capacity
            # (the bootstrap factor as Step.launch_update states it; x ** 1 is x)
            io.discount = float(a.config.discount) ** int(a.config.n_step)
            io.batch, io.double_q = self.batch, int(bool(a.config.double_q))
            self.update_ios.rows[k] = io
            f, o = a._fused, OptimLane()
            o.param, o.grad, o.square_avg, o.grad_avg = f.flat.flat.data_ptr(), f.flat.grad.data_ptr(), f.state1.data_ptr(), f.state2.data_ptr()
            o.out_norm, o.n = f.norm.data_ptr(), f.flat.numel
            self.opt_lanes.rows[k] = o
            c = CopyLane()
            c.dst, c.src, c.n = a._target_flat.flat.data_ptr(), f.flat.flat.data_ptr(), f.flat.numel
            self.copy_lanes.rows[k] = c
        self.regions = dict(act=Region("the %s lanes' acting launch" % self.ENTRY, cfg, self.WARMUP),
                            learn=Region("the %s lanes' agent step" % self.ENTRY, cfg, self.WARMUP))
        self.launches = self.agent_steps = 0

    # -- evaluation of every lane in one launch (eval_lanes) -------------------------------------------------------------------
    def _wire_eval(self):
        """Every lane's config.eval_env onto the device through the lane Step's own eval_vec (checked eligible in __init__), the
        io table, and a lane agent whose own eval_episodes() says where evaluation lives instead of stepping a retired host
        environment."""
        n_ep = int(self.cfg.eval_episodes)
        self.eval_vecs = [st.eval_vec(n_ep) for st in self.steps_]
        self.eval_ios = LaneTable(dqn_mlp.EvalIO, len(self.agents))
        self._eval_blocks = {}
        self.eval_launches = self.eval_copies = 0
        self.eval_returns = self.eval_lengths = self.eval_steps = None      # the last evaluation's
        for k, a in enumerate(self.agents):
            # (the evaluation reads the ONLINE parameters through the acting lanes' net table, self.nets: Kind.eval_net changes nothing
            # in net_struct()'s struct for the kinds that have lanes)
            a.eval_episodes = a.eval_episode = self._not_per_lane

    def _not_per_lane(self, *args, **kwargs):
        raise RuntimeError("%s: this agent is a lane of an eval_lanes batch, whose evaluation environment lives on the device and is "
                           "stepped by the batch's launch: call the batch's eval_episodes() (or evaluate(n)), not the lane's"
                           % self.ENTRY)

    def _eval_block(self, n):
        """Per episode count ONE device block [n_lanes][n + 1 + (n + 1) // 2] fp64 -- each row dqn_mlp.Step._eval_buffers' layout:
        fp64 returns [n] | int64 steps | int32 lengths [n] -- and its pinned twin: what an evaluation leaves comes back in one copy."""
        if n not in self._eval_blocks:
            shape = (len(self.agents), n + 1 + (n + 1) // 2)
            self._eval_blocks[n] = (torch.zeros(shape, dtype=torch.float64, device=Config.DEVICE),
                                    torch.zeros(shape, dtype=torch.float64).pin_memory())
        return self._eval_blocks[n]

    def evaluate(self, n=None):
        """`n` (default: config.eval_episodes) greedy episodes of EVERY lane's evaluation environment under the lane's online
        network, as ONE launch on the current stream (eagerly, outside both captured regions, behind whatever the steps queued)
        and ONE copy back, whatever the lane count -> the episodic returns, fp64 [n_lanes][n], each row what the single run's
        Step.evaluate(n) gives (kept in eval_returns).  eval_lengths [n_lanes][n] and eval_steps [n_lanes] hold the episodes' lengths
        and their sums.
        Nothing is drawn from np.random and no generator state is touched (the cart-pole's reset is a hash of seed and counter),
        with device_draws or without."""
        if not self.eval_lanes:
            raise dqn_mlp.DraError("%s lanes: evaluate() needs a batch built with eval_lanes=True" % self.ENTRY)
        n = int(self.cfg.eval_episodes if n is None else n)
        lanes, horizon = len(self.agents), self.eval_vecs[0].horizon
        if lib.dra_mlp_eval_lanes_supported.raw(n, horizon, lanes):
            raise dqn_mlp.DraError("%s is not built for %d lanes of %d episodes of at most %d steps" % (self.EVAL_LANES, lanes, n, horizon))
        dev, host = self._eval_block(n)
        for k, vec in enumerate(self.eval_vecs):
            io, row = dqn_mlp.EvalIO(), dev[k]
            io.env_state, io.env_counter, io.env_seed = vec.env_state.data_ptr(), vec.env_counter.data_ptr(), vec.env_seed.data_ptr()
            io.ep_steps, io.ep_return = vec.ep_steps.data_ptr(), vec.ep_return.data_ptr()
            io.out_return, io.out_steps, io.out_length = row.data_ptr(), row[n:].data_ptr(), row[n + 1:].data_ptr()
            io.horizon, io.n_episodes = vec.horizon, n
            self.eval_ios.rows[k] = io
        getattr(lib, self.EVAL_LANES)(self.nets.ptr, self.eval_ios.ptr, lanes, stream_ptr())
        self.eval_launches += 1
        host.copy_(dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        self.eval_copies += 1
        raw = host.numpy()
        self.eval_steps = raw[:, n].copy().view(np.int64)
        self.eval_lengths = np.ascontiguousarray(raw[:, n + 1:]).view(np.int32)[:, :n].copy()
        self.eval_returns = raw[:, :n].copy()
        return self.eval_returns

    def eval_episodes(self):
        """BaseAgent.eval_episodes of every lane: the pending training episodes first (drain_episodes, as the single run's
        eval_episodes does), then evaluate(config.eval_episodes) and per lane the agent's own _report_eval, so each lane's logger
        receives the 'episodic_return_test' line and scalar the single run writes -> the list of their dicts."""
        self.drain_episodes()
        returns = self.evaluate(self.cfg.eval_episodes)
        return [a._report_eval(returns[k]) for k, a in enumerate(self.agents)]

    # -- the launches --------------------------------------------------------------------------------------------------------
    def _draw(self, learn):
        """device_draws: the lanes' blocks filled by dra_np_mt_draw_lanes (WINDOW: dra_np_mt_draw_window_lanes with the batch's
        n_step) from the lanes' generators, ahead of the launches that read them."""
        lay = self.layout
        args = (self._mt.data_ptr(), self._blocks.data_ptr(), self._common.dev.data_ptr(), self.err.data_ptr(), len(self.agents), self.k,
                self.batch, self.steps_[0].shape[1], int(learn), lay['idx'], lay['rand'], lay['flag'], lay['stride'])
        if self.WINDOW:
            lib.dra_np_mt_draw_window_lanes(*args, self.n_step, stream_ptr())
        else:
            lib.dra_np_mt_draw_lanes(*args, stream_ptr())
        self.launches += 1

    def _act(self, learn=False):
        if self.device_draws:
            self._draw(learn)
        getattr(lib, self.ACT_LANES)(self.nets.ptr, self.act_ios.ptr, len(self.agents), stream_ptr())
        self.launches += 1

    def _learn(self):
        n, h = len(self.agents), self.agents[0]._fused.hyper
        self._act(learn=True)
        getattr(lib, self.UPDATE_LANES)(self.nets.ptr, self.update_ios.ptr, n, stream_ptr())
        lib.dra_clip_rmsprop_step_lanes(self.opt_lanes.ptr, n, float(self.cfg.gradient_clip or 0.0), float(h['lr']), float(h['alpha']),
                                        float(h['eps']), int(bool(h['centered'])), stream_ptr())

    def sync_targets(self):
        """DQN_agent.py:136-138 of every lane as one launch."""
        lib.dra_copy_f32_lanes(self.copy_lanes.ptr, len(self.agents), stream_ptr())

    # -- one agent step of every lane --------------------------------------------------------------------------------------
    def prepare(self):
        """dqn_mlp.Step.prepare of every lane: the schedule's epsilons once, then per lane the draws in the reference's order from
        the lane's RandomState and the host bookkeeping, staged in the one block and sent with one copy.  -> whether the step
        updates."""
        k, lay, cfg = self.k, self.layout, self.cfg
        a0 = self.agents[0]
        actor_steps = a0.actor._total_steps
        # plan_actor_epsilon_greedy calls the schedule once per transition at or behind exploration_steps: lane 0's is called,
        # the others replay its values and end where it ends
        eps = [cfg.random_action_prob() for t in range(k) if not actor_steps + t < cfg.exploration_steps]
        learn = a0.total_steps + k > cfg.exploration_steps
        if self.device_draws:
            return self._prepare_counters(eps, learn)
        raw = self._up.stage().numpy()
        for n, (agent, st, rs) in enumerate(zip(self.agents, self.steps_, self.rngs)):
            replay = iter(eps)
            explore, rand = plan_actor_epsilon_greedy(lambda: next(replay), k, st.shape[1], actor_steps, cfg.exploration_steps, rng=rs)
            if n:
                vars(agent.config.random_action_prob).update(vars(cfg.random_action_prob))
            agent.actor._total_steps += k
            rp = agent._inner_replay()
            slot0 = int(rp.pos)
            rp.advance(k)
            st.episodes.begin(k)
            agent.total_steps += k
            idx = rp.draw_indices(rng=rs) if learn else None
            blk = raw[n * lay['stride']:(n + 1) * lay['stride']]
            blk[:8].view(np.int64)[0] = slot0
            if idx is not None:
                blk[lay['idx']:lay['rand']].view(np.int64)[...] = idx
            blk[lay['rand']:lay['flag']].view(np.int64)[...] = rand
            blk[lay['flag']:lay['flag'] + k] = explore
            st.last_draws = (explore, rand, slot0, idx)
        self._up.send()
        return learn

    def _prepare_counters(self, eps, learn):
        """prepare() with device_draws: the common block (first slot, the ring's pos / size after the k appends, the k epsilons)
        staged and sent, then per lane the host bookkeeping alone -- no numpy draw, no per-lane staging."""
        k, cfg = self.k, self.cfg
        a0 = self.agents[0]
        rp0 = a0._inner_replay()
        slot0 = int(rp0.pos)
        pos, size = ring_after(slot0, rp0.size(), rp0.memory_size, k)
        if learn and valid_index_count(pos, size, self.n_step) == 0:
            raise ValueError("device_draws: a replay ring of size %d at pos %d holds no valid index%s, the minibatch's rejection loop "
                             "could not end" % (size, pos, " over an n-step window of %d" % self.n_step if self.WINDOW else ""))
        c = NpMtCommon.from_buffer(self._common.stage().numpy())
        c.slot0, c.ring_pos, c.ring_size = slot0, pos, size
        behind = k - len(eps)      # transitions below exploration_steps: epsilon is 1 and the schedule is not called
        for t in range(k):
            c.eps[t] = 1.0 if t < behind else eps[t - behind]
        self._common.send()
        for n, (agent, st) in enumerate(zip(self.agents, self.steps_)):
            if n:
                vars(agent.config.random_action_prob).update(vars(cfg.random_action_prob))
            agent.actor._total_steps += k
            agent._inner_replay().advance(k)
            st.episodes.begin(k)
            agent.total_steps += k
            st.last_draws = None
            self._mt_stale[n] = True
        self._learned = learn
        return learn

    def step(self):
        learn = self.prepare()
        a0, cfg = self.agents[0], self.cfg
        region, body = (self.regions['learn'], self._learn) if learn else (self.regions['act'], self._act)
        key = a0._fused.hyper_signature() if learn else None
        if region.due(key) and (region.graph is not None or region.capture(body, key)):
            region.replay()
        else:
            body()
        if learn:
            for a, st in zip(self.agents, self.steps_):
                a._fused.steps += 1
                a.last_loss = st.loss
        # DQN_agent.py:136-138, after the update of the step: eager, between graph replays
        if a0.total_steps / cfg.sgd_update_frequency % cfg.target_network_update_freq == 0:
            self.sync_targets()
        self.agent_steps += 1
        if self.agent_steps % max(1, int(getattr(cfg, 'episode_drain_interval', 64))) == 0:
            self.drain_episodes()

    # -- what comes back -------------------------------------------------------------------------------------------------------
    @property
    def total_steps(self):
        """Environment steps of EVERY lane so far (the lanes advance together; the aggregate is len(seeds) times this)."""
        return self.agents[0].total_steps

    def _fetch(self):
        self._rings_host.copy_(self._rings, non_blocking=True)
        torch.cuda.current_stream().synchronize()

    def _lane_rows(self, k):
        """DeviceCartPoleVec.drain of lane k over the shared tensor (ONE copy for all lanes; inside drain_episodes() the copy has
        been made)."""
        if not self._draining:
            self._fetch()
        return self.steps_[k].vec.rows_since_drain(self._rings_host[k].numpy())

    def check(self):
        """dqn_mlp.Step.check of every lane with one copy."""
        bad = self.err.cpu().numpy()
        if (bad & NP_MT_ERR_BUDGET).any():
            raise dqn_mlp.DraError("%s lanes %r: the draw kernel gave up on a draw after its budget of words (err %r)"
                                   % (self.ENTRY, [self.seeds[i] for i in np.nonzero(bad & NP_MT_ERR_BUDGET)[0]], bad[bad != 0].tolist()))
        if bad.any():
            raise dqn_mlp.DraError("%s lanes %r: staged ring slots / indices were outside the ring and have been clamped (%r)"
                                   % (self.ENTRY, [self.seeds[i] for i in np.nonzero(bad)[0]], bad[bad != 0].tolist()))

    def drain_episodes(self):
        """One device-to-host copy for all lanes -> per lane the (step, return) pairs of the episodes that ended since the last
        drain (each lane's agent logs its 'episodic_return_train' lines, as the single run does)."""
        self.check()
        self._fetch()
        self._draining = True
        try:
            return [st.episodes.drain() for st in self.steps_]
        finally:
            self._draining = False

    def episodes(self, k):
        """(step, return) of lane k's training episodes since the previous call."""
        self.drain_episodes()
        return self.steps_[k].episodes.episodes()

    def lane(self, k):
        return self.agents[k]

    def _lane_block(self, k):
        lay = self.layout
        torch.cuda.current_stream().synchronize()
        return self._blocks[k * lay['stride']:(k + 1) * lay['stride']].cpu().numpy()

    def fetch_draws(self, k, learned=None):
        """device_draws: (explore, random_action, first slot, indices) of lane k's last step, copied from the lane's device block
        -- last_draws' counterpart, for tests and debugging.  The indices are None when the step did not update (`learned`: whether
        it did, where the caller knows better than the last prepare())."""
        if not self.device_draws:
            return self.steps_[k].last_draws
        lay, blk = self.layout, self._lane_block(k)
        learned = self._learned if learned is None else learned
        idx = blk[lay['idx']:lay['rand']].view(np.int64).copy() if learned else None
        return (blk[lay['flag']:lay['flag'] + self.k].astype(np.bool_), blk[lay['rand']:lay['flag']].view(np.int64).copy(),
                int(blk[:8].view(np.int64)[0]), idx)

    def mt_words(self, k):
        """device_draws: the dra_np_mt_state words of lane k as they stand on the device (one copy behind a stream sync)."""
        torch.cuda.current_stream().synchronize()
        return self._mt[k].cpu().numpy().view(np.uint32)

    def rng_tail(self, k):
        """Lane k's RandomState, standing where the single run's np.random stands.  With device_draws the lane's state is copied
        back from the device first (one copy behind a stream sync); the device keeps its own copy and goes on from it, so draws
        made from the returned generator do not move the lane."""
        if self.device_draws and self._mt_stale[k]:
            np_mt_restore(self.rngs[k], self.mt_words(k))
            self._mt_stale[k] = False
        return self.rngs[k]

    def close(self):
        if self.agents:
            self.drain_episodes()
            for k in range(len(self.agents) if self.device_draws else 0):
                self.rng_tail(k)
            for a in self.agents:
                a.close()
            self.agents = []


class DQNFeatureSeeds(FeatureSeeds):
    """Seeds of dqn_feature: DQNAgent over dqn_mlp.Step with config.fused_dqn_feature set here, on dra_dqn_mlp_act_lanes and
    dra_dqn_mlp_update_lanes.  `make_config(seed)` -> a Config for DQNAgent (dqn_feature's).  The surface is FeatureSeeds'."""
    ENTRY, MODULE = 'dqn_feature', dqn_mlp
    ACT_LANES, UPDATE_LANES, LANES_SUPPORTED = 'dra_dqn_mlp_act_lanes', 'dra_dqn_mlp_update_lanes', 'dra_dqn_mlp_lanes_supported'
    EVAL_LANES = 'dra_dqn_mlp_eval_lanes'

    def agent_class(self):
        from .agents import DQNAgent
        return DQNAgent

    def update_outputs(self, io, st):
        io.out_q_target, io.out_td, io.out_loss = st.q_target.data_ptr(), st.td.data_ptr(), st.loss.data_ptr()


class ReplayModule:
    """What FeatureSeeds reads from MODULE for dqn_feature under config.fused_dqn_replay_feature: the Step, its kind, why_not and
    the update io are dqn_replay_mlp's; the net and the acting io are dqn_mlp's as they are (the window changes nothing in acting)."""
    Net, ActIO = dqn_mlp.Net, dqn_mlp.ActIO
    UpdateIO, Step, Kind = dqn_replay_mlp.UpdateIO, dqn_replay_mlp.Step, dqn_replay_mlp.WindowKind
    why_not = staticmethod(dqn_replay_mlp.why_not)


def replay_lane_signature(agent):
    """lane_signature with what the window's launches share on top: n_step (one launch, one window; the draws' validity test) and
    the replay's discount (the fold's factor)."""
    rp = agent._inner_replay()
    return lane_signature(agent, n_step=int(rp.n_step), replay_discount=float(rp.discount))


class DQNReplayFeatureSeeds(FeatureSeeds):
    """Seeds of dqn_feature with an n-step window (n_step 1..8 over a UniformReplay): DQNAgent over dqn_replay_mlp.Step with
    config.fused_dqn_replay_feature set here, on dra_dqn_mlp_act_lanes, dra_dqn_replay_mlp_update_lanes and (eval_lanes)
    dra_dqn_mlp_eval_lanes; with device_draws the minibatch's indices are drawn valid over the window
    (dra_np_mt_draw_window_lanes).  The lanes share n_step and the replay's discount on top of DQNFeatureSeeds' signature.  A
    PrioritizedReplay stays refused: the prioritised draw (python's `random` per lane, the tree's launches) and the priorities'
    commit (per-lane pending sets) have no lane form, although the update launch itself takes priorities per lane.
    `make_config(seed)` -> a Config for DQNAgent (dqn_feature's).  The surface is FeatureSeeds'."""
    ENTRY, MODULE, WINDOW = 'dqn_feature', ReplayModule, True
    ACT_LANES, UPDATE_LANES = 'dra_dqn_mlp_act_lanes', 'dra_dqn_replay_mlp_update_lanes'
    LANES_SUPPORTED, EVAL_LANES = 'dra_dqn_replay_mlp_lanes_supported', 'dra_dqn_mlp_eval_lanes'

    def agent_class(self):
        from .agents import DQNAgent
        return DQNAgent

    def why_not(self, agent):
        if isinstance(getattr(agent, '_feature', None), dqn_replay_mlp.PerStep):
            return ("the replay is a PrioritizedReplay: the prioritised draw and the priorities' commit have no lane form")
        return lane_why_not(agent, self.MODULE)

    def signature(self, agent):
        return replay_lane_signature(agent)

    def lanes_supported_args(self, shape, n):
        return (*shape[:3], self.k, self.batch, shape[3], self.n_step, n)

    def update_outputs(self, io, st):
        """The whole io as the lane Step's own replay_io() states it -- the outputs, the window and the fold's discount have one
        source --; _wire fills the ring, the indices and the scalars over it, as Step.launch_update does."""
        ctypes.memmove(ctypes.byref(io), ctypes.byref(st.replay_io()), ctypes.sizeof(io))


def dist_lane_signature(agent):
    """lane_signature with what the distributional launches share on top: the head kind, the atoms per action (the launches' LDS
    size follows from lane 0's) and the categorical support (per-lane data to the kernels, but one configuration is what a sweep
    over seeds means)."""
    shp = dist_mlp.shape(agent.network)
    return lane_signature(agent, shape=shp[:4], head=shp[4], n_atoms=shp[5], support=dist_mlp.support(agent.config, shp[4]))


class DistFeatureSeeds(FeatureSeeds):
    """Seeds of categorical_dqn_feature / quantile_regression_dqn_feature (the two subclasses below name the agent class):
    CategoricalDQNAgent / QuantileRegressionDQNAgent over dist_mlp.Step on dra_dist_mlp_act_lanes and dra_dist_mlp_update_lanes.
    config.fused_dist_feature is set here, and config.fused_dist_update is set to True where it is unset: the module-path update
    has no lane form, so the lanes always run the update kernel.  For quantiles that is the single run's default; for the
    categorical head the unset default of a SINGLE run is the module update (dist_mlp.Kind.fused_update), so a
    categorical lane is -- to the bit -- the single run with config.fused_dist_update = True, and equals the default single run only
    within that form's float32 error.  An explicit config.fused_dist_update = False is refused, as fused_eval, an optimiser other
    than RMSprop and lanes that differ in head, atoms per action or categorical support are."""
    MODULE = dist_mlp
    ACT_LANES, UPDATE_LANES, LANES_SUPPORTED = 'dra_dist_mlp_act_lanes', 'dra_dist_mlp_update_lanes', 'dra_dist_mlp_lanes_supported'
    EVAL_LANES = 'dra_dist_mlp_eval_lanes'
    AGENT = None

    def agent_class(self):
        from . import agents
        return getattr(agents, self.AGENT)

    def switch_on(self, cfg):
        kind = dist_mlp.Kind
        setattr(cfg, kind.SWITCH, True)
        if getattr(cfg, kind.UPDATE_SWITCH, None) is None:
            setattr(cfg, kind.UPDATE_SWITCH, True)

    def signature(self, agent):
        return dist_lane_signature(agent)

    def update_outputs(self, io, st):
        io.out_loss, io.out_loss_vec = st.loss.data_ptr(), st.loss_vec.data_ptr()
        io.out_q_next, io.out_target = st.q_next.data_ptr(), st.target.data_ptr()


class CategoricalDQNFeatureSeeds(DistFeatureSeeds):
    """DistFeatureSeeds over CategoricalDQNAgent (categorical_dqn_feature)."""
    ENTRY, AGENT = 'categorical_dqn_feature', 'CategoricalDQNAgent'


class QuantileRegressionDQNFeatureSeeds(DistFeatureSeeds):
    """DistFeatureSeeds over QuantileRegressionDQNAgent (quantile_regression_dqn_feature)."""
    ENTRY, AGENT = 'quantile_regression_dqn_feature', 'QuantileRegressionDQNAgent'


# zoo.run_seeds: the entries with a lane form
SEED_CLASSES = {c.ENTRY: c for c in (DQNFeatureSeeds, CategoricalDQNFeatureSeeds, QuantileRegressionDQNFeatureSeeds)}
# ... and the ones picked instead where a keyword of run_seeds sets the class's own switch (fused_dqn_replay_feature=True)
REPLAY_SEED_CLASSES = {c.ENTRY: c for c in (DQNReplayFeatureSeeds,)}
