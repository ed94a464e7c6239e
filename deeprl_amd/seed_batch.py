"""Many seeds of dqn_feature as lanes of the same device launches (csrc/dqn_mlp.hip and csrc/optim.hip: seed lanes).

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

What the lanes cannot be is named in a ValueError: an agent that stayed on the host path (dqn_mlp.why_not's reason: n_step > 1, a
PrioritizedReplay, another network, ...), the module-path update, fused_eval, an optimiser other than RMSprop, lanes that differ
in anything the launches share (first_mismatch), more than MAX_LANES seeds."""
import ctypes

import numpy as np
import torch

from . import dqn_mlp
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


def lane_signature(agent):
    """What the lanes' launches and the host's common decisions share, in the order first_mismatch names it."""
    cfg, rp, opt = agent.config, agent._inner_replay(), agent.optimizer
    g = opt.param_groups[0]
    return dict(shape=tuple(dqn_mlp.shape(agent.network)), sgd_update_frequency=int(cfg.sgd_update_frequency),
                batch=int(rp.batch_size), memory_size=int(rp.memory_size), schedule=_schedule_signature(cfg.random_action_prob),
                exploration_steps=cfg.exploration_steps, target_network_update_freq=cfg.target_network_update_freq,
                gradient_clip=cfg.gradient_clip, discount=float(cfg.discount),
                optimizer=(type(opt).__name__, g['lr'], g.get('alpha'), g.get('eps'), bool(g.get('centered', False))),
                double_q=bool(cfg.double_q), graph_update=getattr(cfg, 'graph_update', True) is not False)


def first_mismatch(signatures):
    """None when every lane's signature is lane 0's, else 'lane K differs from lane 0 in FIELD (A, lane 0: B)' of the first."""
    for k, sig in enumerate(signatures[1:], 1):
        for field, want in signatures[0].items():
            if sig.get(field) != want:
                return "lane %d differs from lane 0 in %s (%r, lane 0: %r)" % (k, field, sig.get(field), want)
    return None


def lane_why_not(agent):
    """None when `agent`, built with config.fused_dqn_feature on, can be a lane; else the first reason."""
    cfg = agent.config
    step = getattr(agent, '_feature', None)
    if type(step) is not dqn_mlp.Step:
        return dqn_mlp.why_not(agent) or "the agent runs on %s, not on the fused_dqn_feature path" % type(step).__name__
    if not dqn_mlp.Kind.fused_update(cfg, step.shape):
        return "config.fused_dqn_update is off: the module-path update has no lane form"
    if getattr(cfg, dqn_mlp.EVAL_SWITCH, False) is True:
        return "config.fused_eval is on: the evaluation launch has no lane form"
    if agent._fused.kind != 'rmsprop':
        return "the optimizer is not RMSprop: the lanes' clip + step launch is dra_clip_rmsprop_step_lanes"
    return None


class DQNFeatureSeeds:
    """See the module's docstring.  `make_config(seed)` -> a Config for DQNAgent (dqn_feature's); config.fused_dqn_feature is set
    here.  Surface: step(), total_steps (of every lane: they advance together), episodes(k), drain_episodes(), lane(k) -- the
    underlying agent, whose network, _target_flat, replay ring and save() see the lane's live buffers --, rng_tail(k) -- the
    lane's RandomState --, close()."""
    WARMUP = dqn_mlp.Step.WARMUP

    def __init__(self, make_config, seeds):
        from .agents import DQNAgent
        seeds = [int(s) for s in seeds]
        if not 1 <= len(seeds) <= MAX_LANES:
            raise ValueError("DQNFeatureSeeds runs 1 to %d seeds as lanes, not %d" % (MAX_LANES, len(seeds)))
        self.seeds, self.agents, self.rngs = seeds, [], []
        try:
            for seed in seeds:
                random_seed(seed)
                torch.manual_seed(seed)
                cfg = make_config(seed)
                cfg.fused_dqn_feature = True
                agent = DQNAgent(cfg)
                self.agents.append(agent)
                why = lane_why_not(agent)
                if why is not None:
                    raise ValueError("seed %d cannot run as a lane: %s" % (seed, why))
                rs = np.random.RandomState()
                rs.set_state(np.random.get_state())      # where the single run's draws would start
                self.rngs.append(rs)
            why = first_mismatch([lane_signature(a) for a in self.agents])
            if why is not None:
                raise ValueError("the lanes do not share one configuration: %s" % why)
            self._wire()
        except Exception:
            for a in self.agents:
                a.close()
            raise

    # -- construction: the lanes' buffers that become one, the tables ------------------------------------------------------
    def _wire(self):
        dev, n = Config.DEVICE, len(self.agents)
        steps = self.steps_ = [a._feature for a in self.agents]
        s0, cfg = steps[0], self.agents[0].config
        self.k, self.batch, self.cfg = s0.k, s0.batch, cfg
        if lib.dra_dqn_mlp_lanes_supported.raw(*s0.shape[:3], self.k, self.batch, s0.shape[3], n):
            raise ValueError("dra_dqn_mlp_*_lanes are not built for %d lanes of shape %r" % (n, (s0.shape, self.k, self.batch)))
        # ONE staged block of [n] per-lane blocks; every lane's Step sees its block through the views it had of its own
        lay = self.layout = lane_layout(self.k, self.batch)
        self._up = StagedUpload(n * lay['stride'], torch.uint8, dev)
        # the episode rings [n][3 cap + 1] and the error words [n] as one tensor each, and the rings' pinned twin
        cap3 = 3 * s0.vec.ring_cap + 1
        self._rings = torch.zeros((n, cap3), dtype=torch.float64, device=dev)
        self._rings_host = torch.zeros((n, cap3), dtype=torch.float64).pin_memory()
        self.err = torch.zeros(n, dtype=torch.int32, device=dev)
        self._draining = False
        for k, st in enumerate(steps):
            d = self._up.dev[k * lay['stride']:(k + 1) * lay['stride']]
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
        self.nets, self.act_ios = LaneTable(dqn_mlp.Net, n), LaneTable(dqn_mlp.ActIO, n)
        self.update_ios, self.opt_lanes, self.copy_lanes = LaneTable(dqn_mlp.UpdateIO, n), LaneTable(OptimLane, n), LaneTable(CopyLane, n)
        for k, (a, st) in enumerate(zip(self.agents, steps)):
            self.nets.rows[k] = st.net_struct()
            self.act_ios.rows[k] = st.act_io()
            io = dqn_mlp.UpdateIO()
            io.out_q_target, io.out_td, io.out_loss = st.q_target.data_ptr(), st.td.data_ptr(), st.loss.data_ptr()
            io.ring_frames, io.ring_actions, io.ring_rewards, io.ring_masks = st.ring.pointers()
            io.idx, io.grad, io.err, io.capacity = st.idx.data_ptr(), a._fused.flat.grad.data_ptr(), st.err.data_ptr(), st.capacity
            io.discount, io.batch, io.double_q = float(a.config.discount), self.batch, int(bool(a.config.double_q))
            self.update_ios.rows[k] = io
            f, o = a._fused, OptimLane()
            o.param, o.grad, o.square_avg, o.grad_avg = f.flat.flat.data_ptr(), f.flat.grad.data_ptr(), f.state1.data_ptr(), f.state2.data_ptr()
            o.out_norm, o.n = f.norm.data_ptr(), f.flat.numel
            self.opt_lanes.rows[k] = o
            c = CopyLane()
            c.dst, c.src, c.n = a._target_flat.flat.data_ptr(), f.flat.flat.data_ptr(), f.flat.numel
            self.copy_lanes.rows[k] = c
        self.regions = dict(act=Region("the dqn_feature lanes' acting launch", cfg, self.WARMUP),
                            learn=Region("the dqn_feature lanes' agent step", cfg, self.WARMUP))
        self.launches = self.agent_steps = 0

    # -- the launches --------------------------------------------------------------------------------------------------------
    def _act(self):
        lib.dra_dqn_mlp_act_lanes(self.nets.ptr, self.act_ios.ptr, len(self.agents), stream_ptr())
        self.launches += 1

    def _learn(self):
        n, h = len(self.agents), self.agents[0]._fused.hyper
        self._act()
        lib.dra_dqn_mlp_update_lanes(self.nets.ptr, self.update_ios.ptr, n, stream_ptr())
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
        if bad.any():
            raise dqn_mlp.DraError("dqn_feature lanes %r: staged ring slots / indices were outside the ring and have been clamped (%r)"
                                   % ([self.seeds[i] for i in np.nonzero(bad)[0]], bad[bad != 0].tolist()))

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

    def rng_tail(self, k):
        return self.rngs[k]

    def close(self):
        if self.agents:
            self.drain_episodes()
            for a in self.agents:
                a.close()
            self.agents = []
