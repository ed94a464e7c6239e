"""Python host of the fused DQN learner (deeprl_amd/csrc/learner.hip).

`DQNLearner` binds a VanillaNet(NatureConvBody) pair (online / target), the optimiser
hyper-parameters and an HBM replay ring to the C-ABI learner: after that, one whole agent step
(DQN_agent.py:101-138: 4 actor transitions + sample + update) is ONE ctypes call that replays
captured hipGraphs and never synchronises with the host.  All RNG stays on the host in the
reference's draw order.

`DQNLearnerBench` is the synthetic-workload driver bench.py times (BASELINE configs[1]).
"""
import ctypes
import os

import numpy as np
import torch

from . import ops
from ._lib import DraError, lib
from .optim import FlatParams
from .replay import draw_uniform_indices   # noqa: F401  (the vectorised rejection loop lives with UniformReplay; re-exported here)
from .support import Config

_ORDER = ["body.conv1.weight", "body.conv1.bias", "body.conv2.weight", "body.conv2.bias", "body.conv3.weight",
          "body.conv3.bias", "body.fc4.weight", "body.fc4.bias", "fc_head.weight", "fc_head.bias"]


# CU-partitioned stream pairs live for the whole process, one pair per (device, actor CUs): PyTorch's pinned-memory
# allocator keeps events recorded on them (non_blocking copies), so destroying such a stream while the process
# runs crashes later inside the HIP runtime; every learner on the device shares the pair.
_PARTITIONED_STREAMS = {}


class DqnConfig(ctypes.Structure):
    """Mirror of dra_dqn_config (include/deeprl_amd.h)."""
    _fields_ = [("batch", ctypes.c_int32), ("n_actions", ctypes.c_int32), ("double_q", ctypes.c_int32),
                ("ksplit", ctypes.c_int32), ("centered", ctypes.c_int32), ("env_done_period", ctypes.c_int32),
                ("gamma_n", ctypes.c_float), ("gradient_clip", ctypes.c_float), ("lr", ctypes.c_float),
                ("alpha", ctypes.c_float), ("eps", ctypes.c_float), ("replay_eps", ctypes.c_float),
                ("replay_alpha", ctypes.c_float), ("variant", ctypes.c_int32), ("u8_coef", ctypes.c_double),
                ("n_params", ctypes.c_int64), ("conv_end", ctypes.c_int64), ("ring_capacity", ctypes.c_int64),
                ("env_seed", ctypes.c_uint64), ("offset", ctypes.c_int64 * 10),
                ("head_kind", ctypes.c_int32), ("n_atoms", ctypes.c_int32), ("v_min", ctypes.c_float),
                ("v_max", ctypes.c_float), ("optimizer", ctypes.c_int32), ("beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("reserved", ctypes.c_int32)]


HEAD_VANILLA, HEAD_CATEGORICAL, HEAD_QUANTILE = 0, 1, 2        # DRA_HEAD_*
OPT_RMSPROP, OPT_ADAM = 0, 1                                     # DRA_OPT_*
_HEAD_PARAM = {HEAD_VANILLA: "fc_head", HEAD_CATEGORICAL: "fc_categorical", HEAD_QUANTILE: "fc_quantiles"}


class StepParams(ctypes.Structure):
    """Mirror of dra_dqn_step_params (include/deeprl_amd.h)."""
    _fields_ = [("slot", ctypes.c_int64 * 8), ("counter", ctypes.c_int64 * 8), ("rcounter", ctypes.c_int64 * 8),
                ("random_action", ctypes.c_int32 * 8), ("store_action", ctypes.c_int32 * 8), ("dice", ctypes.c_float * 8),
                ("epsilon", ctypes.c_float * 8), ("stack_age", ctypes.c_int32 * 8), ("n_env", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("idx", ctypes.c_int64 * 1024)]


def _param_order(head_kind=HEAD_VANILLA):
    return _ORDER[:8] + [_HEAD_PARAM[head_kind] + ".weight", _HEAD_PARAM[head_kind] + ".bias"]


def _ordered_params(net, head_kind=HEAD_VANILLA):
    named = dict(net.named_parameters())
    order = _param_order(head_kind)
    missing = [k for k in order if k not in named]
    if missing or len(named) != len(order):
        raise DraError("the fused learner supports VanillaNet / CategoricalNet / QuantileNet over NatureConvBody; "
                       "parameters found: %s" % sorted(named))
    return [named[k] for k in order]


class DQNLearner:
    def __init__(self, network, target_network, ring, batch, n_actions, gamma_n, gradient_clip, lr, alpha, eps,
                 centered=True, double_q=False, u8_coef=1.0 / 255, replay_eps=0.01, replay_alpha=0.5, ksplit=16,
                 env_seed=0, env_done_period=800, variant=-1, cu_partition=True, head_kind=HEAD_VANILLA, n_atoms=0,
                 v_min=0.0, v_max=0.0, optimizer=OPT_RMSPROP, betas=(0.9, 0.999)):
        """`variant`: DRA_VAR_* kernel-selection mask (ops.VAR_*); -1 = the process default (ops.set_tuning).
        `cu_partition=False` drops DRA_VAR_CU_PARTITION from it: a caller that never runs the device actor
        concurrently (in-order mode, host environments) wants every CU for the update chain."""
        self.network, self.target_network, self.ring = network, target_network, ring
        self.head_kind = int(head_kind)
        po, pt = _ordered_params(network, self.head_kind), _ordered_params(target_network, self.head_kind)
        self.flat = FlatParams(po, koc=(po[0], po[2], po[4]))        # conv segment first, conv weights in KOC
        self.target_flat = FlatParams(pt, koc=(pt[0], pt[2], pt[4]))
        self.state1 = torch.zeros_like(self.flat.flat)
        self.state2 = torch.zeros_like(self.flat.flat)
        self.variant = int(variant) if int(variant) >= 0 else ops.get_tuning()
        if not cu_partition:
            self.variant &= ~ops.VAR_CU_PARTITION
        if self.head_kind != HEAD_VANILLA:   # (dra_dqn_learner_create does the same: the launches that fold the VanillaNet
            # head into a neighbouring kernel do not exist for the distributional heads)
            self.variant = (self.variant | ops.VAR_ACTOR_V2) & ~(ops.VAR_ACTOR_V3 | ops.VAR_ACTOR_FUSED_HEAD |
                                                                 ops.VAR_GATHER_IN_GRAPH)
            if os.environ.get("DRA_ACTOR_DIST_FUSED", "1") == "0":
                self.variant &= ~ops.VAR_ACTOR_FUSED_CONV1
        variant = self.variant
        cfg = DqnConfig()
        cfg.batch, cfg.n_actions, cfg.double_q, cfg.ksplit, cfg.centered = batch, n_actions, int(double_q), ksplit, int(centered)
        cfg.gamma_n, cfg.gradient_clip, cfg.lr, cfg.alpha, cfg.eps = gamma_n, gradient_clip or 0.0, lr, alpha, eps
        cfg.replay_eps, cfg.replay_alpha, cfg.u8_coef = replay_eps, replay_alpha, u8_coef
        cfg.env_seed, cfg.env_done_period = env_seed, env_done_period
        cfg.head_kind, cfg.n_atoms, cfg.v_min, cfg.v_max = self.head_kind, int(n_atoms), float(v_min), float(v_max)
        cfg.optimizer, cfg.beta1, cfg.beta2 = int(optimizer), float(betas[0]), float(betas[1])
        cfg.variant = int(variant)
        cfg.n_params = self.flat.numel
        cfg.conv_end = self.flat.offsets[6]                          # start of fc4.weight
        cfg.ring_capacity = ring.capacity
        for i, o in enumerate(self.flat.offsets):
            cfg.offset[i] = o
        self.cfg = cfg
        self.batch, self.n_actions = batch, n_actions
        h = ctypes.c_void_p()
        lib.dra_dqn_learner_create(ctypes.byref(h), ring.h, ctypes.byref(cfg), ctypes.c_void_p(self.flat.flat.data_ptr()),
                                   ctypes.c_void_p(self.target_flat.flat.data_ptr()),
                                   ctypes.c_void_p(self.flat.grad.data_ptr()), ctypes.c_void_p(self.state1.data_ptr()),
                                   ctypes.c_void_p(self.state2.data_ptr()))
        self.h = h
        ps = [ctypes.c_void_p() for _ in range(8)]
        lib.dra_dqn_learner_buffers(h, *[ctypes.byref(p) for p in ps])
        w = ops._wrap_device_pointer
        self.idx = w(ps[0].value, batch, torch.int64)
        self.sampling_prob = w(ps[1].value, batch + 1, torch.float32)    # [batch] = the PER exponent beta of the update
        self._loss_per = w(ps[2].value, 1, torch.float32)
        self.norm = w(ps[3].value, 1, torch.float32)
        # head outputs of the online net on the sampled states: q [B, A], or logits / quantiles [B, A, N]
        self.n_out = n_actions * (int(n_atoms) if self.head_kind != HEAD_VANILLA else 1)
        self.q = w(ps[4].value, batch * self.n_out, torch.float32)
        self.q = self.q.view(batch, n_actions) if self.head_kind == HEAD_VANILLA else self.q.view(batch, n_actions, int(n_atoms))
        self.delta = w(ps[5].value, batch, torch.float32)
        self.prio = w(ps[6].value, batch, torch.float32)
        self.actor_q = w(ps[7].value, n_actions, torch.float32)
        self.update_cus = self.actor_cus = None      # CUs of the two chains' streams (None: the whole device)
        if self.variant & ops.VAR_CU_PARTITION:
            try:
                self.stream, self.actor_stream = self._partitioned_streams()
            except DraError as e:           # e.g. a device mode without CU masking: plain streams, same results
                import warnings
                warnings.warn("CU-partitioned streams unavailable (%s); using plain streams" % (e,))
                self.stream, self.actor_stream = torch.cuda.Stream(), torch.cuda.Stream()
                self.update_cus = self.actor_cus = None
        else:
            self.stream = torch.cuda.Stream()                        # graphs cannot capture on the NULL stream
            self.actor_stream = torch.cuda.Stream()
        if self.actor_cus:
            # (DRA_VAR_ACTOR_PERSIST: the one-launch agent step needs 32 co-resident workgroups, one per CU of the actor's stream)
            lib.dra_dqn_learner_set_actor_cus(self.h, int(self.actor_cus))
        # DRA_VAR_TARGET_AHEAD: the target net's forward of the NEXT update runs on a third stream (the update's CU partition)
        self.ahead_stream = None
        if self.variant & ops.VAR_TARGET_AHEAD:
            self.ahead_stream = self._ahead_stream()
            lib.dra_dqn_learner_set_ahead_stream(self.h, self._sp(self.ahead_stream))
            if not self.ahead_stats()["active"]:
                self.ahead_stream = None
        self.params = StepParams()
        self._idx_view = np.ctypeslib.as_array(self.params.idx)[:batch]
        self._k = 0

    def _partitioned_streams(self):
        """Update stream / actor stream on disjoint CU sets (DRA_VAR_CU_PARTITION).  On MI355X mask bit i is CU
        (i // 32) of shader engine (i // 8) % 4 of XCD i % 8 (tools/probe_cu_mask.py), and a workgroup's XCD is
        fixed by the dispatcher (round robin), so the first DRA_ACTOR_CUS (default 1/8 of the device = 32) bits give
        the actor chain the same 4 CUs (1 per shader engine) in every XCD and the update chain the other 28.
        End of round 2 (actor conv2 / conv3 split over two workgroups, ring-direct update: the update chain is the longer one):
        64 -> 8 347, 40 -> 8 383, 32 -> 8 490, 24 -> 7 709 updates/s on one box (profiles/r02zj_ab_actor_cus.json).
        Round 2 (4-launch env step, 8-wave batch-1 convolutions): 96 -> 6876, 64 -> 7438, 56 -> 7082, 48 -> 6379 updates/s on
        one box (profiles/r02f_*): at 192 CUs conv2 / conv3 backward (384 workgroups at 2 per CU) and the optimizer fit
        ONE round of workgroups, at 160 they do not (phase traces, profiles/r02b_*)."""
        import os
        n_cu = torch.cuda.get_device_properties(Config.DEVICE).multi_processor_count
        n_act = max(8, min(n_cu - 8, int(os.environ.get("DRA_ACTOR_CUS", str(n_cu // 8)))))   # 32 of 256
        key = (Config.DEVICE.index, n_act)
        self.update_cus, self.actor_cus = n_cu - n_act, n_act
        if key in _PARTITIONED_STREAMS:
            return _PARTITIONED_STREAMS[key]
        actor_bits = set(range(n_act))
        words = (n_cu + 31) // 32
        out = []
        with torch.cuda.device(Config.DEVICE):      # the stream is created on the current HIP device
            for bits in (set(range(n_cu)) - actor_bits, actor_bits):
                mask = (ctypes.c_uint32 * words)()
                for b in bits:
                    mask[b // 32] |= 1 << (b % 32)
                h = ctypes.c_void_p()
                lib.dra_stream_create_masked(ctypes.byref(h), mask, words)
                out.append(torch.cuda.ExternalStream(h.value, device=Config.DEVICE))
        _PARTITIONED_STREAMS[key] = out
        return out

    def _ahead_stream(self):
        """A second stream on the update stream's CU set (or a plain one without DRA_VAR_CU_PARTITION)."""
        if not self.update_cus:
            return torch.cuda.Stream()
        key = (Config.DEVICE.index, self.actor_cus, "ahead")
        if key not in _PARTITIONED_STREAMS:
            n_cu = self.update_cus + self.actor_cus
            words = (n_cu + 31) // 32
            mask = (ctypes.c_uint32 * words)()
            for b in range(self.actor_cus, n_cu):
                mask[b // 32] |= 1 << (b % 32)
            h = ctypes.c_void_p()
            with torch.cuda.device(Config.DEVICE):
                lib.dra_stream_create_masked(ctypes.byref(h), mask, words)
            _PARTITIONED_STREAMS[key] = torch.cuda.ExternalStream(h.value, device=Config.DEVICE)
        return _PARTITIONED_STREAMS[key]

    def stage_next_indices(self, idx_next):
        """DRA_VAR_TARGET_AHEAD: the minibatch indices of the update AFTER the coming step() (numpy int64 [batch])."""
        a = np.ascontiguousarray(idx_next, dtype=np.int64)
        lib.dra_dqn_learner_stage_next_indices(self.h, a.ctypes.data_as(ctypes.c_void_p), int(a.size))

    def ahead_stats(self):
        out = (ctypes.c_int64 * 8)()
        lib.dra_dqn_learner_ahead_stats(self.h, out)
        return {"from_stash": int(out[0]), "in_line": int(out[1]), "skipped_slot_hazard": int(out[2]),
                "index_mismatch": int(out[3]), "active": bool(out[4])}

    def close(self):
        if self.h:
            lib.dra_dqn_learner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sp(self, stream=None):
        return ctypes.c_void_p((stream or self.stream).cuda_stream)

    @property
    def loss(self):
        """Reduced loss of the last update: mean(0.5 * delta^2) recovered from the TD errors (DQN_agent.py:78-79); for the
        distributional heads `delta` holds the per-sample KL / quantile-Huber loss and this is its mean."""
        if self.head_kind == HEAD_QUANTILE:
            return self._loss_per[0]          # the quantile loss kernel reduces it itself (one entry per target quantile)
        if self.head_kind != HEAD_VANILLA:
            return self.delta.mean()
        return self.delta.pow(2).mul(0.5).mean()

    def upload_indices(self, idx):
        """numpy int64[batch] -> the learner's device idx buffer (async, the learner's pinned staging)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        lib.dra_dqn_learner_upload_indices(self.h, idx.ctypes.data_as(ctypes.c_void_p), int(idx.shape[0]), self._sp())

    def upload_sampling_prob(self, prob, beta):
        """PER: numpy sampling probabilities [batch] + the importance exponent -> the learner's device buffer (async,
        pinned staging).  The kernels read beta from device memory, so the PER update replays from a captured graph."""
        prob = np.ascontiguousarray(prob, dtype=np.float64)   # (f64 -> f32 in the C call, as tensor(transitions.sampling_prob) does)
        lib.dra_dqn_learner_upload_sampling_prob(self.h, prob.ctypes.data_as(ctypes.c_void_p), int(prob.shape[0]), float(beta),
                                                 self._sp())

    def update(self, idx=None, use_graph=True, sampling_prob=None, beta=0.0):
        """One gradient update (gather + forward/backward graph + optimizer) on the update stream.  sampling_prob (numpy
        [batch]) makes it a PER update with importance exponent beta (DQN_agent.py:120-127)."""
        if idx is not None:
            self.upload_indices(idx)
        per = sampling_prob is not None
        if per:
            self.upload_sampling_prob(np.asarray(sampling_prob), beta)
        lib.dra_dqn_learner_update(self.h, int(use_graph), int(per), -1.0 if per else 0.0, self._sp())

    def update_async(self, idx=None, use_graph=True, sampling_prob=None, beta=0.0):
        """update() for the async actor over a HOST environment: the optimizer also mirrors the new parameters into the
        actor copy q_host_async() reads one update later (dra_dqn_learner_update_async)."""
        if idx is not None:
            self.upload_indices(idx)
        per = sampling_prob is not None
        if per:
            self.upload_sampling_prob(np.asarray(sampling_prob), beta)
        lib.dra_dqn_learner_update_async(self.h, int(use_graph), int(per), -1.0 if per else 0.0, self._sp())

    def q_host_async(self, state):
        """q(state) on the ACTOR stream from the parameter copy of the update before the most recent one: the forward of
        agent step t+1 runs while update t trains (BaseAgent.py:142-162, async_actor=True with a host emulator)."""
        state = np.ascontiguousarray(state, dtype=np.uint8)
        if state.size != 4 * 7056:
            raise DraError("q_host_async: expected a uint8 [4,84,84] observation, got shape %s" % (state.shape,))
        q = np.empty(self.n_actions, dtype=np.float32)
        lib.dra_dqn_learner_q_host_async(self.h, state.ctypes.data_as(ctypes.c_void_p), q.ctypes.data_as(ctypes.c_void_p),
                                         self._sp(self.actor_stream), self._sp())
        return q

    def set_env_steps(self, slots, counters, random_actions, dices, epsilons, store=True, rcounters=None, ages=None):
        """Describes the next env transitions.  rcounters: counter whose hashes give the reward / mask stored with each
        slot (default: the frame's own counter); ages: observations of the same episode before each one, capped at 3
        (default 3 = the actor's stack is the last 4 ring frames)."""
        p = self.params
        n = len(slots)
        p.n_env = n
        for e in range(n):
            p.slot[e], p.counter[e] = int(slots[e]), int(counters[e])
            p.rcounter[e] = int(counters[e] if rcounters is None else rcounters[e])
            p.random_action[e], p.dice[e], p.epsilon[e] = int(random_actions[e]), float(dices[e]), float(epsilons[e])
            p.store_action[e] = int(store)
            p.stack_age[e] = 3 if ages is None else int(ages[e])

    def act(self, use_graph=True, stream=None):
        """Runs the env transitions currently described by self.params (set_env_steps)."""
        lib.dra_dqn_learner_act(self.h, ctypes.byref(self.params), int(use_graph), self._sp(stream))

    def step(self, idx, do_update=True, async_actor=False):
        """One agent step: the env transitions in self.params + one update on `idx`."""
        if idx is not None:
            self._idx_view[:] = idx
        lib.dra_dqn_learner_step(self.h, ctypes.byref(self.params), int(do_update), self._sp(),
                                 self._sp(self.actor_stream) if async_actor else None)

    def set_per(self, per, beta):
        """The next in-order step() applies PER importance weights (exponent beta) from self.sampling_prob and leaves the
        new priorities in self.prio."""
        lib.dra_dqn_learner_set_per(self.h, int(bool(per)), float(beta))

    def set_per_chain2(self, tree, stat, blocks, rng_words):
        """PrioritizedReplay.sample() on the device (dra_sumtree_per_chain2): four pinned dra_per_chain2_io blocks and the
        pinned ring of Mersenne-Twister words; before the first prioritized update."""
        lib.dra_dqn_learner_set_per_chain2(self.h, tree.h, ctypes.c_void_p(stat.data_ptr()),
                                           *[ctypes.c_void_p(ctypes.addressof(b)) for b in blocks],
                                           ctypes.c_void_p(rng_words.data_ptr()))

    def per_chain2_seed(self, tree_idx, data_idx, prob, beta, rng_cursor, seq):
        """The NEXT update's minibatch from the host (first prioritized update / resume)."""
        t = np.ascontiguousarray(tree_idx, dtype=np.int64)
        d = np.ascontiguousarray(data_idx, dtype=np.int64)
        p = np.ascontiguousarray(prob, dtype=np.float64)
        lib.dra_dqn_learner_per_chain2_seed(self.h, t.ctypes.data_as(ctypes.c_void_p), d.ctypes.data_as(ctypes.c_void_p),
                                            p.ctypes.data_as(ctypes.c_void_p), float(beta), int(rng_cursor), int(seq), self._sp())

    def per_chain2_wait(self, slot, seq, timeout_us=20_000_000):
        lib.dra_dqn_learner_per_chain2_wait(self.h, int(slot), int(seq), int(timeout_us))

    def step_update(self):
        """First half of an async step() whose prioritized minibatch is already in device memory: the update."""
        lib.dra_dqn_learner_step_update(self.h, ctypes.byref(self.params), self._sp(), self._sp(self.actor_stream))

    def step_actor(self, idx):
        """Second half: the next agent step's transitions; idx = the indices of the update just issued (hazard check)."""
        self._idx_view[:] = idx
        lib.dra_dqn_learner_step_actor(self.h, ctypes.byref(self.params), self._sp(), self._sp(self.actor_stream))

    def next_slot(self):
        q = ctypes.c_int()
        lib.dra_dqn_learner_next_slot(self.h, ctypes.byref(q))
        return q.value

    def sync_loss(self):
        lib.dra_dqn_learner_sync_loss(self.h)

    def wait_loss(self, stream):
        """`stream` waits until the TD errors / new priorities of the PER update issued last exist (its backward pass and
        optimizer are still running then)."""
        lib.dra_dqn_learner_wait_loss(self.h, self._sp(stream))

    def keep_minibatch(self, keep):
        """Checkers: with the ring-direct update (VAR_RING_DIRECT) no gathered minibatch exists; keep=True makes the pipelined
        step also gather it into the buffers last_minibatch() returns."""
        lib.dra_dqn_learner_keep_minibatch(self.h, int(bool(keep)))

    def sync_target(self):
        lib.dra_dqn_learner_sync_target(self.h, self._sp())

    def q_host(self, state):
        """q(state) for a host environment: uint8 [4,84,84] observation (numpy) -> float32 [n_actions] numpy.
        Batch-1 forward of the online parameters on the update stream, synchronous (DQN_agent.py:29-33)."""
        state = np.ascontiguousarray(state, dtype=np.uint8)
        if state.size != 4 * 7056:
            raise DraError("q_host: expected a uint8 [4,84,84] observation, got shape %s" % (state.shape,))
        q = np.empty(self.n_actions, dtype=np.float32)
        lib.dra_dqn_learner_q_host(self.h, state.ctypes.data_as(ctypes.c_void_p), q.ctypes.data_as(ctypes.c_void_p),
                                   self._sp())
        return q

    def profile(self):
        """Per-kernel-group milliseconds of one eager update (HIP events on the launch stream)."""
        n = lib.dra_dqn_learner_kernel_count.raw()
        out = (ctypes.c_float * (n + 1))()
        lib.dra_dqn_learner_profile(self.h, out, n + 1, self._sp())
        names = []
        for k in range(n):
            buf = ctypes.create_string_buffer(32)
            lib.dra_dqn_learner_kernel_name(k, buf, 32)
            names.append(buf.value.decode())
        res = dict(zip(names, [float(v) for v in out[:n]]))
        res["_event_bracket"] = float(out[n])      # two event records with nothing in between (the bracket's own cost)
        return res

    def kernel_replay(self, name, reps=64):
        """Kernel group `name` of the update alone: `reps` dependent launches in one captured graph between two events.
        Returns (us per launch incl. one in-graph boundary, us per launch of an EMPTY kernel in the same form); the
        difference is the kernel's own duration (what rocprofv3 reports), measured live."""
        n = lib.dra_dqn_learner_kernel_count.raw()
        for k in range(n):
            buf = ctypes.create_string_buffer(32)
            lib.dra_dqn_learner_kernel_name(k, buf, 32)
            if buf.value.decode() == name:
                out = (ctypes.c_float * 2)()
                lib.dra_dqn_learner_kernel_replay(self.h, k, int(reps), out, self._sp())
                return float(out[0]), float(out[1])
        raise DraError("kernel_replay: no kernel group named %r" % (name,))

    def chain_replay(self, which, reps=64):
        """The chained forward (which="fwd") or backward ("bwd") launch of the update alone, `reps` times in one captured graph
        (each followed / preceded by the one-thread epoch launch).  Returns (us per repetition, us per repetition with an empty
        kernel in the chain launch's place); the difference is the chained kernel's own duration, live."""
        out = (ctypes.c_float * 2)()
        lib.dra_dqn_learner_chain_replay(self.h, {"fwd": 0, "bwd": 1}[which], int(reps), out, self._sp())
        return float(out[0]), float(out[1])

    CHAIN_COUNTER_CLASSES = ("fwd_conv1_to_conv2", "fwd_conv2_to_conv3", "bwd_conv3_dgrad", "bwd_conv2_dgrad", "bwd_conv3_wgrad",
                             "bwd_conv2_wgrad", "bwd_fc4_dgrad")

    def chain_set_epoch(self, epoch):
        """Test aid (dra_dqn_learner_chain_set_epoch): the chained launches' never-reset 32-bit arrival counters and their epoch
        word as they stand after `epoch` updates.  Returns {counter class: arrivals per epoch} of the classes this learner's
        launches use, plus "target_ahead": whether the target-ahead chains were set as well.  Synchronises."""
        out = (ctypes.c_int64 * 8)()
        lib.dra_dqn_learner_chain_set_epoch(self.h, int(epoch), out, 8, self._sp())
        res = {k: int(out[i]) for i, k in enumerate(self.CHAIN_COUNTER_CLASSES) if out[i]}
        res["target_ahead"] = bool(out[7])
        return res

    def synchronize(self):
        # (DRA_VAR_DEFER_FC4: a pending fc4 segment of the last optimizer step is completed first -- after this call the
        # parameters, the optimizer state and the actor copies are what optimizer.step() of DQN_agent.py:133 left)
        lib.dra_dqn_learner_flush(self.h, self._sp())
        self.stream.synchronize()
        self.actor_stream.synchronize()

    def host_stats(self, reset=True):
        """Host-side accounting of dra_dqn_learner_step since the last reset: number of calls, mean microseconds inside the
        C call, and of those the microseconds BLOCKED on a pinned staging slot, i.e. waiting for the GPU (back-pressure: a
        loop whose calls never block is host-bound)."""
        out = (ctypes.c_double * 3)()
        lib.dra_dqn_learner_host_stats(self.h, out, int(reset))
        n = max(1.0, out[0])
        return {"calls": int(out[0]), "call_us": 1e6 * out[1] / n, "blocked_on_gpu_us": 1e6 * out[2] / n}

    def lane_stats(self):
        """DRA_VAR_FLAG_SYNC: {'steps', 'entries', 'hazard_bumps', 'host_waits'} of the event-free lane since creation."""
        out = (ctypes.c_int64 * 12)()
        lib.dra_dqn_learner_lane_stats(self.h, out)
        n = max(1, int(out[0]))
        return {"steps": int(out[0]), "entries": int(out[1]), "hazard_bumps": int(out[2]), "host_waits": int(out[3]),
                "host_us_per_step": {"pacing_wait": out[4] / n / 1e3, "index_staging": out[5] / n / 1e3,
                                     "update_launches": out[6] / n / 1e3, "actor_launch": out[7] / n / 1e3,
                                     "whole_call": out[8] / n / 1e3}}

    def path_flags(self):
        """The code paths this learner resolved (dra_dqn_learner_path_flags; read-only, for checkers): `late`, `defer`, `fchain`,
        `bchain`, `fs`, `ah` as decided at creation; `per2_ride`, `head_chain`, `head_pf` as of the last launch issued or captured;
        `head_launches` VanillaNet head launches issued or captured so far; `variant` the resolved DRA_VAR_* mask; `timed_out` a
        bounded device-side wait gave up (what the next step / update reports as DRA_ETIMEDOUT)."""
        out = (ctypes.c_int64 * 12)()
        lib.dra_dqn_learner_path_flags(self.h, out)
        keys = ("late", "defer", "fchain", "bchain", "fs", "ah", "per2_ride", "head_chain", "head_pf")
        res = {k: bool(out[i]) for i, k in enumerate(keys)}
        res["head_launches"], res["variant"], res["timed_out"] = int(out[9]), int(out[10]), bool(out[11])
        return res

    def invalidate_actor_copy(self):
        """The parameters were changed from outside (checkpoint load): the async actor's copies are reseeded on the next step."""
        lib.dra_dqn_learner_invalidate_actor_copy(self.h)

    def export_state(self):
        """CPU copies, in the MODULE's layout and keyed like state_dict(), of everything an update reads and writes:
        {'params', 'target', 'square_avg', 'grad_avg'} -> {name: tensor}.  (The flat buffers keep the conv weights
        as [(c,kh,kw)][oc]; this undoes that.)  Used by checkpointing and by the parity checkers; synchronises."""
        self.synchronize()
        torch.cuda.synchronize()
        names = _param_order(self.head_kind)
        net_p = dict(self.network.named_parameters())

        def per_tensor(buf):
            out = {}
            for k in names:
                p = net_p[k]
                o = self.flat.offset_of(p)
                v = buf[o:o + p.numel()]
                if p.dim() == 4 and not p.is_contiguous():      # KOC storage -> [oc, c, kh, kw]
                    oc, c, kh, kw = p.shape
                    v = v.view(c, kh, kw, oc).permute(3, 0, 1, 2)
                else:
                    v = v.view(p.shape)
                out[k] = v.detach().cpu().contiguous().clone()
            return out

        return {"params": per_tensor(self.flat.flat), "target": per_tensor(self.target_flat.flat),
                "square_avg": per_tensor(self.state1), "grad_avg": per_tensor(self.state2),   # RMSprop's names
                "state1": per_tensor(self.state1), "state2": per_tensor(self.state2)}         # Adam: exp_avg, exp_avg_sq

    # -- true resume ---------------------------------------------------------------------------
    def _resume_buffers(self):
        n = lib.dra_dqn_learner_resume_buffer_count.raw()
        out = []
        for i in range(n):
            p, nb = ctypes.c_void_p(), ctypes.c_int64()
            name = ctypes.create_string_buffer(32)
            lib.dra_dqn_learner_resume_buffer(self.h, i, ctypes.byref(p), ctypes.byref(nb), name, 32)
            if p.value and nb.value:
                out.append((name.value.decode(), ops._wrap_device_pointer(p.value, nb.value, torch.uint8)))
        return out

    def resume_state(self):
        """Everything of the learner a bit-exact continuation in a FRESH process needs: the flat parameter / target /
        optimizer-state buffers in their device layout (KOC conv weights: no conversion, no rounding), the learner-internal
        device buffers (optimizer step count, the actor's rotating parameter copies, the actor parameter-block ring and its
        counter, the pending observation, ...) and the host-side pipeline counters.  Synchronises first."""
        self.synchronize()
        torch.cuda.synchronize()
        counters = (ctypes.c_int64 * 16)()
        lib.dra_dqn_learner_resume_counters(self.h, counters, 16, 0)
        return dict(flat=self.flat.flat.detach().cpu().clone(), target=self.target_flat.flat.detach().cpu().clone(),
                    state1=self.state1.cpu().clone(), state2=self.state2.cpu().clone(),
                    buffers={k: v.cpu().clone() for k, v in self._resume_buffers()}, counters=list(counters),
                    variant=self.variant, n_params=self.flat.numel)

    def load_resume_state(self, st):
        """Into a fresh learner of the same configuration, before its first step."""
        if st["variant"] != self.variant or st["n_params"] != self.flat.numel:
            raise DraError("resume state of another learner configuration (variant %d / %d parameters, this one %d / %d)"
                           % (st["variant"], st["n_params"], self.variant, self.flat.numel))
        self.synchronize()
        torch.cuda.synchronize()
        self.flat.flat.copy_(st["flat"])
        self.target_flat.flat.copy_(st["target"])
        self.state1.copy_(st["state1"])
        self.state2.copy_(st["state2"])
        mine = dict(self._resume_buffers())
        for k, v in st["buffers"].items():
            if k not in mine or mine[k].numel() != v.numel():
                raise DraError("resume buffer %r does not exist in this learner" % k)
            mine[k].copy_(v)
        counters = (ctypes.c_int64 * 16)(*st["counters"])
        lib.dra_dqn_learner_resume_counters(self.h, counters, 16, 1)
        torch.cuda.synchronize()

    def last_minibatch(self):
        """(state, next_state, action, reward, mask) device tensors of the most recently issued update (views of the
        learner's own gather buffers; synchronize() first).  For checkers."""
        ps = [ctypes.c_void_p() for _ in range(5)]
        lib.dra_dqn_learner_last_minibatch(self.h, *[ctypes.byref(p) for p in ps])
        w, b = ops._wrap_device_pointer, self.batch
        return (w(ps[0].value, b * 4 * 7056, torch.uint8).view(b, 4, 84, 84), w(ps[1].value, b * 4 * 7056, torch.uint8).view(b, 4, 84, 84),
                w(ps[2].value, b, torch.int64), w(ps[3].value, b, torch.float32), w(ps[4].value, b, torch.float32))


def actor_randomness_block(rs, n_actions, k):
    """k pairs (randint(n_actions, size=1)[0], rand(1)[0]) of RandomState `rs` -- the epsilon-greedy draws of k env steps in
    the reference's order (torch_utils.py:51-58) -- from ONE call for 3 k raw 32-bit words: for a power-of-two n_actions the
    legacy bounded draw is `word & (n_actions - 1)` (its rejection loop never rejects) and rand() is
    ((a >> 5) * 2^26 + (b >> 6)) / 2^53 of the next two words.  The stream position afterwards is the scalar calls' one.
    Returns None when n_actions is not a power of two (the masked rejection consumes a data-dependent number of words)."""
    if n_actions < 1 or (n_actions & (n_actions - 1)) or n_actions > (1 << 31):
        return None
    if n_actions == 1:                                             # randint(1) consumes no word
        w = rs.randint(0, 1 << 32, size=2 * k, dtype=np.uint32).reshape(k, 2)
        return np.zeros(k, dtype=np.int64), ((w[:, 0] >> 5) * 67108864.0 + (w[:, 1] >> 6)) / 9007199254740992.0
    w = rs.randint(0, 1 << 32, size=3 * k, dtype=np.uint32).reshape(k, 3)
    return (w[:, 0] & np.uint32(n_actions - 1)).astype(np.int64), ((w[:, 1] >> 5) * 67108864.0 + (w[:, 2] >> 6)) / 9007199254740992.0


# numpy view of dra_dqn_step_params' head (everything before idx), one record per agent step
_STEP_HEAD_FIELDS = [("slot", "<i8", 8), ("counter", "<i8", 8), ("rcounter", "<i8", 8), ("random_action", "<i4", 8),
                     ("store_action", "<i4", 8), ("dice", "<f4", 8), ("epsilon", "<f4", 8), ("stack_age", "<i4", 8), ("n_env", "<i4", 1)]
_STEP_PARAMS_DTYPE = np.dtype({"names": [f[0] for f in _STEP_HEAD_FIELDS],
                               "formats": [(f[1], (f[2],)) if f[2] > 1 else f[1] for f in _STEP_HEAD_FIELDS],
                               "offsets": [getattr(StepParams, f[0]).offset for f in _STEP_HEAD_FIELDS],
                               "itemsize": ctypes.sizeof(StepParams)})


class SyntheticEpisodeStream:
    """Host-side shadow of ONE device-resident synthetic Atari environment: the counters, episode boundaries, rewards
    and returns envs.SyntheticAtari + DummyVecEnv's auto-reset (envs.py:126-150 of the reference) would produce, computed
    from the same counter hashes -- no device round trip.  For each transition it yields what the device kernels need
    (dra_dqn_step_params): counter of the observation acted on, counter whose hash gives the reward / done of leaving it,
    and the number of earlier observations of the same episode (the frame stack repeats the first frame after a reset)."""

    def __init__(self, seed, counter0=0, done_period=800, history=4):
        self.seed, self.done_period, self.history = int(seed), int(done_period), int(history)
        self.next_counter = int(counter0)
        self.c = None
        self.age = 0
        self.ret = 0.0
        self._cache_base = None

    def state_dict(self):
        return dict(next_counter=self.next_counter, c=self.c, age=self.age, ret=self.ret)

    def load_state_dict(self, st):
        self.next_counter, self.c, self.age, self.ret = st["next_counter"], st["c"], st["age"], st["ret"]
        self._cache_base = None

    def _reset(self):
        self.c = self.next_counter          # SyntheticAtari.reset(): one new frame, repeated `history` times
        self.next_counter += 1
        self.age = 0
        self.ret = 0.0

    def _reward_done(self, counter):
        """synthetic_reward_done(counter), hashed 4096 counters at a time (the scalar numpy hash is ~15 us per transition:
        more than the whole device-side agent step of four transitions and one update)."""
        base = self._cache_base
        if base is None or not (base <= counter < base + 4096):
            from .envs import synthetic_reward_done_vec
            base = self._cache_base = counter
            r, d = synthetic_reward_done_vec(np.arange(base, base + 4096, dtype=np.int64), np.full(4096, self.seed, dtype=np.int64),
                                             np.full(4096, self.done_period, dtype=np.int64))
            self._cache_r, self._cache_d = r.tolist(), d.tolist()
        return self._cache_r[counter - base], self._cache_d[counter - base]

    def transition(self):
        """-> (counter, rcounter, stack_age, reward, done, info) of the next transition (SyntheticAtari.step)."""
        if self.c is None:
            self._reset()
        counter, age = self.c, self.age
        rc = self.next_counter              # step(): reward / done hashed from the counter of the frame it generates
        reward, done = self._reward_done(rc)
        self.next_counter += 1
        self.ret += reward
        info = {'episodic_return': self.ret if done else None}
        if done:
            self._reset()                   # DummyVecEnv: the post-step frame is dropped, the stack restarts
        else:
            self.c = rc
            self.age = min(age + 1, self.history - 1)
        return counter, rc, age, reward, done, info


class DeviceActorPipeline:
    """DQNAgent.step() for a device-resident environment (DQN_agent.py:101-138): per call `n_env` actor transitions
    (forward, epsilon-greedy, environment step, replay feed) and one update, as ONE C call.

    async_actor=False: transitions then update, in order, every random draw from the GLOBAL np.random stream in the
    reference's order (torch_utils.py:51-58 per transition, then replay.py:92-103) -- the parity mode.
    async_actor=True (the reference's dqn_pixel setting, BaseAgent.py:108-182): the two-stream pipeline of
    csrc/learner.hip; the actor runs one agent step ahead on its own CU partition, its randomness comes from its own
    RandomState (the reference's actor process has its own np.random state too), parameter blocks are generated 16
    agent steps ahead."""
    AHEAD = 16

    def __init__(self, learner, replay, stream, n_actions, n_env, epsilon_fn, async_actor, actor_seed=None, beta_fn=None):
        self.L, self.rp, self.stream = learner, replay, stream
        self.per = hasattr(replay, 'draw')          # PrioritizedReplay: one host round trip per step (the draw)
        self.beta_fn = beta_fn
        # the priority tree's kernels (adds of the new transitions, stratified descent, write-back) are single-workgroup
        # latency chains of ~20 dependent levels each; they depend on the previous UPDATE only, so they run on their own
        # stream underneath the actor's forward passes
        self.tree_stream = torch.cuda.Stream() if self.per else None
        # PER + async (the ring-direct pipeline, minibatches up to 1024): the whole of sample() -- write-back, the next step's adds,
        # descent, valid_index filter, padding -- runs INSIDE the update and hands the next minibatch over in device memory
        # (dra_sumtree_per_chain2, replay.DeviceDraw): no host wait at all.  chain = 2 names that form (0: the round-2
        # tree-stream form, the fallback for other kernel variants / larger minibatches; round 3's intermediate form 1 -- the
        # host between two updates -- was removed in round 4)
        need2 = (ops.VAR_PIPE_GATHER | ops.VAR_ACTOR_PARAMS | ops.VAR_GATHER_ON_UPDATE | ops.VAR_RING_DIRECT | ops.VAR_ACTOR_RING)
        mode = 2 if (self.per and async_actor and (learner.variant & need2) == need2 and replay.batch_size <= 1024) else 0
        self.chain = mode
        self._dd = None                       # replay.DeviceDraw (mode 2)
        self.A, self.n_env, self.epsilon_fn, self.async_actor = int(n_actions), int(n_env), epsilon_fn, bool(async_actor)
        self.rs = np.random.RandomState(actor_seed) if async_actor else np.random
        self.capacity = replay.memory_size
        self.slot = replay.pos               # slot the next generated transition goes to
        self.pending = []                    # per issued-but-unreported agent step: list of (reward, done, info)
        self.pushed = self.issued = 0
        self.primed = False
        v = learner.variant
        need = ops.VAR_ACTOR_RING | ops.VAR_PIPE_GATHER | ops.VAR_ACTOR_PARAMS
        self.ring_mode = async_actor and (v & need) == need and not (v & (ops.VAR_ACTOR_V3 | ops.VAR_GATHER_IN_GRAPH))
        if async_actor and not self.ring_mode:
            raise DraError("the async device pipeline needs the default kernel variant (actor parameter ring)")

    def state_dict(self):
        """Host side of the pipeline between two agent steps: where the next transition goes, the (reward, done, info) of
        the agent steps issued ahead, how far ahead the parameter blocks have been generated / issued, and the actor's own
        random stream."""
        chain_prev = None
        if self._dd is not None and self._dd.active:
            dd = self._dd
            dd.release()                       # python `random` is the reference's again; the newest draw is the next update's
            chain_prev = (dd.next_tree_idx.tolist(), dd.next_p.tolist(), dd.next_total, dd.next_beta)
        return dict(slot=self.slot, pending=[list(p) for p in self.pending], pushed=self.pushed, issued=self.issued,
                    primed=self.primed, rs=(self.rs.get_state() if self.async_actor else None), stream=self.stream.state_dict(),
                    chain_prev=chain_prev)

    def sync_host(self):
        """Host bookkeeping caught up with the device; python's `random` where the reference's would be (DeviceDraw.release)."""
        if self._dd is not None and self._dd.active:
            self._dd.release()

    def load_state_dict(self, st):
        self.slot, self.pushed, self.issued, self.primed = st["slot"], st["pushed"], st["issued"], st["primed"]
        self.pending = [[tuple(x) for x in p] for p in st["pending"]]
        if self.async_actor:
            self.rs.set_state(st["rs"])
        self.stream.load_state_dict(st["stream"])
        if st.get("chain_prev") is not None:
            # a saved draw has already consumed python's `random`: dropping it would silently fork the resumed run
            if self.chain != 2:
                raise DraError("the checkpoint holds a pending device-side prioritized draw (chain_prev) but this pipeline "
                               "draws on the host: resume with the same async_actor / replay configuration it was saved with")
            from .replay import DeviceDraw
            if self._dd is None:
                self._dd = DeviceDraw(self.rp, self.L)
            prev = tuple(st["chain_prev"])
            if len(prev) == 3:
                # written by the retired chain mode 1: no importance exponent in the record, and guessing one (the schedule's
                # start value, say) would silently change the first resumed update's weights once beta has annealed
                raise DraError("the checkpoint's pending prioritized draw (chain_prev) has no importance exponent: it was written "
                               "by a round-3 build; save it again with this version (load it there, step once, save_full)")
            if len(prev) != 4:
                raise DraError("unrecognised chain_prev record of %d fields in the checkpoint" % len(prev))
            idx, p, total, beta = prev
            self._dd.start(idx, p, total, float(beta))

    def _block(self):
        """Host side of one agent step's transitions -> (StepParams head filled in learner.params, infos)."""
        slots, counters, rcs, ages, ras, dices, epss, infos = [], [], [], [], [], [], [], []
        for _ in range(self.n_env):
            c, rc, age, reward, done, info = self.stream.transition()
            eps = self.epsilon_fn()                                  # DQN_agent.py:34-39, once per transition
            ras.append(int(self.rs.randint(self.A, size=1)[0]))      # epsilon_greedy, 2-D branch: randint, (argmax), rand
            dices.append(float(self.rs.rand(1)[0]))
            slots.append(self.slot)
            counters.append(c); rcs.append(rc); ages.append(age); epss.append(eps)
            infos.append((reward, done, info))
            self.slot = (self.slot + 1) % self.capacity
        self.L.set_env_steps(slots, counters, ras, dices, epss, rcounters=rcs, ages=ages)
        return infos

    def _push(self, n=None):
        """Generates and uploads the parameter blocks of the next n agent steps.  Async mode fills the n blocks as arrays: the
        actor's randomness of all n x n_env transitions in one call on its own RandomState (actor_randomness_block: the scalar
        calls' stream word for word), the per-transition python left is the episode shadow and the epsilon schedule -- the
        per-field loop cost ~25 us of host time per agent step, a fifth of the device-side step."""
        L = self.L
        n = self.AHEAD if n is None else int(n)
        ne = self.n_env
        rnd = actor_randomness_block(self.rs, self.A, n * ne) if (self.async_actor and ne <= 8) else None
        if rnd is None:
            blocks = (StepParams * n)()
            for i in range(n):
                self.pending.append(self._block())
                ctypes.memmove(ctypes.byref(blocks[i]), ctypes.byref(L.params), StepParams.idx.offset)
            lib.dra_dqn_learner_actor_ring_push(L.h, blocks, n, L._sp(L.actor_stream))
            self.pushed += n
            return
        if getattr(self, "_blk", None) is None or len(self._blk) != n:
            self._blk = np.zeros(n, dtype=_STEP_PARAMS_DTYPE)
            self._blk["store_action"][:, :ne] = 1
            self._blk["n_env"] = ne
        b = self._blk
        k = n * ne
        tr, eps = [], []
        transition, epsilon_fn = self.stream.transition, self.epsilon_fn
        for _ in range(k):
            tr.append(transition())
            eps.append(epsilon_fn())                                 # DQN_agent.py:34-39, once per transition
        b["slot"][:, :ne] = ((self.slot + np.arange(k, dtype=np.int64)) % self.capacity).reshape(n, ne)
        b["counter"][:, :ne] = np.fromiter((t[0] for t in tr), dtype=np.int64, count=k).reshape(n, ne)
        b["rcounter"][:, :ne] = np.fromiter((t[1] for t in tr), dtype=np.int64, count=k).reshape(n, ne)
        b["stack_age"][:, :ne] = np.fromiter((t[2] for t in tr), dtype=np.int32, count=k).reshape(n, ne)
        b["random_action"][:, :ne] = rnd[0].reshape(n, ne)
        b["dice"][:, :ne] = rnd[1].reshape(n, ne)                    # (float64 -> float32 as the ctypes field assignment rounds)
        b["epsilon"][:, :ne] = np.asarray(eps, dtype=np.float64).reshape(n, ne)
        self.slot = (self.slot + k) % self.capacity
        for i in range(n):
            self.pending.append([t[3:] for t in tr[i * ne:(i + 1) * ne]])
        ctypes.memmove(ctypes.byref(L.params), b[n - 1:].ctypes.data, StepParams.idx.offset)   # (what the per-field path leaves there)
        lib.dra_dqn_learner_actor_ring_push(L.h, ctypes.cast(b.ctypes.data, ctypes.POINTER(StepParams)), n, L._sp(L.actor_stream))
        self.pushed += n

    def step(self, account):
        """One agent step.  account(infos) is called with the (reward, done, info) of the transitions this call reports
        (async mode: the ones the actor produced one call earlier) and returns whether this step updates
        (DQN_agent.py:114: total_steps > exploration_steps)."""
        L, rp = self.L, self.rp
        if not self.async_actor:
            infos = self._block()
            if self.per:
                rp.advance(self.n_env, stream=self.tree_stream)
            else:
                rp.advance(self.n_env)
            do_update = bool(account(infos))
            if self.per and do_update:
                # DQN_agent.py:114-127 with PrioritizedReplay: the tree descent (host-drawn uniforms) is enqueued BEFORE
                # the actor's transitions and its leaves land in pinned memory, so the one host round trip of the draw
                # (validity / padding stay on the host, draw for draw) hides under the actor's forward passes; importance
                # weights are applied inside the update (captured graph, exponent from device memory) and the new priorities
                # go back to the tree without leaving the device
                pending_draw = rp.draw_begin(stream=self.tree_stream)
                L.set_per(False, 0.0)
                L.step(None, False, False)            # actor transitions only (in order, on the update stream)
                tree_idx, prob, data_idx = rp.draw_end(pending_draw)
                L.update(data_idx, use_graph=True, sampling_prob=prob, beta=self.beta_fn())
                self.tree_stream.wait_stream(L.stream)                # the write-back reads this update's priorities
                rp.commit_device(tree_idx, L.prio, stream=self.tree_stream)
                return infos
            idx = rp.draw_indices() if do_update else None
            if self.per:
                L.set_per(False, 0.0)
            L.step(idx, do_update, False)
            return infos
        if not self.primed:
            self._push()
            L.params.n_env = self.n_env
            L.act(use_graph=False, stream=L.actor_stream)          # transitions of agent step 0
            self.issued += 1
            L.actor_stream.synchronize()
            self.primed = True
        infos = self.pending.pop(0)                                  # produced by the actor launch issued last call
        if self.per:
            # (chain mode, once primed: the tree side of these adds ran inside the previous update's chain kernel)
            primed = self._dd is not None and self._dd.active
            rp.advance(self.n_env, stream=self.tree_stream, tree=not (self.chain and primed))
        else:
            rp.advance(self.n_env)
        do_update = bool(account(infos))
        if self.pushed - self.issued < 8:
            self._push()
        L.params.n_env = self.n_env
        if self.per and do_update and self.chain == 2:
            if self._dd is None:
                from .replay import DeviceDraw
                self._dd = DeviceDraw(rp, L)
            dd = self._dd
            if not dd.active:
                # the first prioritized update: a classic draw (tree stream); the tree then belongs to the update stream
                tree_idx, prob, _ = rp.draw_end(rp.draw_begin(stream=self.tree_stream))
                self.tree_stream.synchronize()
                dd.start(tree_idx, prob, 1.0, self.beta_fn())         # (sampling probabilities as they are: p / 1.0)
            dd.fill(L.next_slot(), self.n_env, self.beta_fn())        # (the exponent of the update AFTER this one)
            L.set_per(True, -1.0)
            L.step_update()                                          # [fwd + loss][commit, adds, next draw][bwd + optimizer]
            L.step_actor(dd.issued_idx())                            # actor(t+1); hazard check on the minibatch just issued
            self.issued += 1
            if self.pushed - self.issued < 16:
                self._push(1)
            return infos
        if self.per and do_update:
            # PrioritizedReplay inside the two-stream pipeline: the draw of step t needs the priorities update t-1 wrote
            # back, so the host does wait once per step (tree stream: write-back t-1, adds t, descent t -> pinned memory);
            # the actor transitions of step t+1 still run underneath update t on their own stream and CU partition
            # (every tree-stream call takes the stream explicitly: torch's stream / device context managers and per-call Event
            # objects were ~100 us of host time per step, and the host IS on this pipeline's critical path)
            pending_draw = rp.draw_begin(stream=self.tree_stream)
            tree_idx, prob, data_idx = rp.draw_end(pending_draw)
            L.upload_sampling_prob(prob, self.beta_fn())
            L.set_per(True, -1.0)
            L.step(data_idx, True, True)                             # update(t) with importance weights, actor(t+1)
            L.wait_loss(self.tree_stream)                            # the write-back starts under the backward pass
            rp.commit_device(tree_idx, L.prio, stream=self.tree_stream)
            self.issued += 1
            return infos
        if self.per:
            L.set_per(False, 0.0)
        idx = rp.draw_indices() if do_update else None
        L.step(idx, do_update, True)                                 # gather(t), actor(t+1), update(t)
        self.issued += 1
        return infos


class DQNLearnerBench:
    """BASELINE configs[1] on synthetic data.  Per step: 4 env transitions (device frame source +
    device actor, epsilon-greedy with host-drawn randomness), one reference-exact uniform minibatch
    draw, one fused update; target sync every 10 000 updates (examples.py:90).

    async_actor=True is the reference's dqn_pixel setting (examples.py:96): the actor works one
    agent step ahead of the learner on its own stream; async_actor=False is the in-order mode the
    parity tests use."""

    def __init__(self, ring_capacity=1_000_000, batch=32, seed=0, actor=True, async_actor=True, n_actions=4,
                 prefill=None, variant=-1, head="vanilla"):
        """head: "vanilla" (BASELINE configs[1]: VanillaNet, centered RMSprop, clip 5), "c51" (CategoricalNet 51 atoms on
        [-10, 10], Adam lr 2.5e-4 eps 0.01/32, clip 0.5: examples.py:127-158) or "qr" (QuantileNet 200 quantiles, Adam lr 5e-5,
        clip 5: examples.py:192-222) -- the same pipeline with config 4's heads, for the schedule oracle."""
        from .nets import CategoricalNet, NatureConvBody, QuantileNet, VanillaNet
        dev = Config.DEVICE
        if dev.type != "cuda":
            raise DraError("DQNLearnerBench needs select_device(gpu_id >= 0)")
        self.batch, self.capacity, self.seed, self.actor, self.async_actor = batch, ring_capacity, seed, actor, async_actor
        self.history, self.n_step, self.n_actions = 4, 1, n_actions
        self.ring = ops.Ring(ring_capacity, 7056, 8, self.history, self.n_step, 0.99)
        self.head = head
        if head == "vanilla":
            make, extra = (lambda: VanillaNet(n_actions, NatureConvBody())), dict(gradient_clip=5.0, lr=0.00025, alpha=0.95, eps=0.01)
        elif head == "c51":
            make = lambda: CategoricalNet(n_actions, 51, NatureConvBody())
            extra = dict(gradient_clip=0.5, lr=0.00025, alpha=0.0, eps=0.01 / 32, head_kind=HEAD_CATEGORICAL, n_atoms=51,
                         v_min=-10.0, v_max=10.0, optimizer=OPT_ADAM)
        elif head == "qr":
            make = lambda: QuantileNet(n_actions, 200, NatureConvBody())
            extra = dict(gradient_clip=5.0, lr=0.00005, alpha=0.0, eps=0.01 / 32, head_kind=HEAD_QUANTILE, n_atoms=200,
                         optimizer=OPT_ADAM)
        else:
            raise DraError("DQNLearnerBench: head must be vanilla / c51 / qr")
        self.network, self.target_network = make(), make()
        self.target_network.load_state_dict(self.network.state_dict())
        clip, lr, alpha, eps = extra.pop("gradient_clip"), extra.pop("lr"), extra.pop("alpha"), extra.pop("eps")
        self.learner = DQNLearner(self.network, self.target_network, self.ring, batch, n_actions, 0.99, clip, lr, alpha,
                                  eps, centered=(head == "vanilla"), env_seed=seed, env_done_period=800, variant=variant,
                                  cu_partition=bool(actor and async_actor), **extra)
        # resident replay before the timed region: fill the whole ring (exploration phase done)
        prefill = ring_capacity if prefill is None else prefill
        with torch.cuda.stream(self.learner.stream):
            self.ring.fill_synthetic(0, prefill, 0, seed, n_actions=n_actions, done_period=800)
        self.counter = prefill        # next synthetic frame
        self.size = prefill
        self.pos = prefill % ring_capacity
        self.updates = 0
        self.epsilon = 0.01
        self.learner.synchronize()
        self._primed = False
        v = self.learner.variant
        need = ops.VAR_GATHER_IN_GRAPH | ops.VAR_PIPE_GATHER | ops.VAR_ACTOR_PARAMS
        self._gather_in_graph = async_actor and (v & need) == need and not (v & ops.VAR_ACTOR_V3)
        need = ops.VAR_ACTOR_RING | ops.VAR_PIPE_GATHER | ops.VAR_ACTOR_PARAMS
        self._actor_ring = (async_actor and (v & need) == need and not self._gather_in_graph and not (v & ops.VAR_ACTOR_V3))
        # async_actor=True is a separate PROCESS in the reference (BaseAgent.py:108-182) with its own np.random
        # state: the actor's epsilon-greedy randomness comes from its own stream here too (the in-order mode keeps
        # the single global stream, draw for draw)
        self.actor_rs = np.random.RandomState(seed + 977) if async_actor else None
        self._ring_pushed = self._ring_issued = 0
        self._fed_steps = 0
        self._idx_next = None
        self._pos0, self._size0 = self.pos, self.size

    def _queue_env_steps(self, n=4):
        """Host side of n env transitions: slots / frame counters and the epsilon-greedy randomness in
        the reference's draw order (torch_utils.py:51-58).  Returns (pos, size) after feeding them."""
        slots, counters, ras, dices = [], [], [], []
        pos, size = self.pos, self.size
        for _ in range(n):
            slots.append(pos)
            counters.append(self.counter)
            rs = self.actor_rs if self.actor_rs is not None else np.random
            ras.append(int(rs.randint(self.n_actions, size=1)[0]))
            dices.append(float(rs.rand(1)[0]))
            self.counter += 1
            size = min(size + 1, self.capacity)
            pos = (pos + 1) % self.capacity
        self.learner.set_env_steps(slots, counters, ras, dices, [self.epsilon] * n)
        return pos, size

    def step(self):
        L = self.learner
        if not self.actor:
            L.params.n_env = 0
            L.step(draw_uniform_indices(self.size, self.pos, self.batch, self.history, self.n_step), True, False)
        elif not self.async_actor:
            self.pos, self.size = self._queue_env_steps(4)
            L.step(draw_uniform_indices(self.size, self.pos, self.batch, self.history, self.n_step), True, False)
        elif self._actor_ring:
            # parameter blocks are generated and uploaded ahead of time (16 agent steps per upload); a call carries
            # only the minibatch indices
            if not self._primed:
                self._push_blocks()
                L.params.n_env = 4
                L.act(use_graph=False, stream=L.actor_stream)      # transitions of step 0
                self._ring_issued += 1
                L.actor_stream.synchronize()
                self._primed = True
            self._fed_steps += 1                                   # transitions of this step are in the ring
            if L.ahead_stream is not None:
                # DRA_VAR_TARGET_AHEAD: this step's minibatch was drawn one call ago (the same draws in the same order: nothing
                # else consumes np.random here -- the async actor has its own RandomState), the next one is drawn now and handed
                # over with this call, which issues its target(next_states) under this step's update
                idx = self._idx_next if self._idx_next is not None else self._draw_at(self._fed_steps)
                self._idx_next = self._draw_at(self._fed_steps + 1)
                L.stage_next_indices(self._idx_next)
            else:
                idx = self._draw_at(self._fed_steps)
            if self._ring_pushed - self._ring_issued < 8:
                self._push_blocks()
            L.params.n_env = 4
            L.step(idx, True, True)                                # gather(t), actor(t+1) from the ring, update(t)
            self._ring_issued += 1
        elif self._gather_in_graph:
            # one call = transitions of a step + the minibatch sampled after them (reference draw order: actor
            # randomness, then the sample); the C side issues the update of the PREVIOUS call's minibatch
            self.pos, self.size = self._queue_env_steps(4)
            L.step(draw_uniform_indices(self.size, self.pos, self.batch, self.history, self.n_step), True, True)
        else:
            if not self._primed:  # the actor runs one agent step ahead
                self._next = self._queue_env_steps(4)
                L.act(use_graph=True, stream=L.actor_stream)
                L.actor_stream.synchronize()
                self._primed = True
            self.pos, self.size = self._next                      # transitions of this step are in the ring
            idx = draw_uniform_indices(self.size, self.pos, self.batch, self.history, self.n_step)
            self._next = self._queue_env_steps(4)                 # next step's transitions, overlapped with the update
            L.step(idx, True, True)
        self.updates += 1
        if self.updates % 10000 == 0:
            L.sync_target()

    def _draw_at(self, fed_steps):
        """The uniform minibatch of the agent step after `fed_steps` x 4 transitions (replay.py:92-110 on the ring's cursor then)."""
        n = 4 * fed_steps
        pos, size = (self._pos0 + n) % self.capacity, min(self._size0 + n, self.capacity)
        return draw_uniform_indices(size, pos, self.batch, self.history, self.n_step)

    def _push_blocks(self, n=16):
        """Generates the parameter blocks of the next n agent steps (slots / counters / actor randomness) and
        uploads them into the learner's device ring on the actor stream.  The blocks of one upload are filled as arrays
        (the actor's own RandomState stream word for word: actor_randomness_block); a per-field python loop over 16 blocks
        cost 270 us of host time per upload -- more than the three steps the host runs ahead of the GPU."""
        L = self.learner
        rnd = actor_randomness_block(self.actor_rs, self.n_actions, 4 * n) if self.actor_rs is not None else None
        if rnd is None:                                            # (no vectorised form of this stream: the scalar draws)
            blocks = (StepParams * n)()
            for i in range(n):
                self.pos, self.size = self._queue_env_steps(4)
                ctypes.memmove(ctypes.byref(blocks[i]), ctypes.byref(L.params), StepParams.idx.offset)
            lib.dra_dqn_learner_actor_ring_push(L.h, blocks, n, L._sp(L.actor_stream))
            self._ring_pushed += n
            return
        if getattr(self, "_blk", None) is None or len(self._blk) != n:
            self._blk = np.zeros(n, dtype=_STEP_PARAMS_DTYPE)
            self._blk["store_action"][:, :4] = 1
            self._blk["stack_age"][:, :4] = 3
            self._blk["n_env"] = 4
        b = self._blk
        k = np.arange(4 * n, dtype=np.int64).reshape(n, 4)
        b["slot"][:, :4] = (self.pos + k) % self.capacity
        b["counter"][:, :4] = b["rcounter"][:, :4] = self.counter + k
        b["random_action"][:, :4] = rnd[0].reshape(n, 4)
        b["dice"][:, :4] = rnd[1].reshape(n, 4)                   # (float64 -> float32 as the ctypes field assignment rounds)
        b["epsilon"][:, :4] = self.epsilon
        self.counter += 4 * n
        self.pos = (self.pos + 4 * n) % self.capacity
        self.size = min(self.size + 4 * n, self.capacity)
        ctypes.memmove(ctypes.byref(L.params), b[n - 1:].ctypes.data, StepParams.idx.offset)   # (what the scalar path leaves there)
        lib.dra_dqn_learner_actor_ring_push(L.h, ctypes.cast(b.ctypes.data, ctypes.POINTER(StepParams)), n, L._sp(L.actor_stream))
        self._ring_pushed += n

    def host_profile(self, n=200):
        """Host-side cost of one agent step with the GPU idle (synchronise before every call): python
        bookkeeping + RNG vs the C call that enqueues the step.  Microseconds."""
        import time
        L = self.learner
        py = call = 0.0
        for _ in range(n):
            L.synchronize()
            t0 = time.perf_counter()
            if self._actor_ring:
                t0 = time.perf_counter()
                self.step()
                t2 = time.perf_counter()
                call += t2 - t0
                continue
            if self._gather_in_graph:
                self.pos, self.size = self._queue_env_steps(4)
                idx = draw_uniform_indices(self.size, self.pos, self.batch, self.history, self.n_step)
                t1 = time.perf_counter()
                L.step(idx, True, True)
                t2 = time.perf_counter()
                py += t1 - t0
                call += t2 - t1
                continue
            self.pos, self.size = self._next if self.async_actor and self._primed else (self.pos, self.size)
            idx = draw_uniform_indices(self.size, self.pos, self.batch, self.history, self.n_step)
            nxt = self._queue_env_steps(4)
            t1 = time.perf_counter()
            if self.async_actor:
                self._next = nxt
                L.step(idx, True, True)
            else:
                self.pos, self.size = nxt
                L.step(idx, True, False)
            t2 = time.perf_counter()
            py += t1 - t0
            call += t2 - t1
        L.synchronize()
        return {"python_us": 1e6 * py / n, "enqueue_call_us": 1e6 * call / n}

    def roofline(self, n=200):
        """Per-kernel-group times of the update with HIP events on the learner's stream, and the
        roofline position of the dominant one."""
        L = self.learner
        L.synchronize()
        acc = {}
        for _ in range(n):
            L.upload_indices(draw_uniform_indices(self.size, self.pos, self.batch, self.history, self.n_step))
            for k, v in L.profile().items():
                acc.setdefault(k, []).append(v)
        # mean over the launches after dropping the 5 % slowest and fastest of each group: ONE multi-millisecond host / clock
        # hiccup inside an event pair otherwise moves a 13 us average to 36 us (seen once in 30 runs, profiles/r02zg_*)
        cut = n // 20
        ms = {k: float(np.mean(sorted(v)[cut:n - cut])) for k, v in acc.items()}
        # an event pair around a kernel reads (kernel duration) + (dependent-launch boundary + the record itself: ~2.8 us
        # against rocprofv3's per-kernel durations).  The same pair with NOTHING in between is reported next to it but NOT
        # subtracted: two back-to-back records cost more (4.6-5.2 us) than the pair adds around a kernel, the difference
        # would under-state the kernel (measured: 11.1 us vs 13.1 us by rocprofv3, profiles/r02zzz_*)
        self.event_bracket_ms = ms.pop("_event_bracket", 0.0)
        self.kernel_ms = ms
        b = self.batch
        flops = {"conv1_fwd": 2 * 2 * b * 400 * 32 * 256, "conv2_fwd": 2 * 2 * b * 81 * 64 * 512,
                 "conv3_fwd": 2 * 2 * b * 49 * 64 * 576, "fc4_fwd": 2 * 2 * b * 512 * 3136,
                 "conv3_bwd_w": 2 * b * 49 * 64 * 576, "conv3_bwd_x": 2 * b * 49 * 64 * 576,
                 "conv2_bwd_w": 2 * b * 81 * 64 * 512, "conv2_bwd_x": 2 * b * 81 * 64 * 512,
                 "conv1_bwd_w": 2 * b * 400 * 32 * 256, "fc4_bwd_w": 2 * b * 512 * 3136, "fc4_bwd_x": 2 * b * 512 * 3136}
        variant = L.cfg.variant if L.cfg.variant >= 0 else ops.get_tuning()
        if variant & (ops.VAR_FUSED_BWD | ops.VAR_ONESHOT_WGRAD):
            # a layer's weight- and input-gradient kernels share one launch, charged to the *_bwd_x group
            for lay in ("fc4", "conv3", "conv2"):
                flops[lay + "_bwd_x"] += flops.pop(lay + "_bwd_w")
        # optimizer launch: p, g, two state buffers read, p, the two state buffers and the actor's parameter copy written
        # (32 B / parameter); with DRA_VAR_LATE_FOLD the same launch also folds conv1's weight-gradient slabs (read once)
        step_bytes = 32 * L.flat.numel
        if variant & ops.VAR_LATE_FOLD:
            n1 = ops.conv_wgrad_slabs(1, b, 16, variant)
            step_bytes += 4 * n1 * (32 * 4 * 8 * 8 + 32)
        bytes_ = {"gather": b * (5 * 7056) + 2 * b * 4 * 7056, "rmsprop_step": step_bytes}

        # algorithmic HBM bytes of the MFMA launches (every distinct operand read once, every result written once, fp32):
        # what the PMC traffic of the same launch is compared with (`traffic_ratio`)
        w1, w2, w3 = 32 * 4 * 64 + 32, 64 * 32 * 16 + 64, 64 * 64 * 9 + 64
        y1, y2, y3 = b * 32 * 400, b * 64 * 81, b * 64 * 49
        alg_hbm = {"conv1_fwd": 2 * b * 4 * 7056 + 4 * (2 * w1 + 2 * y1), "conv2_fwd": 4 * (2 * y1 + 2 * w2 + 2 * y2),
                   "conv3_fwd": 4 * (2 * y2 + 2 * w3 + 2 * y3), "conv3_bwd_x": 4 * (y3 + y2 + w3 + y2 + w3),
                   "conv2_bwd_x": 4 * (y2 + y1 + w2 + y1 + w2), "conv1_bwd_w": b * 4 * 7056 + 4 * (y1 + w1)}

        def entry(k):
            if k in flops:
                ach = flops[k] / (ms[k] * 1e-3) / 1e12
                return {"kernel": k, "bound": "mfma", "achieved": ach, "peak": 157.3, "unit": "TFLOP/s",
                        "frac": ach / 157.3, "traffic": None, "avg_ms": ms[k], "algorithmic_flops": flops[k],
                        "algorithmic_bytes_hbm": alg_hbm.get(k), "event_pair_empty_ms": self.event_bracket_ms}
            byt = bytes_.get(k, 0)
            ach = byt / (ms[k] * 1e-3) / 1e9
            return {"kernel": k, "bound": "hbm", "achieved": ach, "peak": 8000.0, "unit": "GB/s", "frac": ach / 8000.0,
                    "traffic": None, "avg_ms": ms[k], "algorithmic_bytes": byt, "event_pair_empty_ms": self.event_bracket_ms}

        dom = max(ms, key=ms.get)
        out = entry(dom)
        # The MFMA-bound kernel reported next to it is conv2's backward launch (input + weight gradient: the largest MFMA
        # launch of the backward pass, the one VERDICT r2 / r3 price the path by) -- by name, not "whichever MFMA kernel read
        # longest in this run": the four convolution launches are within a microsecond of each other and the pick flipped
        # between runs.  Every MFMA kernel's live reading is in `mfma_kernels`, longest first.
        mfma = "conv2_bwd_x" if "conv2_bwd_x" in ms and "conv2_bwd_x" in flops else max((k for k in ms if k in flops), key=ms.get, default=None)
        self.roofline_mfma = entry(mfma) if mfma is not None and mfma != dom else None
        if self.roofline_mfma is not None:
            # the same kernel replayed ALONE, 64 dependent launches in one captured graph between two events (no event pair per
            # launch): per-launch period, the period of an empty kernel in the same form (the in-graph launch boundary), and
            # their difference = the kernel's own duration, live in this run
            try:
                per_us, empty_us = L.kernel_replay(mfma, 64)
                own_us = max(per_us - empty_us, 1e-3)
                self.roofline_mfma["graph_replay"] = {
                    "launches": 64, "us_per_launch": per_us, "empty_kernel_us_per_launch": empty_us, "kernel_us": own_us,
                    "achieved": flops[mfma] / (own_us * 1e-6) / 1e12, "frac": flops[mfma] / (own_us * 1e-6) / 1e12 / 157.3,
                    "frac_with_boundary": flops[mfma] / (per_us * 1e-6) / 1e12 / 157.3}
            except DraError as e:
                self.roofline_mfma["graph_replay"] = {"error": str(e)}
            # DRA_VAR_FWD_CHAIN / DRA_VAR_BWD_CHAIN: the timed pipeline runs conv1 + conv2 + conv3 forward (both nets) and the three
            # conv backward layers as ONE launch each; the per-layer groups above are what the eager profile launches, not what is
            # timed.  The headline MFMA kernel is then the chained forward launch (the longest kernel of the update stream),
            # replayed alone the same way; the chained backward beside it.
            chains = {}
            if (variant & ops.VAR_FWD_CHAIN) and (variant & ops.VAR_BWD_CHAIN):
                spec = {"fwd": ("conv_fwd_chain", ("conv1_fwd", "conv2_fwd", "conv3_fwd"),
                                alg_hbm["conv1_fwd"] + 4 * (2 * w2 + 2 * y2) + 4 * (2 * w3 + 2 * y3)),
                        "bwd": ("conv_bwd_chain", ("conv3_bwd_x", "conv2_bwd_x", "conv1_bwd_w"),
                                4 * (y3 + y2 + 2 * w3) + 4 * (y1 + 2 * w2) + b * 4 * 7056 + 4 * w1)}
                if variant & ops.VAR_BWD_CHAIN_FC:      # fc4's + the head's backward lead the chained backward launch
                    w4 = 512 * 3136
                    spec["bwd"] = ("conv_bwd_chain", ("fc4_bwd_x",) + spec["bwd"][1], spec["bwd"][2] + 4 * (2 * w4 + b * 512 + 2 * y3))
                for which, (name, parts, alg) in spec.items():
                    try:
                        per_us, empty_us = L.chain_replay(which, 64)
                    except DraError as e:
                        chains[name] = {"error": str(e)}
                        continue
                    fl = sum(flops[k] for k in parts)
                    own_us = max(per_us - empty_us, 1e-3)
                    with_boundary_us = own_us + 0.5 * empty_us      # (the empty pass is two launches per repetition)
                    chains[name] = {"kernel": name, "bound": "mfma", "peak": 157.3, "unit": "TFLOP/s", "layers": list(parts),
                                    "algorithmic_flops": fl, "algorithmic_bytes_hbm": alg, "traffic": None,
                                    "avg_ms": with_boundary_us * 1e-3, "achieved": fl / (with_boundary_us * 1e-6) / 1e12,
                                    "frac": fl / (with_boundary_us * 1e-6) / 1e12 / 157.3,
                                    "event_pair_empty_ms": self.event_bracket_ms,
                                    "graph_replay": {"launches": 64, "us_per_launch": with_boundary_us,
                                                     "us_per_repetition_with_epoch_launch": per_us,
                                                     "empty_kernel_us_per_repetition": empty_us, "kernel_us": own_us,
                                                     "achieved": fl / (own_us * 1e-6) / 1e12,
                                                     "frac": fl / (own_us * 1e-6) / 1e12 / 157.3,
                                                     "frac_with_boundary": fl / (with_boundary_us * 1e-6) / 1e12 / 157.3}}
            self.roofline_chains = chains
            self.roofline_mfma["mfma_kernels"] = [
                {"kernel": k, "avg_ms": ms[k], "algorithmic_flops": flops[k], "frac": flops[k] / (ms[k] * 1e-3) / 1e12 / 157.3}
                for k in sorted((k for k in ms if k in flops), key=ms.get, reverse=True)]
        return out

    def report(self):
        ms = getattr(self, "kernel_ms", {})
        # an EAGER update with an event pair around every kernel group (dra_dqn_learner_profile): each entry includes the
        # pair's own launch boundary, and the eager form gathers its minibatch (the timed ring-direct graphs do not launch
        # `gather`); groups the learner's variant does not launch at all (a bare event pair) are dropped.  Not a
        # decomposition of ms_per_step.
        floor = 1.05 * getattr(self, "event_bracket_ms", 0.0)
        shown = {k: round(v, 5) for k, v in ms.items() if v > floor}
        return {"eager_profile_ms": shown, "eager_profile_note": "event-pair readings of ONE eager update, launch boundaries "
                "included; `gather` runs only in this eager form (the timed graphs read the ring directly)"}
