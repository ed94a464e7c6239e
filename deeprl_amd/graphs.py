"""Everything about capturing device work as a hipGraph: the capture protocol, once (Region), and the wrappers that put the
agents' regions on it ("The capture protocol").  What is specific to a site -- what it stages, what it keeps eager,
which counter it restores -- stays with the site; the order of the steps around a capture, and what a failed one leaves behind, do
not."""
import contextlib
import gc
import warnings

import numpy as np
import torch

from . import ops
from .envs import LazyFrames
from .support import Config, StagedUpload, random_sample, tensor, to_np


@contextlib.contextmanager
def _capture(graph):
    """torch.cuda.graph(graph) with the cyclic garbage collector held off for the duration of the capture.  A collection that
    runs INSIDE a capture may finalise objects of an earlier agent that own HIP resources (pinned host tensors, the fused
    learner's library handle): their frees / device synchronisation are illegal while a stream captures and end the process
    (std::terminate out of a deleter) -- seen as a sporadic abort of the test suite at the first captured update that followed a
    closed device-pipeline agent.  Collect first, then capture without the collector."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was:
            gc.enable()


def _capture_failed(config, what, error):
    """A hipGraph capture failed.  Falling back to the eager kernels silently would turn a broken capture into nothing but a
    slower number, so it is an error unless the configuration opts into the fallback (config.allow_eager_fallback = True:
    e.g. a user network with host-side control flow)."""
    if not getattr(config, 'allow_eager_fallback', False):
        raise RuntimeError("%s could not be captured as a hipGraph (%r); set config.allow_eager_fallback = True to run it "
                           "eagerly, or config.graph_update = False to skip capturing" % (what, error)) from error
    warnings.warn("%s could not be captured as a graph (%r); using the eager path" % (what, error))


def _fused_noisy(config, net):
    """Noisy layers on csrc/noisy.hip: config.fused_noisy (default on) over a network that stages its noise in one block
    (nets.RainbowNet), on the device.  Only then may the actor forward / the update of a noisy agent be captured."""
    return (getattr(config, 'fused_noisy', True) is not False and Config.DEVICE.type == 'cuda' and net is not None
            and hasattr(net, 'noise_block') and getattr(net, 'fused_noisy', False))


class Region:
    """One region of device work that runs eagerly for `warmup` calls and is replayed from a captured hipGraph afterwards.
    `what` names it in _capture_failed's message; `opts` are the FusedOptimizers that step INSIDE the graph (capture() may name
    them instead, where that is decided per capture); `validate_off`: torch.distributions' argument validation is off while
    capturing -- its checks synchronise with the host.  A call goes
        if region.due(key):                        # counts the call; a key other than the captured one drops the graph
            if region.graph is not None or region.capture(body, key):
                return region.replay()             # the capturing call replays too: the capture pass only records
        ... the eager path ...
    `graph` / `out` are one CUDAGraph and what its body returned or, for a dict of bodies, dicts of them under the same names."""

    def __init__(self, what, config, warmup, opts=(), validate_off=False):
        self.what, self.config, self.warmup, self.opts, self.validate_off = what, config, warmup, opts, validate_off
        self.calls = 0
        self.graph = None
        self.out = None
        self.key = None
        self.failed = False     # sticky: a capture failed and config.allow_eager_fallback let the run go on eagerly

    def on(self):
        return not self.failed and getattr(self.config, 'graph_update', True) is not False

    def due(self, key=None):
        self.calls += 1
        if self.calls <= self.warmup or not self.on():
            return False
        if self.graph is not None and key != self.key:
            self.graph = None
        return True

    def capture(self, body, key=None, opts=None):
        """Records body() -- or every body of a dict, in order -- and keeps graph, out and key -> whether a graph now exists.  The
        optimizers go into graph mode BEFORE the capture begins (their device scalars must not come from the graph's pool).  A
        failure raises out of _capture_failed, or else leaves failed set, no graph, and the optimizers back in eager mode."""
        if opts is not None:
            self.opts = opts
        named = isinstance(body, dict)
        bodies = body if named else {None: body}
        validate = torch.distributions.Distribution._validate_args
        try:
            if self.validate_off:
                torch.distributions.Distribution.set_default_validate_args(False)
            for o in self.opts:
                o.enable_graph_mode()
            graphs = {name: torch.cuda.CUDAGraph() for name in bodies}
            outs = {}
            torch.cuda.synchronize()
            for name, fn in bodies.items():
                with _capture(graphs[name]):
                    outs[name] = fn()
            self.graph, self.out = (graphs, outs) if named else (graphs[None], outs[None])
            self.key = key
        except Exception as e:      # e.g. a network with host-side control flow
            _capture_failed(self.config, self.what, e)
            self.failed = True
            self.graph = None
            for o in self.opts:
                o.graph_mode = False
        finally:
            if self.validate_off:
                torch.distributions.Distribution.set_default_validate_args(validate)
        return self.graph is not None

    def replay(self):
        for o in self.opts:
            o.prepare_step()
        self.graph.replay()
        return self.out


class _GraphedQ(Region):
    """DQNActor's forward (DQN_agent.py:29-33) as ONE hipGraph replay for image observations: the uint8
    [1,C,H,W] observation goes through pinned staging into a static device buffer; normaliser table kernel,
    network forward and the action-value reduction replay from a graph captured (torch.cuda.graphs) after four
    eager calls (one agent step: by then a DQNAgent that qualifies for the fused learner has switched to it).
    Same kernels, same arguments as the eager path -> bit-identical action values."""
    WARMUP = 4

    def __init__(self, actor):
        Region.__init__(self, "the actor forward", actor.config, self.WARMUP)
        self.actor = actor
        self.upload = None

    def usable(self, state):
        from .normalizers import RescaleNormalizer
        cfg = self.config
        if not self.on():
            return False
        if cfg.noisy_linear and not _fused_noisy(cfg, self.actor._network):
            return False        # the module path materialises the mixed weights with ATen kernels: eager
        if not isinstance(cfg.state_normalizer, RescaleNormalizer):
            return False
        first = state[0] if isinstance(state, (list, tuple)) else state
        return isinstance(first, LazyFrames) or (isinstance(first, np.ndarray) and first.dtype == np.uint8)

    def __call__(self, state):
        """The action values of `state` on the host, or None (warming up, or the capture failed: the caller's eager forward)."""
        if not self.due():
            return None
        a, cfg = self.actor, self.config
        x = np.ascontiguousarray(np.asarray(state, dtype=np.uint8))
        if self.graph is None:
            self.upload = StagedUpload(x.shape, torch.uint8, next(a._network.parameters()).device)

            def forward():
                with torch.no_grad():
                    return a.q_device(a._network(cfg.state_normalizer(self.upload.dev)))
            forward()       # eager dry run of exactly what is captured: creates every lazily built object (normaliser table, ...)
            if not self.capture(forward):
                return None
        self.upload.put(x)
        return to_np(self.replay())


class _GraphedUpdate(Region):
    """One DQN-family update (DQN_agent.py:114-134: normalise, target / online forwards, fused loss kernel,
    backward, clip, optimizer) as ONE hipGraph replay over static minibatch buffers that the ring gather refills
    in place.  Captured with torch.cuda.graphs after two eager updates (which also run every lazy one-time
    initialisation); same kernels and arguments as the eager path -> bit-identical parameters.  Re-captured when a
    hyper-parameter baked into the graph changes (an lr schedule: FusedOptimizer.hyper_signature).

    Agents without noisy layers: uniform replay only.  Noisy layers on csrc/noisy.hip (_fused_noisy): uniform replay and the
    PER form -- rp.draw() -> gather into the static buffers -> sampling probabilities and the importance exponent in one
    small upload (the captured launches read beta from a device word) -> replay -> rp.commit_device(tree_idx, prio): the
    priorities never visit the host.  reset_noise() (target, then online: DQN_agent.py:116-118) runs outside the captured
    region; the graph reads the noise through static addresses."""
    WARMUP = 2

    def __init__(self, agent):
        Region.__init__(self, "the update", agent.config, self.WARMUP)
        self.agent = agent
        self.static = None
        self.per_words = None       # [batch sampling probabilities | beta] f32, device
        self._per_up = None

    def usable(self, rp):
        cfg = self.config
        if not self.on() or self.agent._fused is None:
            return False
        if cfg.noisy_linear:
            return _fused_noisy(cfg, self.agent.network) and _fused_noisy(cfg, self.agent.target_network)
        return not hasattr(rp, 'draw')

    def _upload_per(self, prob, beta):
        from .replay import _PinnedUploader
        b = len(prob)
        if self.per_words is None:
            dev = next(self.agent.network.parameters()).device
            self.per_words = torch.zeros(b + 1, dtype=torch.float32, device=dev)
            self._per_up = _PinnedUploader(torch.float32, b + 1, dev)
        words = np.empty(b + 1, dtype=np.float32)
        words[:b] = prob            # (f64 -> f32: the rounding the eager path's .float() applies)
        words[b] = beta
        self._per_up.upload_into(self.per_words, words)

    def run(self, rp):
        """Returns the loss-kernel outputs of the update it performed, or None (caller runs the eager update)."""
        agent, cfg = self.agent, self.config
        opt = agent._fused
        key = opt.hyper_signature()
        if not self.due(key):
            return None
        per = hasattr(rp, 'draw')
        tree_idx = None
        if per:
            tree_idx, prob, idx = rp.draw()
            self._upload_per(prob, cfg.replay_beta())
        else:
            idx = rp.draw_indices()
        if cfg.noisy_linear:
            agent.target_network.reset_noise()
            agent.network.reset_noise()
        if self.graph is None:
            self.static = rp.gather(idx)
            fields = dict(state=self.static['state'], action=self.static['action'], reward=self.static['reward'],
                          next_state=self.static['next_state'], mask=self.static['mask'])
            per_args = None
            if per:
                b = len(idx)
                fields.update(sampling_prob=self.per_words[:b], idx=None)
                # beta < 0: dra_td_loss reads the exponent behind the probabilities; beta_dev: dra_per_weights_dev
                per_args = dict(sampling_prob=self.per_words[:b], beta=-1.0, beta_dev=self.per_words[b:b + 1],
                                replay_eps=cfg.replay_eps, replay_alpha=cfg.replay_alpha)
            tr = rp.TransitionCLS(**fields)

            def update():
                out, (net_out, grad) = agent._loss_grad(tr, per_args)
                opt.zero_grad()
                agent._backward(net_out, grad)
                opt.step(cfg.gradient_clip)
                return out
            if not self.capture(update, key, (opt,)):
                g = rp.gather(idx)
                if per:
                    dev = g['state'].device
                    g.update(sampling_prob=torch.from_numpy(prob).to(dev), idx=torch.from_numpy(tree_idx).to(dev))
                    return agent._learn(rp.TransitionCLS(**{k: v for k, v in g.items() if k in rp.TransitionCLS._fields}),
                                        beta=float(self.per_words[-1].item()))
                return agent._learn(rp.TransitionCLS(**{k: v for k, v in g.items() if k in rp.TransitionCLS._fields}))
        else:
            rp.gather(idx, out=self.static)
        out = self.replay()
        if per:
            rp.commit_device(tree_idx, out['prio'])      # replay.py:193-196, the priorities stay on the device
        return out


class _OnPolicyGraph(Region):
    """Replays an on-policy agent's device-side work of one rollout (A2CAgent._rollout_compute: T forwards with action
    sampling, the return scan, loss, backward, clip, optimizer) from ONE captured hipGraph after two eager rollouts.  The
    rollout plan lives in persistent device buffers (DeviceAtariVec.plan), so every kernel argument is constant across
    rollouts; torch's graph-safe Philox bookkeeping continues the sampling generator exactly as the eager kernels would.
    Data parallel (dist.DataParallel): the captured region ends BEFORE the gradient exchange -- run(plan, compute, tail)
    replays [rollout + loss + backward] and then calls tail() eagerly (all-reduce of the flat gradient over RCCL / gloo,
    clip + optimizer step: three launches), so that ranks x environments-per-rank runs at the single-process graph speed.
    Not used with grad hooks or config.graph_update off.  Re-captured when the plan's counters move, the rollout length or a
    hyper-parameter baked into the graph changes, or a caller sets `.graph = None` (A2CAgent._step_device_rollout)."""
    WARMUP = 2

    def __init__(self, agent, optimizer_inside=True):
        Region.__init__(self, "the rollout", agent.config, self.WARMUP, validate_off=True)
        self.agent = agent
        self.optimizer_inside = optimizer_inside      # the captured region ends with agent._fused.step()

    def run(self, plan, compute, tail=None):
        """compute(plan): the capturable device work; tail(out) (optional): what must stay eager after it (the data-parallel
        exchange and the optimizer step behind it) -- called after the eager compute as well as after a replay."""
        a = self.agent
        opts = (a._fused,) if (self.optimizer_inside and tail is None) else ()
        key = (plan.counters.data_ptr(), plan.t_len, opts[0].hyper_signature() if opts else None)
        live = self.due(key) and a.grad_hook is None
        if live and self.graph is None:
            steps = a._rollout_step
            live = self.capture(lambda: compute(plan), key, opts)
            a._rollout_step = steps       # the capture pass only recorded the work -- or failed part-way through it
        if live:
            out = self.replay()
            a._rollout_step += plan.t_len + (1 if hasattr(a, '_act') else 0)
        else:
            out = compute(plan)
        return out if tail is None else tail(out)


class _GraphedAct(Region):
    """PPOAgent._act's no-grad forward (PPO_agent.py:35-36, incl. the action sample) over host observations, _GraphedQ's twin:
    the f32 observations go through pinned staging into a static input, and after two eager calls the forward is replayed from
    a captured hipGraph -- same kernels, same arguments, and torch's graph-safe Philox bookkeeping continues the generator's
    sequence exactly as the eager sampling kernels would.  Re-captured when the observations' shape changes.  Its switch is
    config.graph_rollout, which defaults to config.graph_update."""
    WARMUP = 2

    def __init__(self, agent):
        Region.__init__(self, "the rollout forward", agent.config, self.WARMUP, validate_off=True)
        self.agent = agent
        self.upload = None
        self.u = None       # a categorical net's uniforms: the static row the captured forward reads

    def on(self):
        cfg = self.config
        return not self.failed and bool(getattr(cfg, 'graph_rollout', getattr(cfg, 'graph_update', True)))

    def __call__(self, states):
        """(prediction dict, the f32 device copy of `states`), or None (not usable, warming up, or the capture failed)."""
        if Config.DEVICE.type != 'cuda' or isinstance(states, torch.Tensor) or not self.on():
            return None
        x = np.ascontiguousarray(np.asarray(states, dtype=np.float32))    # what tensor() uploads (torch_utils.py:23)
        if not self.due(x.shape):
            return None
        net = self.agent.network
        if self.graph is None:
            self.upload = StagedUpload(x.shape, torch.float32, Config.DEVICE)
            # (a categorical net reads its uniforms from the rollout's one draw: the captured forward reads a static row that
            # every replay fills from that draw first)
            slots = getattr(net, 'rollout_slots', None)
            self.u = None
            if slots is not None and getattr(net, 'sampler', None) is None:
                self.u = torch.zeros(x.shape[0], dtype=torch.float32, device=Config.DEVICE)
                slots.pin(self.u)

            def forward():
                with torch.no_grad():
                    return net(self.upload.dev)
            try:
                captured = self.capture(forward, x.shape)
            finally:
                if slots is not None:
                    slots.pin(None)
            if not captured:
                return None
        self.upload.put(x)
        if self.u is not None:
            u = net.rollout_slots.next_uniform()
            if u is not None and u.numel() == self.u.numel():
                self.u.copy_(u)
            else:
                self.u.uniform_()
        return {key: v.clone() for key, v in self.replay().items()}, self.upload.dev.clone()


class _GraphedPPO(Region):
    """PPO's optimisation phase (PPO_agent.py:71-99: epochs x minibatches, each a forward, the clip loss, a
    backward and one or two Adam steps -- 320 tiny updates per rollout at ppo_continuous's sizes) with every
    full-size minibatch replayed from captured hipGraphs: the rollout's rows live in static buffers, a static
    index tensor selects the minibatch inside the graph, Adam's step-dependent scalars (and a scheduled lr) reach
    the kernels through device memory (FusedOptimizer.prepare_step).  shared_repr: one graph (forward, loss,
    backward, clip, step).  Separate actor / critic optimisers: the KL gate of PPO_agent.py:88-93 needs the
    forward's result on the host first, so a forward+loss graph runs, the host decides, and one of two update
    graphs (actor+critic, critic only) -- each recomputing the same forward -- runs.  Same kernels and arguments
    as the eager path: bit-identical parameters.  First rollout and odd-sized remainder minibatches run eagerly.
    Re-captured, into new static buffers, when the rollout's shapes change."""
    WARMUP = 1

    def __init__(self, agent):
        Region.__init__(self, "the PPO minibatch update", agent.config, self.WARMUP, validate_off=True)
        self.agent = agent
        self.static = None
        self.idx = None
        self._up = None
        # the whole optimisation phase as one graph (_optimize_block): no warm-up of its own, re-captured when its length changes
        self.block = Region("the PPO optimisation phase", agent.config, 0, validate_off=True)
        self.block_idx = None
        self._block_up = None

    graphs = property(lambda self: self.graph)      # the minibatch graphs by name: 'all', or 'fwd' / 'both' / 'critic'

    def usable(self):
        a = self.agent
        cfg = self.config
        if not self.on() or self.block.failed or a.grad_hook is not None or a.dp.active:
            return False
        if Config.DEVICE.type != 'cuda':
            return False
        opts = [a._fused] if cfg.shared_repr else [a._fused_actor, a._fused_critic]
        return all(o.kind == 'adam' for o in opts)      # scheduled / stepped scalars travel through device memory

    def _forward_loss(self, e):
        cfg = self.config
        p = self.agent.network(e.state, e.action)
        out3, grads = ops.ppo_loss(p['log_pi_a'].detach(), p['entropy'].detach(), p['v'].detach(), e.log_pi_a, e.advantage, e.ret,
                                   cfg.ppo_ratio_clip, cfg.entropy_weight)
        return p, out3, grads

    def _step_split(self, p, grads, actor):
        """Separate optimisers, from one forward: the actor's step where the KL gate (PPO_agent.py:88) lets it, then the critic's --
        the arithmetic of PPOAgent._minibatch."""
        a = self.agent
        g_lp, g_ent, g_v = grads
        if actor:
            a._fused_actor.zero_grad()
            torch.autograd.backward([p['log_pi_a'], p['entropy']], [g_lp, g_ent])
            a._fused_actor.step(None)
        a._fused_critic.zero_grad()
        p['v'].backward(g_v)
        a._fused_critic.step(None)

    def _prepare_split(self, out3):
        """The KL gate on the host -> whether the actor steps too; prepare_step() on the optimisers that will step."""
        a = self.agent
        actor = out3[2].item() <= 1.5 * self.config.target_kl
        if actor:
            a._fused_actor.prepare_step()
        a._fused_critic.prepare_step()
        return actor

    def _bodies(self, entry_cls):
        """What the minibatch graphs record, by name."""
        a = self.agent
        rows = lambda: entry_cls(*ops.gather_rows(list(self.static), self.idx))     # all five fields, one launch
        if self.config.shared_repr:
            return dict(all=lambda: a._minibatch(rows(), prepared=True))

        def fwd():
            with torch.no_grad():
                return self._forward_loss(rows())[1]

        def update(actor):      # (each update graph recomputes the forward)
            p, _, grads = self._forward_loss(rows())
            self._step_split(p, grads, actor)
        return dict(fwd=fwd, both=lambda: update(True), critic=lambda: update(False))

    def optimize(self, entries):
        a = self.agent
        cfg = self.config
        shapes = tuple(x.shape for x in entries)
        if not self.due(shapes):
            return False
        entry_cls = entries.__class__
        mb = cfg.mini_batch_size
        n = entries.state.size(0)
        if self.graph is None:
            from .replay import _PinnedUploader
            self.static = entry_cls(*[x.clone() for x in entries])
            self.idx = torch.zeros(mb, dtype=torch.int64, device=entries.state.device)
            self._up = _PinnedUploader(torch.int64, mb, entries.state.device)
            self.block.graph = None     # (it reads the static buffers it was captured over)
            opts = (a._fused,) if cfg.shared_repr else (a._fused_actor, a._fused_critic)
            if not self.capture(self._bodies(entry_cls), shapes, opts):
                return False
        else:
            for st, x in zip(self.static, entries):
                st.copy_(x)
        if cfg.shared_repr and n % mb == 0 and getattr(cfg, 'graph_ppo_block', True):
            return self._optimize_block(entry_cls, n, mb)
        graphs = self.graph
        out3 = self.out['all' if cfg.shared_repr else 'fwd']
        for _ in range(cfg.optimization_epochs):
            for batch_indices in random_sample(np.arange(n), mb):
                if len(batch_indices) != mb:          # remainder minibatch: eager, optimisers stay in graph mode
                    bi = tensor(batch_indices).long()
                    if cfg.shared_repr:
                        a._fused.prepare_step()
                        last = a._minibatch(entry_cls(*[x[bi] for x in self.static]), prepared=True)
                    else:
                        last = self._eager_split(entry_cls(*[x[bi] for x in self.static]))
                    continue
                self._up.upload_into(self.idx, np.asarray(batch_indices, dtype=np.int64))
                if cfg.shared_repr:
                    a._fused.prepare_step()
                    graphs['all'].replay()
                else:
                    graphs['fwd'].replay()
                    graphs['both' if self._prepare_split(out3) else 'critic'].replay()
                last = out3
        a.last_loss = last
        return True

    def _optimize_block(self, entry_cls, n, mb):
        """shared_repr with full minibatches only (ppo_pixel: 4 epochs x 4 minibatches of 256): the WHOLE optimisation phase is one
        captured graph -- minibatch j gathers its rows by row j of one [epochs x n / mb, mb] index block and reads its Adam scalars
        from row j of one [., 2] block, both uploaded once per rollout -- instead of a graph launch and two uploads per minibatch
        (32 copies of ~4 us in the stream + 15 launch gaps per agent step: profiles/r05t_kernel_stats_ppo_pixel_8.txt).  The
        permutations are drawn exactly as the per-minibatch loop draws them; same kernels, same arguments: same parameters."""
        a = self.agent
        cfg = self.config
        k = cfg.optimization_epochs * (n // mb)
        opt = a._fused
        b = self.block
        b.due(k)        # (usable() has answered for the switch and for a failure: this drops the graph when k changes)
        if b.graph is None:
            from .replay import _PinnedUploader
            idx_all = torch.zeros((k, mb), dtype=torch.int64, device=self.static.state.device)
            hyper = opt.enable_block_mode(k)
            keep = opt._hyper_dev

            def phase():
                for j in range(k):
                    opt._hyper_dev = hyper[j]
                    out3 = a._minibatch(entry_cls(*ops.gather_rows(list(self.static), idx_all[j])), prepared=True)
                return out3
            try:
                captured = b.capture(phase, k, (opt,))
            finally:
                opt._hyper_dev = keep
            if not captured:
                return False
            self.block_idx, self._block_up = idx_all, _PinnedUploader(torch.int64, k * mb, idx_all.device)
        batches = []
        for _ in range(cfg.optimization_epochs):
            batches += [np.asarray(bi, dtype=np.int64) for bi in random_sample(np.arange(n), mb)]
        self._block_up.upload_into(self.block_idx.view(-1), np.concatenate(batches))
        opt.prepare_steps(k)        # (not Region.replay(): its k steps' scalars go up as one block)
        b.graph.replay()
        a.last_loss = b.out
        return True

    def _eager_split(self, entry):
        """remainder minibatch with separate optimisers in graph mode."""
        p, out3, grads = self._forward_loss(entry)
        self._step_split(p, grads, self._prepare_split(out3))
        return out3
