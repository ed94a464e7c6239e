"""Edge-shape parity of the fused DQN learner (csrc/learner.hip) against a float64 reference of the whole update, at the batch
sizes, action counts and head sizes where its code changes path: batches 1 .. 128 around the conv workgroup-shape switches (16 | 17,
127 | 128), the chained launches' range (17 .. 32), the W4 prefetch of the head launch (B % 8 == 0) and the late fold (32 | 33);
1 .. 64 actions around the head's register / fallback switch (8 | 9, with double-Q 5 | 6); the categorical head up to n_out = 4096
and down to two atoms, the quantile head with more and fewer atoms than samples.

Cases, the reference and the bar live in tests/learner_edge_cases.py; tests/test_learner_edge_cases_host.py proves on the CPU that
the inputs carry the bar, that every first update is free of ambiguous ReLU gates and that the expected path flags follow from the
library's conditions.  Here every case
  asserts its path   DQNLearner.path_flags() equals the table's flags (a condition that silently widens or narrows fails here)
  in order           DQNLearner.update(idx): graph capture, two replays, one eager update -- at variant 0 and at the library default,
                     each update against float64 from the learner's own exported state before it: head outputs, loss vector, loss,
                     gradient norm, parameters; after the first update both optimizer-state tensors of every parameter tensor (=
                     every gradient element, signed); at variant 0 the flat gradient too
  actor              set_env_steps + act (variant 0; the default's ring actor owns its environment: the pipelined cases check it):
                     action values against float64, the stored action against the decision rule on the kernel's own values;
                     n_env = 1 .. 8 twice through the five-entry graph cache against the eager launches, bit for bit
  pipelined          DQNLearnerBench(async_actor=True) at the library default, 8 agent steps on a 512-slot ring: per step as above
                     along oracle/async_schedule_oracle.py's schedule, stored actions, ring frames bit for bit; for batches 17 .. 32
                     the same seeds without synchronisation, with the chains cleared and with the opt-in chains set end on
                     identical bits
  limits             out-of-range configurations fail with the library's invalid-argument error
No update or step may return an error (DraError: the ctypes layer raises on every non-zero return, DRA_ETIMEDOUT included), and no
learner may end with its timeout flag set.  Every measured error / scale goes to the parity log."""
import numpy as np
import pytest
import torch

import fake_envs
import learner_edge_cases as E
from parity_log import record_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    from deeprl_amd.support import select_device, Config
    select_device(0)
    return Config.DEVICE


@pytest.fixture(scope="module")
def dra(dev):
    import deeprl_amd as d
    return d


def _ids(cases):
    return [c["name"] for c in cases]


def _nets(c):
    from deeprl_amd.nets import CategoricalNet, NatureConvBody, QuantileNet, VanillaNet
    if c["head"] == "c51":
        make = lambda: CategoricalNet(c["A"], c["atoms"], NatureConvBody())
    elif c["head"] == "qr":
        make = lambda: QuantileNet(c["A"], c["atoms"], NatureConvBody())
    else:
        make = lambda: VanillaNet(c["A"], NatureConvBody())
    return make(), make()


def _learner(c, net, tgt, ring, variant, **over):
    from deeprl_amd import learner as LM
    h = E.HEADS[c["head"]]
    kw = dict(batch=c["B"], n_actions=c["A"], gamma_n=E.GAMMA, gradient_clip=h["clip"], lr=h["lr"], alpha=h["alpha"], eps=h["eps"],
              centered=c["head"] == "vanilla", double_q=c["double_q"], variant=variant, cu_partition=False,
              head_kind={"vanilla": LM.HEAD_VANILLA, "c51": LM.HEAD_CATEGORICAL, "qr": LM.HEAD_QUANTILE}[c["head"]],
              n_atoms=c["atoms"], v_min=h.get("v_min", 0.0), v_max=h.get("v_max", 0.0),
              optimizer=LM.OPT_ADAM if h["optimizer"] == "adam" else LM.OPT_RMSPROP, betas=h.get("betas", (0.9, 0.999)))
    kw.update(over)
    return LM.DQNLearner(net, tgt, ring, **kw)


def _state(learner):
    """export_state() as learner_edge_cases.reference_update takes it."""
    st = learner.export_state()
    return {k: {n: v.numpy() for n, v in st[k].items()} for k in ("params", "target", "state1", "state2")}


def _outputs(d, learner, ref):
    """The update's outputs in the shapes of the reference's."""
    vec = d.ops._wrap_device_pointer(learner.delta.data_ptr(), ref["vec"].size, torch.float32).cpu().numpy().copy()
    return dict(out=learner.q.cpu().numpy().reshape(ref["out"].shape).copy(), vec=vec, loss=float(learner.loss.item()),
                norm=float(learner.norm.item()))


def _judge_update(c, tag, it, got, ref, first, margins):
    ambiguous = ref["margin"] < E.MARGIN
    margins.append(ref["margin"])
    fig = E.measure(c, got, ref, with_state=first)
    # (every tensor's error / scale: tools/learner_edges_summary.py keeps the maximum over a case's updates)
    record_parity("learner_edges[%s %s] update %d%s" % (c["name"], tag, it, " (ambiguous ReLU gate)" if ambiguous else ""),
                  relu_margin=ref["margin"], **fig)
    assert not (first and ambiguous), "%s: the first update has an ambiguous ReLU gate (margin %g)" % (c["name"], ref["margin"])
    E.judge(c, fig, ambiguous, "%s update %d" % (tag, it))


@pytest.mark.parametrize("tag", ["variant0", "default"])
@pytest.mark.parametrize("c", E.IN_ORDER_CASES, ids=_ids(E.IN_ORDER_CASES))
def test_in_order_update_matches_float64(dra, c, tag):
    d = dra
    variant = 0 if tag == "variant0" else d.ops.get_tuning()
    ring = d.ops.Ring(E.CAP, 7056, 8, 4, 1, E.GAMMA)
    learner = None
    try:
        ring.fill_synthetic(0, E.CAP, 0, E.RING_SEED, n_actions=c["A"], done_period=E.DONE_PERIOD)
        torch.cuda.synchronize()
        net, tgt = _nets(c)
        s0 = E.initial_state(c)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in s0["params"].items()})
        tgt.load_state_dict({k: torch.from_numpy(v) for k, v in s0["target"].items()})
        learner = _learner(c, net, tgt, ring, variant)
        want_flags = E.expected_flags(c, learner.variant)
        margins = []
        for it, idx in enumerate(E.case_indices(c)):
            before = _state(learner)
            if it == 0:
                for k in ("params", "target"):
                    for n, v in s0[k].items():
                        assert np.array_equal(before[k][n], v), "the learner does not hold the case's initial %s: %s" % (k, n)
                ref = E.first_update(c["name"], True)
            else:
                ref = E.reference_update(c, before, E.gather(c, idx), it + 1)
            learner.update(idx, use_graph=it < 3)            # capture, two replays, then the eager path
            learner.synchronize()
            got = _outputs(d, learner, ref)
            got.update(_state(learner))
            if variant == 0:    # the norm-then-step form leaves the whole (unclipped) gradient in the flat buffer
                got["grads"] = {n: p.grad.detach().cpu().numpy() for n, p in net.named_parameters()}
            _judge_update(c, tag, it, got, ref, it == 0, margins)
            flags = learner.path_flags()
            assert not flags["timed_out"]
            for k, v in want_flags.items():
                assert flags[k] == v, "%s %s: path flag %s is %s, the table says %s (%s)" % (c["name"], tag, k, flags[k], v, flags)
            if c["head"] == "vanilla":
                assert flags["head_launches"] >= 1
        assert sum(m < E.MARGIN for m in margins[1:]) <= 1, "more than one ambiguous later update: %s" % margins
        if c["actor"] and variant == 0:
            _check_actor(d, c, learner, ring, net)
    finally:
        if learner is not None:
            learner.close()
        ring.close()


def _check_actor(d, c, learner, ring, net):
    """The device actor's env step on frames already in the ring: a stack that wraps the ring end, the greedy and the random
    branch, eager and graphed."""
    a, cap = c["A"], E.CAP
    frames = E.ring_oracle(a).state
    params = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    for newest, eps, rnd, dice, graph in ((1, 0.5, a - 1, 0.9, False), (cap - 1, 0.5, 0, 0.1, True), (100, 0.0, min(1, a - 1), 0.0, True)):
        learner.set_env_steps([newest], [-1], [rnd], [dice], [eps])          # counter < 0: the frame is already in the ring
        learner.act(use_graph=graph)
        learner.synchronize()
        slots = [(newest - 3 + j) % cap for j in range(4)]
        want = E.reference_actor_q(c, params, frames[slots])
        got = learner.actor_q.cpu().numpy().astype(np.float64)
        fig = E._scaled(got, want)
        record_parity("learner_edges[%s variant0] actor at slot %d" % (c["name"], newest), actor_q=fig)
        assert fig <= E.BAR, "%s: actor_q at slot %d: error / scale %.3g" % (c["name"], newest, fig)
        decided = rnd if dice < eps else int(np.argmax(got))
        stored = int(d.ops._wrap_device_pointer(ring.pointers()[1], cap, torch.int64)[newest].item())
        assert stored == decided, "%s: stored action %d, the rule on the kernel's own values gives %d" % (c["name"], stored, decided)
    assert not learner.path_flags()["timed_out"]


def test_actor_graph_cache_cycles_more_keys_than_slots(dra):
    """The first-generation actor's graph cache keeps five (parameter block, n_env) entries; kMaxEnvSteps is 8.  Two learners on
    the same seeded parameters and ring contents run act() with n_env = 1 .. 8, twice -- one through the cached graphs (the
    second round meets evicted entries and recaptures them), one eagerly.  After every call the frames and actions of the slots
    written and actor_q are the same bits on both (the same kernels on the same data), and the frames are the documented counter
    hash."""
    d = dra
    from deeprl_amd.learner import DQNLearner
    from oracle.synth_oracle import synth_transitions
    cap, a, seed, period = 64, 4, 11, 5
    p_np = fake_envs.numpy_params(fake_envs.nature_vanilla_shapes(a), 17)
    sides = []
    try:
        for graph in (True, False):
            ring = d.ops.Ring(cap, 7056, 8, 4, 1, E.GAMMA)
            sides.append([ring, None, graph])
            ring.fill_synthetic(0, cap, 0, seed, n_actions=a, done_period=period)
            torch.cuda.synchronize()
            net, tgt = d.VanillaNet(a, d.NatureConvBody()), d.VanillaNet(a, d.NatureConvBody())
            for m in (net, tgt):
                m.load_state_dict({k: torch.from_numpy(v) for k, v in p_np.items()})
            sides[-1][1] = DQNLearner(net, tgt, ring, 1, a, E.GAMMA, 5.0, 0.00025, 0.95, 0.01, centered=True, env_seed=seed,
                                      env_done_period=period, variant=0, cu_partition=False)
        schedule = list(range(1, 9)) * 2
        want_frames, _, _, _ = synth_transitions(cap, sum(schedule), 7056, seed=seed, n_actions=a, done_period=period)
        rng = np.random.RandomState(5)
        pos, done = 0, 0
        for call, n in enumerate(schedule):
            slots = [(pos + e) % cap for e in range(n)]
            rnd = [int(rng.randint(a)) for _ in range(n)]
            dice = [float(rng.rand()) for _ in range(n)]
            got = []
            for ring, learner, graph in sides:
                learner.set_env_steps(slots, [cap + done + e for e in range(n)], rnd, dice, [0.5] * n)
                learner.act(use_graph=graph)
                learner.synchronize()
                frames = d.ops._wrap_device_pointer(ring.pointers()[0], cap * 7056, torch.uint8).cpu().numpy().reshape(cap, 7056)
                actions = d.ops._wrap_device_pointer(ring.pointers()[1], cap, torch.int64).cpu().numpy()
                got.append((frames[slots].copy(), actions[slots].copy(), learner.actor_q.cpu().numpy().copy()))
            where = "call %d (n_env %d)" % (call, n)
            assert np.array_equal(got[0][0], got[1][0]), "%s: ring frames differ between graph and eager" % where
            assert np.array_equal(got[0][1], got[1][1]), "%s: stored actions differ between graph and eager" % where
            assert np.array_equal(got[0][2].view(np.uint32), got[1][2].view(np.uint32)), "%s: actor_q differs" % where
            assert np.array_equal(got[0][0], want_frames[done:done + n]), "%s: the frames are not the counter hash" % where
            pos, done = (pos + n) % cap, done + n
        for _, learner, _ in sides:
            assert not learner.path_flags()["timed_out"]
    finally:
        for ring, learner, _ in sides:
            if learner is not None:
                learner.close()
            ring.close()


# ---- the pipelined path ----------------------------------------------------------------------------------------------------
def _pipeline(d, c, variant, sync_each):
    """PIPE_STEPS agent steps of the async pipeline.  Returns (per-step records or None, final bits, flags, lane, ahead)."""
    from deeprl_amd.learner import DQNLearnerBench
    keep = np.random.get_state()
    d.random_seed(11)
    torch.manual_seed(5)
    bench = DQNLearnerBench(ring_capacity=E.CAP, batch=c["B"], seed=c["seed"], actor=True, async_actor=True, n_actions=c["A"],
                            variant=variant)
    L = bench.learner
    try:
        with torch.cuda.stream(L.stream):        # the prefilled ring with a third of its transitions terminal (frames unchanged)
            bench.ring.fill_synthetic(0, E.CAP, 0, c["seed"], n_actions=c["A"], done_period=E.DONE_PERIOD)
        L.synchronize()
        p0 = fake_envs.numpy_params(fake_envs.nature_vanilla_shapes(c["A"]), E.PARAM_SEEDS[0])
        bench.network.load_state_dict({k: torch.from_numpy(v) for k, v in p0.items()})
        bench.target_network.load_state_dict({k: torch.from_numpy(v) for k, v in p0.items()})
        np.random.seed(c["draw_seed"])
        steps = [dict(before=_state(L))] if sync_each else None
        for k in range(E.PIPE_STEPS):
            bench.step()
            if sync_each:
                L.synchronize()
                steps[-1].update(out=L.q.cpu().numpy().copy(), vec=L.delta.cpu().numpy().copy(), norm=float(L.norm.item()),
                                 after=_state(L))
                steps.append(dict(before=steps[-1]["after"]))
        L.synchronize()
        torch.cuda.synchronize()
        w = d.ops._wrap_device_pointer
        final = dict(p=L.flat.flat.detach().cpu().numpy().copy(), s1=L.state1.cpu().numpy().copy(), s2=L.state2.cpu().numpy().copy(),
                     pt=L.target_flat.flat.detach().cpu().numpy().copy(),
                     frames=w(bench.ring.pointers()[0], E.CAP * 7056, torch.uint8).cpu().numpy().copy(),
                     acts=w(bench.ring.pointers()[1], E.CAP, torch.int64).cpu().numpy().copy())
        return steps[:-1] if sync_each else None, final, L.path_flags(), L.lane_stats(), L.ahead_stats()
    finally:
        np.random.set_state(keep)
        L.close()
        bench.ring.close()


_PIPE_RESULTS = {}


def _default_run(d, c):
    """The synchronised run at the library default: once per case, shared by the tests below."""
    if c["name"] not in _PIPE_RESULTS:
        _PIPE_RESULTS[c["name"]] = _pipeline(d, c, d.ops.get_tuning(), True)
    return _PIPE_RESULTS[c["name"]]


@pytest.mark.parametrize("c", E.PIPELINED_CASES, ids=_ids(E.PIPELINED_CASES))
def test_pipelined_step_matches_float64(dra, c):
    d = dra
    steps, final, flags, lane, ahead = _default_run(d, c)
    want_flags = E.expected_flags(c, flags["variant"], pipelined=True)
    assert not flags["timed_out"]
    for k, v in want_flags.items():
        assert flags[k] == v, "%s: path flag %s is %s, the table says %s (%s)" % (c["name"], k, flags[k], v, flags)
    n_tr = 4 * (E.PIPE_STEPS + 1)                    # the actor ran one agent step ahead
    p0 = fake_envs.numpy_params(fake_envs.nature_vanilla_shapes(c["A"]), E.PARAM_SEEDS[0])
    orc = E.schedule_oracle(c, p0)
    keep = np.random.get_state()
    near_ties, margins = 0, []

    def check_actions(res, first, who):
        nonlocal near_ties
        for e, (act, gap, rnd) in enumerate(res):
            got = int(final["acts"][first + e])
            assert 0 <= got < c["A"]
            if act != got:
                assert (not rnd) and gap < 1e-5, "%s %s env step %d: action %d vs %d, top-2 gap %g" % (c["name"], who, e, act, got, gap)
                near_ties += 1

    try:
        np.random.seed(c["draw_seed"])
        check_actions(orc.actor_step(orc._snapshot(), override_actions=final["acts"][0:4]), 0, "actor(0)")
        for k, s in enumerate(steps):
            idx, batch = orc.sample()
            # actor(k + 1) acts on the parameters update k starts from
            theta = {n: torch.from_numpy(v).to(torch.float64) for n, v in s["before"]["params"].items()}
            check_actions(orc.actor_step(theta, override_actions=final["acts"][4 * (k + 1):4 * (k + 2)]), 4 * (k + 1), "actor(%d)" % (k + 1))
            ref = E.reference_update(c, s["before"], batch, k + 1)
            got = dict(out=s["out"], vec=s["vec"], norm=s["norm"], loss=0.5 * float(np.mean(s["vec"].astype(np.float64) ** 2)))
            got.update(s["after"])
            _judge_update(c, "pipelined", k, got, ref, k == 0, margins)
    finally:
        np.random.set_state(keep)
    assert near_ties <= 1, "more than one float32 near-tie in %d decisions is not plausible" % n_tr
    assert sum(m < E.MARGIN for m in margins[1:]) <= 1, "more than one ambiguous later update: %s" % margins
    assert np.array_equal(final["frames"][:n_tr * 7056], orc.rep.state[:n_tr].reshape(n_tr * 7056)), "ring frames"
    # the untouched part of the ring keeps the prefill's bytes
    assert np.array_equal(final["frames"][n_tr * 7056:], orc.rep.state[n_tr:].reshape(-1)), "ring frames behind the actor's"


CHAINED = [c for c in E.PIPELINED_CASES if c["chained"]]


@pytest.mark.parametrize("c", CHAINED, ids=_ids(CHAINED))
def test_pipelined_chains_are_bit_identical(dra, c):
    """Batches 17 .. 32: the same seeds (i) without a synchronisation between the steps -- the event-free lane runs -- and (ii) with
    FWD_CHAIN | BWD_CHAIN | BWD_CHAIN_FC | HEAD_CHAIN | DEFER_FC4 | TARGET_AHEAD cleared end on the bits of the synchronised run
    at the library default (what the *_is_bit_identical tests of tests/test_gpu_agents.py assert at batch 32, 4 actions)."""
    d = dra
    default = d.ops.get_tuning()
    _, ref_final, ref_flags, _, _ = _default_run(d, c)
    _, final, flags, lane, _ = _pipeline(d, c, default, False)
    assert not flags["timed_out"] and flags["fs"] and flags["fchain"] and flags["bchain"], flags
    assert lane["steps"] > 0, "the event-free lane never ran: %s" % (lane,)
    for k in ref_final:
        assert np.array_equal(final[k], ref_final[k]), ("synchronised after every step vs not", c["name"], k)
    _, final, flags, lane, _ = _pipeline(d, c, default & ~E.CHAIN_BITS, False)
    assert not flags["timed_out"] and not (flags["fchain"] or flags["bchain"] or flags["defer"] or flags["fs"] or flags["ah"]
                                           or flags["head_chain"]), flags
    assert lane["steps"] == 0
    for k in ref_final:
        assert np.array_equal(final[k], ref_final[k]), ("chains set vs cleared", c["name"], k)
    assert float(np.abs(ref_final["p"]).max()) > 0


@pytest.mark.parametrize("c", CHAINED, ids=_ids(CHAINED))
def test_pipelined_opt_in_chains_are_bit_identical(dra, c):
    """... and with the opt-in HEAD_CHAIN (the head launch sized B + nd + nw + 2 A, refused unless nw + 2 A is the partial count of
    the launch it replaces) and TARGET_AHEAD (the target's partial sums from the stash) set: the chained head launch ran, the
    stash was used, the same bits."""
    d = dra
    default = d.ops.get_tuning()
    _, ref_final, _, _, _ = _default_run(d, c)
    variant = default | d.ops.VAR_HEAD_CHAIN | d.ops.VAR_TARGET_AHEAD
    _, final, flags, lane, ahead = _pipeline(d, c, variant, False)
    want = E.expected_flags(c, variant, pipelined=True)
    assert want["head_chain"] and want["ah"] and not want["head_pf"]
    assert not flags["timed_out"]
    for k, v in want.items():
        assert flags[k] == v, "%s: path flag %s is %s, the table says %s (%s)" % (c["name"], k, flags[k], v, flags)
    assert lane["steps"] > 0 and ahead["active"] and ahead["from_stash"] + ahead["in_line"] > 0, (lane, ahead)
    assert ahead["index_mismatch"] == 0, ahead
    for k in ref_final:
        assert np.array_equal(final[k], ref_final[k]), ("opt-in chains vs the default", c["name"], k)


# ---- limits ----------------------------------------------------------------------------------------------------------------
def test_out_of_range_configurations_are_refused(dra):
    """dra_dqn_learner_create checks its configuration before it allocates or launches anything: each of these fails with the
    library's invalid-argument error."""
    d = dra
    from deeprl_amd._lib import DraError
    ring = d.ops.Ring(E.CAP, 7056, 8, 4, 1, E.GAMMA)
    try:
        van, c51, qr = E.by_name("batch5-odd-below-every-switch"), E.by_name("c51-batch5-actions3"), E.by_name("qr-batch7-atoms200-more-than-batch")
        bad = [(van, dict(batch=0)), (van, dict(batch=1025)), (van, dict(n_actions=0)), (van, dict(n_actions=65)), (van, dict(ksplit=0)),
               (van, dict(ksplit=65)), (c51, dict(n_actions=17, n_atoms=241)),        # n_actions * n_atoms = 4097
               (c51, dict(n_atoms=1)), (qr, dict(n_atoms=1)), (c51, dict(v_min=10.0, v_max=10.0)), (c51, dict(v_min=10.0, v_max=-10.0)),
               (qr, dict(n_actions=17, n_atoms=241))]
        for c, over in bad:
            net, tgt = _nets(c)
            with pytest.raises(DraError, match=r"dra_dqn_learner_create failed with code -22"):
                _learner(c, net, tgt, ring, 0, **over)
        # ... and the limits themselves are accepted (n_actions * n_atoms = 4096 and 64 actions are in-order cases above)
        for c, over in ((van, dict(ksplit=1)), (van, dict(ksplit=64))):
            net, tgt = _nets(c)
            _learner(c, net, tgt, ring, 0, **over).close()
    finally:
        ring.close()
