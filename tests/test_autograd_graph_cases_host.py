"""Proves the table of tests/autograd_graph_cases.py on the CPU -- the integer bounds hold, every graph's float64 reference agrees
with the float32 CPU run of itself within the bar (so the inputs carry the bar), every graph has the fan-out and creation order it
is named for -- and holds the masked-gradient hand-over (nets._mark_masked / nets._already_masked) to a fan-out graph with toy
Functions: a gradient that autograd accumulated IN PLACE into the marked tensor must not count as masked."""
import numpy as np
import pytest
import torch

import autograd_graph_cases as G

INTEGER = [c for c in G.CASES if c["kind"] == "integer"]
RANDOM = [c for c in G.CASES if c["kind"] == "random"]


def test_the_table_holds_every_graph_of_the_list():
    names = set(G.ids())
    for stem in ("chain-koc-b2", "chain-koc-b3", "chain-oihw-b2", "chain-oihw-b3", "two-markers-ab", "two-markers-ba", "stale-mark-then-chain",
                 "retain-graph-twice", "siamese-linear", "siamese-noisy", "siamese-body", "partial-covers"):
        assert stem in names, stem
    for stem in ("fanout-linear", "fanout-noisy", "fanout-policy", "fanout-conv3", "fanout-fc4"):
        assert {"%s-%s" % (stem, o) for o in G.ORDERS} <= names, stem
    assert all(c["title"] and c["act_bwd"] >= 0 for c in G.CASES)
    assert set(G.by_name("siamese-body")["modes"]) == {"accumulate", "direct", "deferred-rmsprop", "deferred-adam"}
    for c in G.CASES:       # conv graphs: Nature geometry at batch 2 or 3, dims of the others at most 48
        for key, a in G.operands(c["name"]).items():
            if a.dtype == np.uint8:
                assert a.shape[0] in (2, 3) and a.shape[1:] == (4, 84, 84)
            elif not key.startswith(("body.", "head.")) and a.ndim <= 2 and c["storage"] is None:
                assert max(a.shape) <= 48, (c["name"], key, a.shape)


@pytest.mark.parametrize("c", INTEGER, ids=G.ids(INTEGER))
def test_integer_graphs_stay_below_2_to_the_24(c):
    ops = G.operands(c["name"])
    for key, a in ops.items():
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 4, key
        if key.endswith((".ein", ".eout", ".eb")):
            assert set(np.unique(a)) <= set(G.NOISE_INTS), key        # f(e) = sign(e) sqrt|e| is an integer
    bound = G.int_bound(c["name"])
    print("autograd graphs %s: largest partial sum %d" % (c["name"], bound))
    assert 0 < bound < G.INT_LIMIT
    grads, fwd = G.reference(c["name"])
    for key, g in list(grads.items()) + list(fwd.items()):
        assert np.array_equal(g, np.round(g)) and np.abs(g).max() <= bound, key
    assert any(np.abs(g).max() > 0 for g in grads.values())


def _gates(fwd):
    return {k: (y > 0).astype(np.float64) for k, y in fwd.items()}


@pytest.mark.parametrize("c", G.CASES, ids=G.ids())
def test_float32_run_of_the_reference_stays_within_the_bar(c):
    """Same graph, same gates (the float64 run's), float32 arithmetic on the CPU: err / scale per tensor against BAR."""
    grads, fwd = G.reference(c["name"])
    g32, f32 = G.reference_with_gates(c["name"], _gates(fwd), dtype=torch.float32)
    worst = 0.0
    for want, got in ((grads, g32), (fwd, f32)):
        assert set(want) == set(got)
        for key in want:
            scale = np.abs(want[key]).max()
            err = np.abs(got[key] - want[key]).max()
            assert err <= G.BAR * scale, "%s %s: float32 CPU run %.3g of scale %.3g" % (c["name"], key, err / max(scale, 1e-300), scale)
            worst = max(worst, err / scale if scale > 0 else 0.0)
    print("autograd graphs %s: float32 CPU run at most %.3g of scale (bar %.0e)" % (c["name"], worst, G.BAR))
    if c["kind"] == "integer":
        assert worst == 0.0
    for key in G.param_names(c["name"]) + G.input_names(c["name"]):
        assert key in grads, key
    for p in G.UNREACHED.get(c["name"], ()):
        assert not grads[p + ".w"].any() and not grads[p + ".b"].any()


def _reads(node, leaf, depth=2):
    """Does the node take the leaf as an input, directly or through one more node (F.linear reads its weight through a transpose)?"""
    return any(m is not None and (getattr(m, "variable", None) is leaf or (depth > 1 and _reads(m, leaf, depth - 1)))
               for m, _ in node.next_functions)


def _is_tap(node):
    return type(node).__name__.startswith("MulBackward")


@pytest.mark.parametrize("c", G.CASES, ids=G.ids())
def test_graphs_have_the_fan_out_and_creation_order_they_are_named_for(c):
    ref = G.RefBackend(c["name"]).run(c["build"], c["order"])
    assert ref.relu_node, "no fused ReLU in the graph"
    for key in ref.relu_node:
        cons = G.consumers(ref, key)
        assert len(cons) == c["fan"].get(key, 1), (c["name"], key, [type(n).__name__ for n in cons])
    for key in (c["fan"] if c["order"] else ()):
        cons = sorted(G.consumers(ref, key), key=lambda n: n._sequence_nr())
        taps = [n for n in cons if _is_tap(n)]
        if c["name"].startswith("two-markers"):
            assert not taps and all(n in ref.marking_nodes for n in cons)
            first = "la.w" if c["order"] == "plain-first" else "lb.w"
            assert _reads(cons[0], ref.leaves[first])
            continue
        assert len(taps) == 1, (c["name"], key)
        marking = [n for n in cons if not _is_tap(n)]
        # (fc4 reads y3 through a view: the node that consumes y3 is the view, the marking layer is the view's consumer)
        assert all(n in ref.marking_nodes or type(n).__name__.startswith(("ViewBackward", "ReshapeAliasBackward", "UnsafeViewBackward"))
                   for n in marking)
        if c["order"] == "plain-first":
            assert taps[0]._sequence_nr() < min(n._sequence_nr() for n in marking)      # the marking backward runs first
        else:
            assert taps[0]._sequence_nr() > max(n._sequence_nr() for n in marking)      # the tap's backward runs first
    n_apps = {p: sum(1 for k in ref.relu_node if k.startswith(p + ".") or k.startswith(p + "#")) for p in G.SHARED.get(c["name"], ())}
    for p, n in n_apps.items():
        assert n == (8 if p == "body" else 2), (p, n)       # applied twice (the body: four layers each time)


# ---------------------------------------------------------------------------------- the hand-over on a fan-out graph
class _Producer(torch.autograd.Function):
    """y = relu(x), the way the fused-ReLU layers go backward: no mask of its own when the gradient is the marked one."""
    hits = []

    @staticmethod
    def forward(ctx, x):
        y = torch.relu(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        from deeprl_amd import nets
        y, = ctx.saved_tensors
        hit = nets._already_masked(dy)
        _Producer.hits.append((hit, dy._version))
        return dy if hit else dy * (y > 0)


class _Marking(torch.autograd.Function):
    """3 * y of a fused-ReLU output y, handing down the gradient of y's PRE-activation and marking it."""

    @staticmethod
    def forward(ctx, y):
        ctx.save_for_backward(y)
        return 3 * y

    @staticmethod
    def backward(ctx, g):
        from deeprl_amd import nets
        y, = ctx.saved_tensors
        dx = 3 * g * (y > 0)
        nets._mark_masked(dx)
        return dx


def _toy(order, fan_out=True):
    x = torch.tensor([-1.0, 2.0, -3.0, 4.0], requires_grad=True)
    _Producer.hits = []
    y = _Producer.apply(x)
    if not fan_out:
        loss = _Marking.apply(y).sum()
    elif order == "plain-first":
        plain = (2 * y).sum()
        loss = plain + _Marking.apply(y).sum()
    else:
        marked = _Marking.apply(y).sum()
        loss = marked + (2 * y).sum()
    loss.backward()
    return x.grad.clone(), list(_Producer.hits)


@pytest.mark.parametrize("order", G.ORDERS)
def test_a_gradient_accumulated_into_the_marked_tensor_is_not_taken_for_masked(order):
    """y = relu(x) into (2 y).sum() and into a marking 3 y.  With the plain consumer created first the marking backward runs
    first, and autograd's input buffer adds the plain gradient INTO the marked tensor: same object, same address, version + 1.
    A mark matched by address alone made the producer skip its mask there: [2, 5, 2, 5] instead of [0, 5, 0, 5]."""
    got, hits = _toy(order)
    x = torch.tensor([-1.0, 2.0, -3.0, 4.0], dtype=torch.float64, requires_grad=True)
    y = torch.relu(x)
    ((2 * y).sum() + (3 * y).sum()).backward()
    print("fan-out %s: producer saw (hit, version) %s, gradient %s, wanted %s" % (order, hits, got.tolist(), x.grad.tolist()))
    assert hits and not hits[0][0], "the producer took an accumulated gradient (version %d) for the masked one" % hits[0][1]
    assert torch.equal(got.double(), x.grad)


def test_a_chain_still_hands_the_mask_down():
    got, hits = _toy(None, fan_out=False)
    assert hits == [(True, 0)] and got.tolist() == [0.0, 3.0, 0.0, 3.0]


def test_flush_fold_folds_one_layer_and_leaves_the_others_registered(monkeypatch):
    """optim.FusedOptimizer.flush_fold (host logic, kernels mocked): a shared conv layer reached a second time folds the slabs
    its first reach registered, before autograd accumulates; other layers' slabs wait for step() as before."""
    from deeprl_amd import ops, optim
    calls = []
    monkeypatch.setattr(ops, "grad_sqnorm_segs", lambda grad, segs, partials: calls.append((grad.data_ptr(), grad.numel(), [s[:2] + s[3:] for s in segs])) or 7)
    monkeypatch.setattr(ops, "norm_partials_max", lambda: 8)
    params = [torch.nn.Parameter(torch.zeros(n)) for n in (32, 64)]
    opt = optim.FusedOptimizer.adopt(torch.optim.RMSprop(params, lr=0.0))
    g = opt.flat.grad
    slabs = torch.zeros(4 * 64)
    assert opt.defer_fold(g[0:32], 32, slabs, 4) and opt.defer_fold(g[32:96], 64, slabs, 3)
    opt.flush_fold(g[32:96])
    assert calls == [(g[32:96].data_ptr(), 64, [(0, 64, 64, 3)])]
    assert [s[0] for s in opt._pending_folds] == [0]
    opt.flush_fold(g[32:96])                # nothing registered for it any more
    opt.flush_fold(None)
    assert len(calls) == 1 and [s[0] for s in opt._pending_folds] == [0]
