"""Autograd graphs that exercise the three stateful protocols the layer Functions of deeprl_amd/nets.py share through module
globals -- the masked-gradient hand-over (_MASKED), direct gradient writes (direct_param_grads) and deferred conv folds
(FusedOptimizer.defer_fold) -- on graphs autograd may reorder: fan-out of a fused-ReLU output in both creation orders, two marking
consumers, marks nobody consumes, weight sharing, backward passes that miss a parameter.  The graph table, the operand sets and a
float64 reference per graph.  CPU only; tests/test_autograd_graph_cases_host.py proves the table (integer bounds, the inputs carry
the bar, every graph has the fan-out and creation order it is named for), tests/test_gpu_autograd_graphs.py runs the graphs on
the product layers.

A graph is written ONCE, as a function of a backend B: RefBackend below (plain torch ops: F.linear, F.conv2d, relu, log_softmax)
or the device backend of the GPU test (nets.linear, nets.Linear, nets.NoisyLinear, nets.NatureConvBody,
nets.CategoricalActorCriticNet).  B offers
  input(name) / frames(name) / const(name) / action(name)       leaves: float input (with gradient), uint8 frames of the body
                                                                (normalised by 1 / 255), constants, stored actions
  linear(p, x, act, x_relu) / module_linear(p, x)               nets.linear on free parameters / a nets.Linear module (fused ReLU)
  noisy(p, x, act, x_relu)                                      a nets.NoisyLinear module in training mode
  torch_relu(x)                                                 a plain torch.relu on either side
  conv(k, x) / fc4(y3) / body(x)                                NatureConvBody "body": one layer, or the whole forward
  actor_critic(x, action, tap)                                  CategoricalActorCriticNet over FCBody((H,), relu): tap(phi) is
                                                                called on the body's output before (tap_first) or after the heads
and build(B) returns the losses to backpropagate in turn, [(loss, retain_graph)].

Operand sets:
  integer  (the linear-only graphs) every operand in [-4, 4], noise vectors in {-4, -1, 0, 1, 4} (f(e) = sign(e) sqrt|e| is then
           an integer), dims <= 48: every product and partial sum is an integer below 2^24 (int_bound: the same graph on the
           operands' absolute values without gates bounds every partial sum of any summation order), so forward, gates and every
           gradient equal the int64 result bit for bit; a pre-activation of exactly 0 gates to 0 on both sides
  random   (graphs with conv layers, and the policy head whose log-softmax is not integer) the generators of conv_edge_cases
           ("random"); linear weights normal / sqrt(K), biases at 0.1 scale.  Every fused-ReLU gate of the reference is taken from
           the DEVICE's forward output (DESIGN.md's gate caveat: a pre-activation within summation noise of zero may be gated
           either way), the forward itself is compared separately.  Bar: BAR = 1e-5 of the reference's max-abs per tensor.

Expected `act_bwd` launches per graph (the column act_bwd): one per fused-ReLU layer that must apply its own mask.  A layer
whose ONLY consumer marks (x_relu / input_is_relu / masks_input_relu / the policy head on fused-ReLU features) receives the
masked gradient and launches nothing; a layer whose output has a second consumer receives an accumulated gradient and must mask,
whichever consumer was created first; a mask applied to an already masked gradient changes nothing ((y > 0) is 0 or 1)."""
import functools
import zlib

import numpy as np

import conv_edge_cases as CE

BAR = 1e-5
F, D = np.float32, np.float64
INT_LIMIT = 1 << 24
NOISE_INTS = (-4, -1, 0, 1, 4)
ORDERS = ("plain-first", "marking-first")      # which consumer of the fused-ReLU output is created first in the forward


# ------------------------------------------------------------------------------------------------------------ graphs
def _sum(t, c):
    return (t * c).sum()


def _fan(B, h, marking, order, cname="ch"):
    """h feeds a marking consumer and a plain tap (h * c).sum(), created in the given order -> (marking output, tap)."""
    if order == "plain-first":
        t = _sum(h, B.const(cname))
        return marking(h), t
    m = marking(h)
    return m, _sum(h, B.const(cname))


def build_chain_linear(B, order=None):
    h = B.linear("l0", B.input("x"), "relu")
    return [(_sum(B.linear("l1", h, None, True), B.const("cm")), False)]


def build_fanout_linear(B, order):
    h = B.linear("l0", B.input("x"), "relu")
    m, t = _fan(B, h, lambda h: B.linear("l1", h, None, True), order)
    return [(_sum(m, B.const("cm")) + t, False)]


def build_chain_noisy(B, order=None):
    h = B.linear("l0", B.input("x"), "relu")
    return [(_sum(B.noisy("n1", h, None, True), B.const("cm")), False)]


def build_fanout_noisy(B, order):
    h = B.linear("l0", B.input("x"), "relu")
    m, t = _fan(B, h, lambda h: B.noisy("n1", h, None, True), order)
    return [(_sum(m, B.const("cm")) + t, False)]


def build_two_markers(B, order):
    """order "plain-first" = linA created first, "marking-first" = linB created first (both mark)."""
    h = B.linear("l0", B.input("x"), "relu")
    if order == "plain-first":
        a = B.linear("la", h, None, True)
        b = B.linear("lb", h, None, True)
    else:
        b = B.linear("lb", h, None, True)
        a = B.linear("la", h, None, True)
    return [(_sum(a, B.const("cm")) + _sum(b, B.const("cm2")), False)]


def build_stale_then_chain(B, order=None):
    """A marking consumer on a plain torch.relu (nobody consumes its mark), then an unrelated fused-ReLU chain."""
    h = B.torch_relu(B.linear("l0", B.input("x"), None))
    first = _sum(B.linear("l1", h, None, True), B.const("cm"))
    second = _sum(B.linear("l2", B.input("x2"), "relu"), B.const("ch"))
    return [(first, False), (second, False)]


def build_retain_twice(B, order=None):
    h = B.linear("l0", B.input("x"), "relu")
    loss = _sum(B.linear("l1", h, None, True), B.const("cm"))
    return [(loss, True), (loss, False)]


def build_siamese_linear(B, order=None):
    s = B.module_linear("ls", B.input("x")) + B.module_linear("ls", B.input("x2"))
    return [(_sum(B.linear("lh", s, None, False), B.const("cm")), False)]


def build_siamese_noisy(B, order=None):
    s = B.noisy("ns", B.input("x"), "relu", False) + B.noisy("ns", B.input("x2"), "relu", False)
    return [(_sum(B.linear("lh", s, None, False), B.const("cm")), False)]


def build_partial(B, order=None):
    """"lu" belongs to the optimizer but not to the graph that is backpropagated."""
    B.touch("lu")
    h = B.linear("l0", B.input("x"), "relu")
    return [(_sum(B.linear("l1", h, None, True), B.const("cm")), False)]


def build_policy_chain(B, order=None):
    lp, ent, v = B.actor_critic(B.input("x"), B.action("a"), None, False)
    return [(_sum(lp, B.const("clp")) + _sum(ent, B.const("cent")) + _sum(v, B.const("cv")), False)]


def build_fanout_policy(B, order):
    taps = []
    lp, ent, v = B.actor_critic(B.input("x"), B.action("a"), lambda phi: taps.append(_sum(phi, B.const("ch"))), order == "plain-first")
    return [(_sum(lp, B.const("clp")) + _sum(ent, B.const("cent")) + _sum(v, B.const("cv")) + taps[0], False)]


def build_chain_body(B, order=None):
    return [(_sum(B.module_linear("head", B.body(B.frames("x"))), B.const("cm")), False)]


def _tail(B, y3):
    return _sum(B.module_linear("head", B.fc4(y3)), B.const("cm"))


def build_fanout_conv3(B, order):
    y2 = B.conv(2, B.conv(1, B.frames("x")))
    y3, t = _fan(B, y2, lambda y: B.conv(3, y), order, "c2")
    return [(_tail(B, y3) + t, False)]


def build_fanout_fc4(B, order):
    y3 = B.conv(3, B.conv(2, B.conv(1, B.frames("x"))))
    phi, t = _fan(B, y3, lambda y: B.fc4(y), order, "c3")
    return [(_sum(B.module_linear("head", phi), B.const("cm")) + t, False)]


def build_siamese_body(B, order=None):
    s = B.body(B.frames("x")) + B.body(B.frames("x2"))
    return [(_sum(B.module_linear("head", s), B.const("cm")), False)]


# dims of the linear graphs: batch 5, 6 inputs, 7 hidden units, 3 outputs (odd everywhere, one partial tile of every kernel);
# "wide" repeats the fan-out at the 48 the issue allows
NB, NK, NH, NO, NA = 5, 6, 7, 3, 3
_X, _X2 = ("input", (NB, NK)), ("input", (NB, NK))
_L0, _L1 = ("lin", NH, NK), ("lin", NO, NH)
_CM, _CH = ("const", (NB, NO)), ("const", (NB, NH))
_BODY = {"body": ("body",), "head": ("lin", NO, 512)}


def _case(name, title, build, spec, act_bwd, kind="integer", order=None, modes=("accumulate", "direct"), storage=None, fan=None,
          optimizer=False):
    """fan: {relu key: number of consumers of that fused-ReLU output in the REFERENCE graph} (1 where not listed; the policy head,
    one node on the device, is two there: fc_action and fc_critic); storage: "koc" (the body's
    parameters adopted by a FusedOptimizer) | "oihw" (a freshly built body) | None (no body); optimizer: the free parameters are
    adopted by a FusedOptimizer as well (needed by `covers` and by the deferred mode)."""
    return dict(name=name, title=title, build=build, spec=spec, act_bwd=act_bwd, kind=kind, order=order, modes=tuple(modes),
                storage=storage, fan=fan or {}, optimizer=optimizer or storage == "koc")


def _both(name, title, build, spec, act_bwd, fan, **kw):
    return [_case("%s-%s" % (name, o), "%s, %s" % (title, "the plain tap created first" if o == "plain-first" else
                                                  "the marking consumer created first"), build, spec, act_bwd, order=o, fan=fan, **kw)
            for o in ORDERS]


def _frames(batch):
    return ("frames", batch)


def _body_spec(batch, **more):
    return dict(_BODY, x=_frames(batch), cm=("const", (batch, NO)), **more)


ALL = "accumulate", "direct", "deferred-rmsprop", "deferred-adam"
CASES = (
    # 1. chains: the hand-over must be LIVE.  KOC: conv3, conv2 and conv1 each receive a hit, only fc4 masks for itself (the plain
    # head does not mark).  OIHW: fc4 marks, so conv3 receives a hit; _ConvFn never marks, so conv2 and conv1 mask for themselves.
    [_case("chain-%s-b%d" % (st, b), "NatureConvBody + a plain Linear head on uint8 frames, %s weights, batch %d" % (st.upper(), b),
           build_chain_body, _body_spec(b), 1 if st == "koc" else 3, kind="random", storage=st) for st in ("koc", "oihw") for b in (2, 3)] +
    [_case("chain-linear", "fused-ReLU Linear under a marking Linear: the mask is handed down", build_chain_linear,
           dict(x=_X, l0=_L0, l1=_L1, cm=_CM), 0),
     _case("chain-noisy", "fused-ReLU Linear under a marking NoisyLinear: the mask is handed down", build_chain_noisy,
           dict(x=_X, l0=_L0, n1=("noisy", NO, NH), cm=_CM), 0),
     _case("chain-policy", "fused-ReLU FCBody under the policy head: the mask is handed down", build_policy_chain,
           dict(x=_X, ac=("ac", NK, NH, NA), a=("action", NB, NA), clp=("const", (NB,)), cent=("const", (NB,)), cv=("const", (NB,))),
           0, kind="random", fan={"ac.body#0": 2})] +
    # 2. fan-out: the layer below receives an ACCUMULATED gradient in either creation order and must mask for itself
    _both("fanout-linear", "fused-ReLU h into nets.linear(x_relu=True) and into (h * c).sum()", build_fanout_linear,
          dict(x=_X, l0=_L0, l1=_L1, cm=_CM, ch=_CH), 1, {"l0#0": 2}) +
    _both("fanout-linear-wide", "the same at 48 x 48 x 48, batch 33", build_fanout_linear,
          dict(x=("input", (33, 48)), l0=("lin", 48, 48), l1=("lin", 48, 48), cm=("const", (33, 48)), ch=("const", (33, 48))), 1, {"l0#0": 2}) +
    _both("fanout-noisy", "fused-ReLU h into a NoisyLinear with masks_input_relu and into (h * c).sum()", build_fanout_noisy,
          dict(x=_X, l0=_L0, n1=("noisy", NO, NH), cm=_CM, ch=_CH), 1, {"l0#0": 2}) +
    _both("fanout-policy", "FCBody's fused-ReLU phi into the policy head and into (phi * c).sum()", build_fanout_policy,
          dict(x=_X, ac=("ac", NK, NH, NA), a=("action", NB, NA), clp=("const", (NB,)), cent=("const", (NB,)), cv=("const", (NB,)), ch=_CH),
          1, {"ac.body#0": 3}, kind="random") +
    # conv3 marks: fc4 masks for itself, conv2 masks for itself (accumulated), conv3 and conv1 receive hits
    _both("fanout-conv3", "y2 into conv3 and into (y2 * c).sum(), batch 3", build_fanout_conv3,
          _body_spec(3, c2=("const", (3, 64, 9, 9))), 2, {"body.conv2#0": 2}, kind="random", storage="koc") +
    # fc4 marks: fc4 and conv3 (accumulated) mask for themselves, conv2 and conv1 receive hits
    _both("fanout-fc4", "y3 into fc4 (through a view) and into (y3 * c).sum(), batch 3", build_fanout_fc4,
          _body_spec(3, c3=("const", (3, 64, 7, 7))), 2, {"body.conv3#0": 2}, kind="random", storage="koc") +
    # 3. two marking consumers: the second mark replaces the first, the sum is no marked tensor: the layer below masks (harmlessly)
    [_case("two-markers-%s" % ("ab" if o == "plain-first" else "ba"), "h into linA(x_relu=True) and linB(x_relu=True), lin%s created first" %
           ("A" if o == "plain-first" else "B"), build_two_markers,
           dict(x=_X, l0=_L0, la=_L1, lb=_L1, cm=_CM, cm2=_CM), 1, order=o, fan={"l0#0": 2}) for o in ORDERS] +
    # 4. stale marks
    [_case("stale-mark-then-chain", "a marking consumer on a plain torch.relu, then an unrelated fused-ReLU layer: it masks for itself",
           build_stale_then_chain, dict(x=_X, x2=_X2, l0=_L0, l1=_L1, l2=_L0, cm=_CM, ch=_CH), 1, modes=("accumulate",)),
     _case("retain-graph-twice", "one chain backpropagated twice with retain_graph, gradients summed: a hit in each pass",
           build_retain_twice, dict(x=_X, l0=_L0, l1=_L1, cm=_CM), 0, modes=("accumulate",))] +
    # 5. weight sharing: each application's fused ReLU masks for itself (the head on the sum does not mark).  Every mode: autograd's
    # accumulation, direct writes, and direct writes with the conv folds deferred to a zero-lr step() of either optimizer
    [_case("siamese-linear", "one nets.Linear (fused ReLU) on two inputs, a head on the sum", build_siamese_linear,
           dict(x=_X, x2=_X2, ls=_L0, lh=_L1, cm=_CM), 2, optimizer=True, modes=ALL),
     _case("siamese-noisy", "one NoisyLinear (fused ReLU) on two inputs, a head on the sum", build_siamese_noisy,
           dict(x=_X, x2=_X2, ns=("noisy", NH, NK), lh=_L1, cm=_CM), 2, optimizer=True, modes=ALL),
     # (per application: fc4 masks for itself, the three conv layers receive hits)
     _case("siamese-body", "one NatureConvBody on two batches of 2 frames, a head on the sum", build_siamese_body,
           _body_spec(2, x2=_frames(2)), 2, kind="random", storage="koc", modes=ALL)] +
    # 6. a backward pass that does not reach every parameter its optimizer covers
    [_case("partial-covers", "the optimizer covers a Linear the backward never reaches", build_partial,
           dict(x=_X, l0=_L0, l1=_L1, lu=_L1, cm=_CM), 0, optimizer=True)]
)
_BY_NAME = {c["name"]: c for c in CASES}
assert len(_BY_NAME) == len(CASES), "case names must be unique"
SHARED = {"siamese-linear": ("ls",), "siamese-noisy": ("ns",), "siamese-body": ("body",)}      # the modules applied twice
UNREACHED = {"partial-covers": ("lu",)}


def by_name(name):
    return _BY_NAME[name]


def ids(cases=CASES):
    return [c["name"] for c in cases]


# ---------------------------------------------------------------------------------------------------------- operands
def _rs(*key):
    return np.random.RandomState(zlib.crc32(("/".join(str(k) for k in key)).encode()) & 0x7FFFFFFF)


def _ints(rs, shape, lo=-4, hi=4):
    return rs.randint(lo, hi + 1, size=shape).astype(F)


@functools.lru_cache(maxsize=None)
def operands(name):
    """-> {operand name: float32 / uint8 / int64 array}; a layer p contributes p.w, p.b (noisy: p.wmu, p.wsig, p.bmu, p.bsig, p.ein,
    p.eout, p.eb; the body: body.conv1.w .. body.fc4.b; the actor-critic net: ac.body.w/b, ac.actor.w/b, ac.critic.w/b)."""
    c = by_name(name)
    rs = _rs("autograd-graphs", name)
    integer = c["kind"] == "integer"
    out = {}

    def lin(p, o, k):
        out[p + ".w"] = _ints(rs, (o, k)) if integer else (rs.standard_normal((o, k)) / np.sqrt(k)).astype(F)
        out[p + ".b"] = _ints(rs, (o,)) if integer else (rs.standard_normal(o) * 0.1).astype(F)

    for key, s in c["spec"].items():
        if s[0] in ("input", "const"):
            out[key] = _ints(rs, s[1]) if integer else rs.standard_normal(s[1]).astype(F)
        elif s[0] == "lin":
            lin(key, s[1], s[2])
        elif s[0] == "noisy":
            o, k = s[1], s[2]
            assert integer, "noisy layers are drawn for the integer set only"
            out[key + ".wmu"], out[key + ".wsig"] = _ints(rs, (o, k), -2, 2), _ints(rs, (o, k), -1, 1)
            out[key + ".bmu"], out[key + ".bsig"] = _ints(rs, (o,), -2, 2), _ints(rs, (o,), -1, 1)
            for e, n in ((".ein", k), (".eout", o), (".eb", o)):
                out[key + e] = rs.choice(NOISE_INTS, size=n).astype(F)
        elif s[0] == "body":
            for layer in (1, 2, 3):
                out["%s.conv%d.w" % (key, layer)], out["%s.conv%d.b" % (key, layer)] = CE.draw_weights(rs, layer, "random")
            lin(key + ".fc4", 512, 3136)
        elif s[0] == "frames":
            out[key] = CE.draw_input(rs, 1, s[1], "random")[0]
        elif s[0] == "ac":
            lin(key + ".body", s[2], s[1]), lin(key + ".actor", s[3], s[2]), lin(key + ".critic", 1, s[2])
        elif s[0] == "action":
            out[key] = rs.randint(0, s[2], size=s[1]).astype(np.int64)
        else:
            raise KeyError(s)
    return out


def param_names(name):
    """The operand names that are parameters (gradients are compared for each of them and for every input)."""
    c = by_name(name)
    out = []
    for key, s in c["spec"].items():
        if s[0] == "lin":
            out += [key + ".w", key + ".b"]
        elif s[0] == "noisy":
            out += [key + e for e in (".wmu", ".wsig", ".bmu", ".bsig")]
        elif s[0] == "body":
            out += ["%s.%s.%s" % (key, l, t) for l in ("conv1", "conv2", "conv3", "fc4") for t in ("w", "b")]
        elif s[0] == "ac":
            out += ["%s.%s.%s" % (key, l, t) for l in ("body", "actor", "critic") for t in ("w", "b")]
    return out


def input_names(name):
    return [k for k, s in by_name(name)["spec"].items() if s[0] == "input"]


# -------------------------------------------------------------------------------------------------------- reference
def noise_f(e):
    return e.sign() * e.abs().sqrt()


class RefBackend:
    """The graph in plain torch ops on the float32 operand values, in `dtype`.  gates: {relu key: 0 / 1 array} replaces each
    fused ReLU by a multiplication with the given gate (the device's); absolute: every operand by its absolute value and every
    gate by 1 -- each tensor and gradient of that run bounds the partial sums of the real one (see int_bound)."""

    def __init__(self, name, dtype=None, gates=None, absolute=False):
        import torch
        self.torch = torch
        self.ops = operands(name)
        self.dtype = dtype or torch.float64
        self.gates, self.absolute = gates, absolute
        self.leaves, self.relu_out, self.relu_node, self.marking_nodes, self.count = {}, {}, {}, [], {}
        self.peak = 0.0

    # leaves
    def _leaf(self, key, grad):
        if key not in self.leaves:
            a = self.ops[key]
            a = np.abs(a) if self.absolute else a
            self.leaves[key] = self.torch.tensor(a.astype(D), dtype=self.dtype, requires_grad=grad)
        return self.leaves[key]

    def input(self, key):
        return self._leaf(key, True)

    def const(self, key):
        return self._leaf(key, False)

    def action(self, key):
        return self.torch.tensor(self.ops[key])

    def frames(self, key):
        if key not in self.leaves:
            self.leaves[key] = self.torch.tensor(CE.normalize(self.ops[key], 1.0 / 255).astype(D), dtype=self.dtype)
        return self.leaves[key]

    def touch(self, p):
        self._leaf(p + ".w", True), self._leaf(p + ".b", True)

    def _watch(self, t):
        if self.absolute:
            self.peak = max(self.peak, float(t.detach().abs().max()))
            if t.requires_grad:
                t.register_hook(lambda g: setattr(self, "peak", max(self.peak, float(g.abs().max()))))
        return t

    # layers
    def _key(self, p):
        n = self.count.get(p, 0)
        self.count[p] = n + 1
        return "%s#%d" % (p, n)

    def _relu(self, pre, p):
        key = self._key(p)
        if self.absolute:
            y = pre * 1.0
        elif self.gates is not None:
            y = pre * self.torch.tensor(np.asarray(self.gates[key], dtype=D), dtype=self.dtype)
        else:
            y = self.torch.relu(pre)
        self.relu_out[key], self.relu_node[key] = y, y.grad_fn
        return self._watch(y)

    def _mark(self, y, x_relu):
        if x_relu:
            self.marking_nodes.append(y.grad_fn)
        return y

    def _affine(self, x, w, b, p, act, x_relu):
        pre = self._mark(self._watch(self.torch.nn.functional.linear(x, w, b)), x_relu)
        return self._relu(pre, p) if act == "relu" else pre

    def linear(self, p, x, act=None, x_relu=False):
        return self._affine(x, self._leaf(p + ".w", True), self._leaf(p + ".b", True), p, act, x_relu)

    def module_linear(self, p, x):
        return self.linear(p, x, "relu" if p != "head" else None, False)

    def noisy(self, p, x, act=None, x_relu=False):
        wmu, wsig, bmu, bsig = [self._leaf(p + e, True) for e in (".wmu", ".wsig", ".bmu", ".bsig")]
        fi, fo, fb = [noise_f(self._leaf(p + e, False)) for e in (".ein", ".eout", ".eb")]
        return self._affine(x, wmu + wsig * self.torch.outer(fo, fi), bmu + bsig * fb, p, act, x_relu)

    def torch_relu(self, x):
        return self._watch(x * 1.0 if self.absolute else self.torch.relu(x))

    def conv(self, k, x):
        p = "body.conv%d" % k
        pre = self.torch.nn.functional.conv2d(x, self._leaf(p + ".w", True), self._leaf(p + ".b", True), stride=CE.GEOM[k][4])
        return self._relu(self._mark(pre, k > 1), p)

    def fc4(self, y3):
        return self._affine(y3.reshape(y3.shape[0], -1), self._leaf("body.fc4.w", True), self._leaf("body.fc4.b", True), "body.fc4", "relu", True)

    def body(self, x):
        return self.fc4(self.conv(3, self.conv(2, self.conv(1, x))))

    def actor_critic(self, x, action, tap, tap_first):
        t = self.torch
        phi = self.linear("ac.body", x, "relu")
        if tap is not None and tap_first:
            tap(phi)
        logits = self._mark(t.nn.functional.linear(phi, self._leaf("ac.actor.w", True), self._leaf("ac.actor.b", True)), True)
        v = t.nn.functional.linear(phi, self._leaf("ac.critic.w", True), self._leaf("ac.critic.b", True)).squeeze(-1)
        self.marking_nodes.append(v.grad_fn.next_functions[0][0])
        if tap is not None and not tap_first:
            tap(phi)
        logp = t.log_softmax(logits, dim=-1)
        return logp.gather(1, action.view(-1, 1)).squeeze(-1), -(logp.exp() * logp).sum(-1), v

    # results
    def run(self, build, order):
        self.losses = build(self, order)
        for loss, retain in self.losses:
            loss.backward(retain_graph=retain)
        return self

    def grads(self):
        """{operand name: gradient} of every parameter and input the graph holds (zeros where the backward never reached it)."""
        out = {}
        for k, t in self.leaves.items():
            if t.requires_grad:
                out[k] = (self.torch.zeros_like(t) if t.grad is None else t.grad).detach().numpy().astype(D)
        return out

    def forwards(self):
        return {k: y.detach().numpy().astype(D) for k, y in self.relu_out.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference with its OWN gates: (gradients, fused-ReLU outputs).  What the integer graphs are held to; for the
    random graphs the GPU test calls reference_with_gates with the device's gates instead."""
    c = by_name(name)
    r = RefBackend(name).run(c["build"], c["order"])
    return r.grads(), r.forwards()


def reference_with_gates(name, gates, dtype=None):
    c = by_name(name)
    r = RefBackend(name, dtype=dtype, gates=gates).run(c["build"], c["order"])
    return r.grads(), r.forwards()


def int_bound(name):
    """Largest |value| any partial sum of the integer graph can reach in any summation order: the graph run on the operands'
    absolute values with every gate open -- all terms non-negative, so each output element and each gradient element of that run
    is the sum of the absolute values of the terms of the real one.  Must stay below 2^24."""
    c = by_name(name)
    assert c["kind"] == "integer"
    r = RefBackend(name, absolute=True).run(c["build"], c["order"])
    return max([r.peak] + [float(np.abs(g).max()) for g in r.grads().values()])


# ------------------------------------------------------------------------------------------------------ graph shape
def graph_nodes(losses):
    seen, stack = {}, [l.grad_fn for l, _ in losses]
    while stack:
        n = stack.pop()
        if n is None or id(n) in seen:
            continue
        seen[id(n)] = n
        stack += [m for m, _ in n.next_functions]
    return list(seen.values())


def consumers(ref, key):
    """Nodes of the reference graph that take the fused-ReLU output `key` as an input."""
    target = ref.relu_node[key]
    return [n for n in graph_nodes(ref.losses) if any(m is target for m, _ in n.next_functions)]
