"""The autograd layer's graph protocols on the device: every graph of tests/autograd_graph_cases.py on the product layers
(nets.linear, nets.Linear, nets.NoisyLinear, nets.NatureConvBody in KOC and OIHW storage, nets.CategoricalActorCriticNet), in
every mode the table gives it -- autograd's accumulation, direct_param_grads(True), and for the shared conv body the deferred
folds followed by a zero-lr optimizer step -- against the float64 reference of the same graph.

Per case and mode:
  parity        integer graphs: forward and every gradient equal the int64 result; random graphs: max |got - want64| <= 1e-5 of
                max |want64| per tensor, no element exempted, the reference's ReLU gates taken from the device's forward output and
                the forward compared on its own; the worst error / bar of the case goes to the parity log
  launches      ops.act_bwd is counted through a pass-through wrapper: the count equals the table's (a hit where the table says
                the mask is handed down, a mask where the gradient was accumulated)
  determinism   a second run on fresh modules is bit-identical
  bounds        direct-mode .grad slots of free parameters sit in NaN-slacked buffers: the slack is untouched
  modes         direct writes equal autograd's accumulation value for value (same kernels); after a deferred backward, step() with
                lr = 0 leaves the parameters alone and .grad holds the sum over both applications; all_direct is False after a
                backward that shared or missed a parameter, and the next zero_grad(direct=True) fills

Each case is a handful of launches at batch <= 3 (or dims <= 48)."""
import copy

import numpy as np
import pytest
import torch

import autograd_graph_cases as G
from parity_log import record_parity

pytestmark = pytest.mark.gpu

SLACK = 64
NAN_BITS = np.float32("nan").view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    from deeprl_amd.support import select_device, Config
    select_device(0)
    return Config.DEVICE


class _Slot:
    """A .grad slot of n zeros with NaN slack on both sides."""

    def __init__(self, shape, dev):
        n = int(np.prod(shape))
        self.whole = torch.full((2 * SLACK + n,), float("nan"), dtype=torch.float32, device=dev)
        self.v = self.whole[SLACK:SLACK + n]
        self.v.zero_()
        self.n = n

    def slack_untouched(self, what):
        w = self.whole.detach().cpu().numpy()
        out = np.concatenate([w[:SLACK], w[SLACK + self.n:]])
        assert np.all(out.view(np.uint32) == NAN_BITS), what + ": written outside its .grad slot"


_BODY_TEMPLATE = []


def _new_body():
    """A NatureConvBody on the CPU (one orthogonal initialisation per session; every use overwrites the values)."""
    from deeprl_amd import nets
    if not _BODY_TEMPLATE:
        _BODY_TEMPLATE.append(nets.NatureConvBody())
    return copy.deepcopy(_BODY_TEMPLATE[0])


class DeviceBackend:
    """The graph on the product layers.  Parameters are torch.nn.Parameters holding the operand values; `mode` decides where
    their gradients go."""

    def __init__(self, c, dev, mode):
        from deeprl_amd import nets, optim
        self.c, self.dev, self.mode, self.nets = c, dev, mode, nets
        self.ops = G.operands(c["name"])
        self.leaves, self.params, self.modules, self.count, self.fwd, self.slots = {}, {}, {}, {}, {}, {}
        self.opt = None
        for key, s in c["spec"].items():
            if s[0] == "lin" and key != "head" and key not in ("ls",):
                for t in (".w", ".b"):
                    self.params[key + t] = torch.nn.Parameter(self._up(key + t))
            elif s[0] == "lin":          # a nets.Linear module: the shared layer (fused ReLU) or the plain head of the body
                m = nets.Linear(s[2], s[1])
                m.fused_act = "relu" if key == "ls" else None
                self._load(m, {"weight": key + ".w", "bias": key + ".b"}, key)
            elif s[0] == "noisy":
                m = nets.NoisyLinear(s[2], s[1])
                self._load(m, {"weight_mu": key + ".wmu", "weight_sigma": key + ".wsig", "bias_mu": key + ".bmu", "bias_sigma": key + ".bsig"}, key)
                with torch.no_grad():
                    for buf, e in (("noise_in", ".ein"), ("noise_out_weight", ".eout"), ("noise_out_bias", ".eb")):
                        getattr(m, buf).copy_(self._up(key + e))
                m.noise_changed()
                m.train()
            elif s[0] == "body":
                m = _new_body()
                names = {}
                for l in ("conv1", "conv2", "conv3", "fc4"):
                    names[l + ".weight"], names[l + ".bias"] = "%s.%s.w" % (key, l), "%s.%s.b" % (key, l)
                self._load(m, names, key)
                for l in ("conv1", "conv2", "conv3", "fc4"):
                    getattr(m, l).register_forward_hook(self._hook("body." + l))
            elif s[0] == "ac":
                m = nets.CategoricalActorCriticNet(s[1], s[3], nets.FCBody(s[1], (s[2],)))
                self._load(m, {"phi_body.layers.0.weight": key + ".body.w", "phi_body.layers.0.bias": key + ".body.b",
                               "fc_action.weight": key + ".actor.w", "fc_action.bias": key + ".actor.b",
                               "fc_critic.weight": key + ".critic.w", "fc_critic.bias": key + ".critic.b"}, key)
        if c["optimizer"]:
            kind = torch.optim.Adam if mode.endswith("adam") else torch.optim.RMSprop
            self.opt = optim.FusedOptimizer.adopt(kind(list(self.params.values()), lr=0.0))
            self.before = self.opt.flat.flat.detach().clone()
        elif mode == "direct":
            for key, p in self.params.items():
                self.slots[key] = _Slot(p.shape, dev)
                p.grad = self.slots[key].v.view(p.shape)

    def _up(self, key):
        return torch.from_numpy(np.ascontiguousarray(self.ops[key])).to(self.dev)

    def _load(self, module, names, key):
        module.to(self.dev)
        named = dict(module.named_parameters())
        assert set(named) == set(names), (sorted(named), sorted(names))
        with torch.no_grad():
            for pname, op in names.items():
                named[pname].copy_(self._up(op))
                self.params[op] = named[pname]
        self.modules[key] = module

    def _hook(self, p):
        def hook(mod, inp, out):
            self._seen(p, out)
        return hook

    def _seen(self, p, y):
        n = self.count.get(p, 0)
        self.count[p] = n + 1
        self.fwd["%s#%d" % (p, n)] = y
        return y

    # leaves
    def input(self, key):
        if key not in self.leaves:
            self.leaves[key] = self._up(key).requires_grad_(True)
        return self.leaves[key]

    def const(self, key):
        return self._up(key)

    def action(self, key):
        return self._up(key)

    def frames(self, key):
        """uint8 frames through ImageNormalizer: the KOC body takes them raw with the normaliser's coefficient on conv1 (what the
        device-resident agents do), the OIHW body takes the normaliser's float32 output (the drop-in path)."""
        from deeprl_amd.normalizers import ImageNormalizer
        norm = ImageNormalizer()
        x = self._up(key)
        if self.c["storage"] == "koc":
            self.modules["body"].conv1.u8_coef = float(norm.coef)
            return x
        return norm(x)

    def touch(self, p):
        pass

    # layers
    def linear(self, p, x, act=None, x_relu=False):
        y = self.nets.linear(x, self.params[p + ".w"], self.params[p + ".b"], act, x_relu)
        return self._seen(p, y) if act == "relu" else y

    def module_linear(self, p, x):
        y = self.modules[p](x)
        return self._seen(p, y) if self.modules[p].fused_act == "relu" else y

    def noisy(self, p, x, act=None, x_relu=False):
        m = self.modules[p]
        m.fused_act, m.masks_input_relu = act, bool(x_relu)
        y = m(x)
        return self._seen(p, y) if act == "relu" else y

    def torch_relu(self, x):
        return torch.relu(x)

    def conv(self, k, x):
        return getattr(self.modules["body"], "conv%d" % k)(x)

    def fc4(self, y3):
        return self.modules["body"].fc4(y3.view(y3.size(0), -1))

    def body(self, x):
        return self.modules["body"](x)

    def actor_critic(self, x, action, tap, tap_first):
        net = self.modules["ac"]
        phis = []

        def hook(mod, inp, out):
            self._seen("ac.body", out)
            phis.append(out)
            if tap is not None and tap_first:
                tap(out)
        h = net.phi_body.register_forward_hook(hook)
        try:
            out = net(x, action)
        finally:
            h.remove()
        if tap is not None and not tap_first:
            tap(phis[0])
        return out["log_pi_a"].squeeze(-1), out["entropy"].squeeze(-1), out["v"].squeeze(-1)

    # one run
    def run(self):
        from deeprl_amd import nets, ops
        c, mode = self.c, self.mode
        launches = []
        real = ops.act_bwd

        def counted(dy, y, act):
            launches.append(act)
            return real(dy, y, act)
        ops.act_bwd = counted
        try:
            if self.opt is not None:
                self.opt.zero_grad(direct=mode != "accumulate")
            losses = c["build"](self, c["order"])
            for loss, retain in losses:
                if mode == "accumulate":
                    ctx = nets.direct_param_grads(False)
                elif mode == "direct":
                    ctx = nets.direct_param_grads(True, covers=[self.opt] if self.opt is not None else ())
                else:
                    ctx = nets.direct_param_grads(True, defer_folds_to=self.opt, covers=[self.opt])
                with ctx:
                    loss.backward(retain_graph=retain)
            self.pending = len(self.opt._pending_folds) if self.opt is not None else 0
            if mode.startswith("deferred"):
                self.opt.step()          # lr = 0: folds what is still registered, moves nothing
        finally:
            ops.act_bwd = real
        torch.cuda.synchronize()
        for key, s in self.slots.items():
            assert self.params[key].grad.data_ptr() == s.v.data_ptr(), key + ": the .grad slot was replaced"
            s.slack_untouched("%s %s" % (c["name"], key))
        grads = {}
        for key, t in list(self.params.items()) + list(self.leaves.items()):
            g = torch.zeros_like(t) if t.grad is None else t.grad
            grads[key] = g.detach().cpu().numpy().copy()
        fwd = {k: y.detach().cpu().numpy().copy() for k, y in self.fwd.items()}
        return grads, fwd, len(launches)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _compare(c, mode, got, want, exact, figs, fails):
    assert set(want) <= set(got), sorted(set(want) - set(got))
    for key, w in want.items():
        g = got[key].astype(np.float64).reshape(w.shape)
        if not np.all(np.isfinite(g)):
            fails.append("%s %s: non-finite" % (mode, key))
            continue
        if exact:
            bad = g != w
            if bad.any():
                i = tuple(np.argwhere(bad)[0])
                fails.append("%s %s: %d of %d elements differ from the int64 result, first at %s: got %r want %r" % (
                    mode, key, int(bad.sum()), bad.size, i, g[i], w[i]))
            continue
        scale, err = float(np.abs(w).max()), float(np.abs(g - w).max())
        fig = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
        print("autograd graphs %s %s %s: err/scale %.3g (bar %.0e), scale %.3g" % (c["name"], mode, key, fig, G.BAR, scale))
        figs[key] = max(figs.get(key, 0.0), fig)
        if not fig <= G.BAR:
            fails.append("%s %s: max abs err %.3e vs scale %.3e (%.2e of it, bar %.0e)" % (mode, key, err, scale, fig, G.BAR))


def _cases_modes():
    return [(c, m) for c in G.CASES for m in c["modes"]]


_ACCUMULATED = {}      # case name -> the accumulate mode's gradients (what the direct mode is held to, bit for bit)


@pytest.mark.parametrize("c,mode", _cases_modes(), ids=["%s-%s" % (c["name"], m) for c, m in _cases_modes()])
def test_autograd_graph(dev, c, mode):
    exact = c["kind"] == "integer"
    b = DeviceBackend(c, dev, mode)
    grads, fwd, launches = b.run()
    print("autograd graphs %s %s: %d act_bwd launches (table: %d), %d folds left to step()" % (c["name"], mode, launches, c["act_bwd"], b.pending))
    if exact:
        want_g, want_f = G.reference(c["name"])
    else:
        want_g, want_f = G.reference_with_gates(c["name"], {k: (y > 0) for k, y in fwd.items()})
    figs, fails = {}, []
    assert set(fwd) == set(want_f), (sorted(fwd), sorted(want_f))
    _compare(c, mode, fwd, want_f, exact, figs, fails)
    _compare(c, mode, grads, want_g, exact, figs, fails)
    record_parity("autograd graphs %s %s" % (c["name"], mode), worst_err_over_bar=max(figs.values()) / G.BAR if figs else 0.0,
                  act_bwd_launches=launches, act_bwd_expected=c["act_bwd"],
                  **{k.replace(".", "_") + "_err_over_scale": v for k, v in figs.items()})
    assert not fails, "%s: %s" % (c["name"], "; ".join(fails))
    assert launches == c["act_bwd"], "%s %s: %d act_bwd launches, the graph calls for %d" % (c["name"], mode, launches, c["act_bwd"])
    # determinism: fresh modules, same bits
    grads2, fwd2, launches2 = DeviceBackend(c, dev, mode).run()
    assert launches2 == launches
    for got, again in ((grads, grads2), (fwd, fwd2)):
        for key in got:
            assert np.array_equal(_bits(got[key]), _bits(again[key])), "%s %s: second run differs in %s" % (c["name"], mode, key)
    # direct writes against autograd's accumulation: the same kernels, the same bits
    if mode == "accumulate":
        _ACCUMULATED[c["name"]] = grads
    elif mode == "direct" and c["name"] in _ACCUMULATED:
        for key, a in _ACCUMULATED[c["name"]].items():
            # (values: 0 + -0.0 is +0.0 where the accumulation starts from a zero fill)
            assert np.array_equal(a, grads[key]), "%s: %s written in place differs from autograd's accumulation" % (c["name"], key)
    # the optimizer's book-keeping
    if b.opt is not None and mode != "accumulate":
        shared_or_missed = c["name"] in G.SHARED or c["name"] in G.UNREACHED
        # (the OIHW head / free parameters of an adopted flat buffer are written directly; a plain chain overwrites everything)
        assert b.opt.all_direct is (not shared_or_missed), "%s %s: all_direct is %r" % (c["name"], mode, b.opt.all_direct)
        for p in G.UNREACHED.get(c["name"], ()):
            assert not grads[p + ".w"].any() and not grads[p + ".b"].any(), p + ": the unreached .grad left its zero fill"
        if shared_or_missed:
            b.opt.flat.grad.fill_(1.0)
            b.opt.zero_grad(direct=True)
            assert not bool(b.opt.flat.grad.any()), "zero_grad(direct=True) skipped its fill after a shared / partial backward"
    if mode.startswith("deferred"):
        # torch accepts lr = 0 for RMSprop and Adam alike, and so do the step kernels: nothing moves, nothing turns NaN
        assert b.opt.hyper["lr"] == 0.0 and b.opt.steps == 1
        assert torch.equal(b.opt.flat.flat, b.before), "a zero-lr step moved the parameters"
        assert not b.opt._pending_folds


def test_deferred_chain_still_folds_in_one_launch(dev):
    """The single-use graph of the agents keeps its one-launch fold: a KOC chain under defer_folds_to registers all three conv
    layers and folds none of them before step()."""
    c = G.by_name("chain-koc-b3")
    b = DeviceBackend(c, dev, "deferred-rmsprop")
    grads, fwd, launches = b.run()
    assert b.pending == 3 and launches == c["act_bwd"] and b.opt.all_direct is True
    want_g, _ = G.reference_with_gates(c["name"], {k: (y > 0) for k, y in fwd.items()})
    figs, fails = {}, []
    _compare(c, "deferred-rmsprop", grads, want_g, False, figs, fails)
    record_parity("autograd graphs chain-koc-b3 deferred-rmsprop", worst_err_over_bar=max(figs.values()) / G.BAR)
    assert not fails, "; ".join(fails)
