"""Edge-shape cases and float64 references for the loss, scan and sampling kernels (csrc/losses.hip, csrc/scan.hip,
dra_soft_update / dra_copy_f32 of csrc/optim.hip).  NOT a test file: pure numpy / torch on the CPU, imported by
tests/test_loss_edge_cases_host.py (which proves on the CPU that these inputs can carry the bars) and by
tests/test_gpu_loss_edges.py (which holds the kernels to them).

Every case is a dict of float32 / int64 numpy inputs made by a seeded np.random.RandomState.  `want_*(case, dtype)` evaluates
the plain-torch oracle (oracle/loss_oracle.py, gradients by autograd) on copies of the SAME values in `dtype`: float64 is the
reference the kernels are compared with, float32 measures the noise floor of the inputs.  Every want carries `margins`: per
row, the gap between the two best candidates of each discrete choice the kernel makes.

Bars (none of them tuned to the kernels):
  BAR        1e-5  the project's fp32 bar: max |got - want64| <= BAR * max |want64| per output tensor
  SCORE_GAP  1e-5  a row whose decision margin on a score (greedy action value, Gumbel score, PPO ratio vs clip bound) is
                   below this may be exempted from exact agreement with the float64 decision
  CUM_GAP    1e-6  the same for an inverse-CDF boundary |cumsum(p) - u|
  EXEMPT_CAP 1 %   of a case's rows at most may be exempted; none in "exact" cases (inputs on small integers and dyadic
                   fractions, where float32 and float64 agree on every tie and boundary hit)."""
import numpy as np
import torch

from oracle import loss_oracle as L
from oracle.synth_oracle import mix64

BAR = 1e-5
SCORE_GAP = 1e-5
CUM_GAP = 1e-6
EXEMPT_CAP = 0.01

_F32, _F64 = torch.float32, torch.float64


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _np(x):
    return x.detach().double().numpy()


def _top2_gap(score):
    """Per row of a [B, K] array: best minus second best (inf for K == 1)."""
    score = np.asarray(score, dtype=np.float64)
    if score.shape[-1] < 2:
        return np.full(score.shape[0], np.inf)
    s = np.sort(score, axis=-1)
    return s[:, -1] - s[:, -2]


def _half_grid(rs, shape, lo, hi):
    """Multiples of 0.5 in [lo, hi]: exact in float32 and float64, and so are their small sums and differences."""
    return (rs.randint(int(2 * lo), int(2 * hi) + 1, size=shape) * 0.5).astype(np.float32)


def clamp_action(action, n_actions):
    """load_action() of losses.hip: an out-of-range record behaves as the nearest valid action."""
    return np.clip(np.asarray(action).astype(np.int64), 0, n_actions - 1)


def exempt_rows(margin, threshold, n_rows, exact, strict=None):
    """(rows that may disagree with the float64 decision, their number, the cap on it); `strict` rows are never exempt."""
    ex = np.asarray(margin) < threshold
    if strict is not None:
        ex &= ~np.asarray(strict)
    cap = 0 if exact else int(EXEMPT_CAP * n_rows)
    return ex, int(ex.sum()), cap


# ------------------------------------------------------------------------------------------------------------ td_loss
TD_BATCHES = (1, 63, 64, 65, 500, 1024)
TD_ACTIONS = (1, 2, 6, 18)
_PER_GRID = (None, (0.5, 0.0), (0.5, 0.4), (0.6, 1.0), (0.6, 0.4), (0.5, 1.0), (0.6, 0.0))


def _td_case(name, b, a, double_q, act_f32, per, seed, mask="rand", exact=False):
    rs = np.random.RandomState(seed)
    c = dict(name=name, B=b, A=a, exact=exact, act_f32=act_f32, per=per, gamma_n=0.99 ** 3, eps=0.01,
             q=rs.standard_normal((b, a)).astype(np.float32), qt=rs.standard_normal((b, a)).astype(np.float32),
             qo=rs.standard_normal((b, a)).astype(np.float32) if double_q else None,
             action=rs.randint(0, a, size=b).astype(np.int64), reward=rs.standard_normal(b).astype(np.float32),
             mask=(rs.rand(b) > 0.2).astype(np.float32) if mask == "rand" else np.zeros(b, np.float32))
    p = rs.rand(b).astype(np.float32) + np.float32(0.05)
    c["sp"] = (p / p.sum()).astype(np.float32)
    return c


def td_cases():
    out = []
    for i, b in enumerate(TD_BATCHES):
        for j, a in enumerate(TD_ACTIONS):
            per = _PER_GRID[(i * len(TD_ACTIONS) + j) % len(_PER_GRID)]
            out.append(_td_case("b%da%d%s%s%s" % (b, a, "dq" if (i + j) % 2 else "", "f" if (i + 2 * j) % 3 == 0 else "",
                                                  "" if per is None else "_per%g_%g" % per),
                                b, a, (i + j) % 2 == 1, (i + 2 * j) % 3 == 0, per, 1000 + 37 * i + j))
    out.append(_td_case("b500a6_mask0", 500, 6, False, False, (0.6, 0.4), 1901, mask="zero"))
    out.append(_td_case("b65a18dq_mask0", 65, 18, True, True, None, 1902, mask="zero"))
    for f in (False, True):   # action records -3 and A+5 must behave as 0 and A-1
        c = _td_case("b65a6dq_oob%s" % ("f" if f else ""), 65, 6, True, f, (0.5, 0.4), 1903)
        c["action"][[0, 7, 64]] = -3
        c["action"][[1, 8, 63]] = 6 + 5
        out.append(c)
    # exact: equal maxima at different positions of the online row, different target values under them
    rs = np.random.RandomState(1904)
    c = _td_case("b128a6dq_ties", 128, 6, True, False, None, 1904, exact=True)
    for k in ("q", "qt", "qo"):
        c[k] = _half_grid(rs, (128, 6), -3, 3)
    c["reward"], c["mask"], c["gamma_n"] = _half_grid(rs, 128, -2, 2), np.ones(128, np.float32), 1.0
    first, second = rs.randint(0, 3, size=128), rs.randint(3, 6, size=128)
    rows = np.arange(128)
    c["qo"][rows, first] = 4.0
    c["qo"][rows, second] = 4.0
    c["qt"][rows, second] = c["qt"][rows, first] + 1.5    # taking the LAST maximum moves delta by 1.5
    out.append(c)
    c2 = dict(c, name="b128a6_ties", qo=None)             # plain max: ties in the target row itself
    c2["qt"] = c["qo"].copy()
    out.append(c2)
    return out


def want_td(c, dtype=_F64, beta=None):
    a = clamp_action(c["action"], c["A"])
    q = _t(c["q"], dtype).requires_grad_(True)
    qo = None if c["qo"] is None else _t(c["qo"], dtype)
    delta = L.dqn_td_error(q, _t(c["qt"], dtype), torch.from_numpy(a), _t(c["reward"], dtype), _t(c["mask"], dtype),
                           c["gamma_n"], qo)
    out = {}
    lw = delta
    if c["per"] is not None:
        alpha, b = c["per"]
        prio, w, lw = L.per_priorities_and_weights(delta, _t(c["sp"], dtype), c["eps"], alpha, b if beta is None else beta)
        out["prio"], out["weights"] = _np(prio), _np(w)
    loss = L.dqn_reduce(lw)
    dq, = torch.autograd.grad(loss, q)
    out.update(loss=_np(loss), delta=_np(delta), dq=_np(dq), action=a)
    sel = c["qt"] if c["qo"] is None else c["qo"]
    out["margins"] = dict(greedy_gap=_top2_gap(sel))
    return out


# ----------------------------------------------------------------------------------------------------------- c51_loss
def _c51_case(name, b, a, n, double_q, weights, lscale, rscale, seed, v=10.0, exact=False):
    rs = np.random.RandomState(seed)
    c = dict(name=name, B=b, A=a, N=n, exact=exact, gamma_n=0.99, v_min=-v, v_max=v,
             atoms=np.linspace(-v, v, n).astype(np.float32),
             logits=(rs.standard_normal((b, a, n)) * lscale).astype(np.float32),
             logits_t=(rs.standard_normal((b, a, n)) * lscale).astype(np.float32),
             logits_o=(rs.standard_normal((b, a, n)) * lscale).astype(np.float32) if double_q else None,
             action=rs.randint(0, a, size=b).astype(np.int64), reward=(rs.standard_normal(b) * rscale).astype(np.float32),
             mask=(rs.rand(b) > 0.2).astype(np.float32),
             weights=(rs.rand(b) + 0.1).astype(np.float32) if weights else None)
    return c


_C51_GRID = (  # B, A, N, double-Q, weights, logits scale, rewards scale
    (1, 1, 2, False, False, 3, 10), (32, 3, 51, True, True, 3, 10), (32, 4, 64, False, True, 1, 10),
    (32, 5, 65, True, False, 3, 1), (32, 18, 128, False, False, 1, 10), (1, 4, 200, True, True, 3, 10),
    (32, 5, 256, True, True, 3, 10), (300, 3, 51, False, True, 1, 1), (300, 18, 2, True, False, 3, 10),
    (32, 1, 256, False, False, 3, 1), (1, 18, 65, True, True, 1, 1), (32, 4, 200, False, True, 3, 1),
    (300, 5, 64, True, True, 1, 10))


def c51_cases():
    out = [_c51_case("b%da%dn%d%s%s_l%dr%d" % (b, a, n, "dq" if dq else "", "w" if w else "", ls, rs_), b, a, n, dq, w, ls, rs_,
                     2000 + i) for i, (b, a, n, dq, w, ls, rs_) in enumerate(_C51_GRID)]
    # exact 1: the selector (online) rows of actions 1 and 3 are identical and greedy; their TARGET rows differ
    rs = np.random.RandomState(2901)
    c = _c51_case("b16a4n17dq_ties", 16, 4, 17, True, False, 1, 1, 2901, v=8.0, exact=True)
    for k in ("logits", "logits_t", "logits_o"):
        c[k] = _half_grid(rs, (16, 4, 17), -2, 2)
    c["logits_o"][:, :, 6:] -= 8.0                        # actions 0 and 2: mass on the low atoms
    c["logits_o"][:, 1, :] = c["logits_o"][:, 0, ::-1]    # action 1: mass on the high atoms
    c["logits_o"][:, 3, :] = c["logits_o"][:, 1, :]       # action 3: the same row again
    c["reward"], c["mask"], c["gamma_n"] = rs.randint(-2, 3, size=16).astype(np.float32), np.ones(16, np.float32), 1.0
    out.append(c)
    # exact 2: mask 1, gamma^n 1, integer rewards, atoms -8..8 at spacing 1: every target lands on an atom
    c = _c51_case("b32a3n17_on_atom", 32, 3, 17, False, True, 1, 1, 2902, v=8.0, exact=True)
    for k in ("logits", "logits_t"):
        c[k] = _half_grid(rs, (32, 3, 17), -2, 2)
    c["reward"], c["mask"], c["gamma_n"] = rs.randint(-5, 6, size=32).astype(np.float32), np.ones(32, np.float32), 1.0
    out.append(c)
    # exact 3: terminal samples with reward +-100: all mass clamped onto the end atoms
    c = _c51_case("b32a3n17_clamped", 32, 3, 17, False, False, 1, 1, 2903, v=8.0, exact=True)
    for k in ("logits", "logits_t"):
        c[k] = _half_grid(rs, (32, 3, 17), -2, 2)
    c["reward"] = np.where(rs.rand(32) < 0.5, -100.0, 100.0).astype(np.float32)
    c["mask"], c["gamma_n"] = np.zeros(32, np.float32), 1.0
    out.append(c)
    return out


def want_c51(c, dtype=_F64):
    a = clamp_action(c["action"], c["A"])
    atoms = _t(c["atoms"], dtype)
    x = _t(c["logits"], dtype).requires_grad_(True)
    pt = torch.softmax(_t(c["logits_t"], dtype), dim=-1)
    po = None if c["logits_o"] is None else torch.softmax(_t(c["logits_o"], dtype), dim=-1)
    r, m = _t(c["reward"], dtype), _t(c["mask"], dtype)
    kl = L.c51_kl(torch.log_softmax(x, dim=-1), pt, torch.from_numpy(a), r, m, c["gamma_n"], atoms, c["v_min"], c["v_max"], po)
    loss = kl.mean() if c["weights"] is None else (kl * _t(c["weights"], dtype)).mean()
    dl, = torch.autograd.grad(loss, x)
    sel = pt if po is None else po
    qsel = (sel * atoms).sum(-1)
    # the projected target once more, for the boundary assertions of the exact cases
    a_next = torch.argmax(qsel, dim=-1)
    pn = pt[torch.arange(c["B"]), a_next]
    tz = (r.unsqueeze(-1) + c["gamma_n"] * m.unsqueeze(-1) * atoms.view(1, -1)).clamp(c["v_min"], c["v_max"])
    dz = (c["v_max"] - c["v_min"]) / float(c["N"] - 1)
    proj = ((1 - (tz.unsqueeze(1) - atoms.view(1, -1, 1)).abs() / dz).clamp(0, 1) * pn.unsqueeze(1)).sum(-1)
    return dict(kl=_np(kl), loss=_np(loss), dlogits=_np(dl), action=a, a_next=a_next.numpy(), tz=_np(tz), m=_np(proj),
                margins=dict(greedy_gap=_top2_gap(_np(qsel))))


# ------------------------------------------------------------------------------------------------------------ qr_loss
_QR_GRID = (  # B, A, N
    (1, 1, 1), (8, 4, 3), (9, 7, 4), (32, 4, 17), (32, 7, 200), (9, 1, 201), (8, 4, 1023), (1, 7, 1024), (32, 7, 4),
    (8, 1, 200), (9, 4, 1024))


def _qr_case(name, b, a, n, seed, exact=False):
    rs = np.random.RandomState(seed)
    return dict(name=name, B=b, A=a, N=n, exact=exact, gamma_n=0.99,
                theta=rs.standard_normal((b, a, n)).astype(np.float32), theta_t=rs.standard_normal((b, a, n)).astype(np.float32),
                action=rs.randint(0, a, size=b).astype(np.int64), reward=rs.standard_normal(b).astype(np.float32),
                mask=(rs.rand(b) > 0.2).astype(np.float32))


def qr_cases():
    out = [_qr_case("b%da%dn%d" % g, g[0], g[1], g[2], 3100 + i) for i, g in enumerate(_QR_GRID)]
    # exact 1: everything on a 0.5 grid, gamma^n = 1, mask = 1: d = 0 and |d| = 1 occur many times
    rs = np.random.RandomState(3901)
    c = _qr_case("b9a4n20_kink", 9, 4, 20, 3901, exact=True)
    c["theta"], c["theta_t"] = _half_grid(rs, (9, 4, 20), -2, 2), _half_grid(rs, (9, 4, 20), -2, 2)
    c["reward"], c["mask"], c["gamma_n"] = _half_grid(rs, 9, -1, 1), np.ones(9, np.float32), 1.0
    out.append(c)
    # exact 2: ties of the greedy action.  Rows 1 and 2 are identical, row 3 is row 1 reversed (the same sum exactly, other
    # quantiles under each index), row 0 is lower: the first maximum is row 1, the last is a DIFFERENT row.
    c = _qr_case("b9a4n16_ties", 9, 4, 16, 3902, exact=True)
    base = np.sort(_half_grid(rs, (9, 16), -2, 2), axis=-1) + (np.arange(16) * 0.5).astype(np.float32)
    c["theta_t"] = np.stack([base - 1.0, base, base, base[:, ::-1]], axis=1).astype(np.float32)
    c["theta"] = _half_grid(rs, (9, 4, 16), -2, 2)
    c["reward"], c["mask"], c["gamma_n"] = _half_grid(rs, 9, -1, 1), np.ones(9, np.float32), 1.0
    out.append(c)
    return out


def want_qr(c, dtype=_F64):
    a = clamp_action(c["action"], c["A"])
    th = _t(c["theta"], dtype).requires_grad_(True)
    tt, r, m = _t(c["theta_t"], dtype), _t(c["reward"], dtype), _t(c["mask"], dtype)
    lv = L.qr_loss(th, tt, torch.from_numpy(a), r, m, c["gamma_n"])
    loss = lv.mean()
    dth, = torch.autograd.grad(loss, th)
    sums = tt.sum(-1)
    a_next = torch.argmax(sums, dim=-1)
    rows = torch.arange(c["B"])
    tgt = r.unsqueeze(-1) + c["gamma_n"] * m.unsqueeze(-1) * tt[rows, a_next]
    d = _np(tgt.unsqueeze(-1) - th.detach()[rows, torch.from_numpy(a)].unsqueeze(1))    # [B, N_j, N_i]
    return dict(loss_vec=_np(lv), loss=_np(loss), dtheta=_np(dth), action=a, a_next=a_next.numpy(), d=d,
                margins=dict(greedy_gap=_top2_gap(_np(sums)), d_to_0=np.abs(d).reshape(c["B"], -1).min(-1),
                             d_to_1=np.abs(np.abs(d) - 1.0).reshape(c["B"], -1).min(-1)))


# ------------------------------------------------------------------------------------------------ ppo_loss / a2c_loss
ONPOLICY_M = (1, 64, 1024, 1025, 5000, 32768)


def _onpolicy_case(name, m, clip, seed, spread=0.3, exact=False):
    rs = np.random.RandomState(seed)
    lp = (-np.abs(rs.standard_normal(m)) - 0.1).astype(np.float32)
    return dict(name=name, M=m, clip=clip, exact=exact, ew=0.01, vw=0.5, lp=lp,
                old_lp=(lp + rs.standard_normal(m).astype(np.float32) * np.float32(spread)).astype(np.float32),
                ent=np.abs(rs.standard_normal(m)).astype(np.float32), v=rs.standard_normal(m).astype(np.float32),
                adv=rs.standard_normal(m).astype(np.float32), ret=rs.standard_normal(m).astype(np.float32))


def ppo_cases():
    grid = [(m, (0.1, 0.2)[i % 2]) for i, m in enumerate(ONPOLICY_M)] + [(1025, 0.1), (5000, 0.2)]
    out = [_onpolicy_case("m%d_clip%g" % (m, clip), m, clip, 4000 + i, spread=0.3 if i % 2 else 0.1)
           for i, (m, clip) in enumerate(grid)]
    c = _onpolicy_case("m5000_far_outside", 5000, 0.2, 4101)    # ratios e^-3 .. e^3 under both signs of the advantage
    c["old_lp"] = (c["lp"] - np.where(np.arange(5000) % 2 == 0, 3.0, -3.0).astype(np.float32)).astype(np.float32)
    out.append(c)
    c = _onpolicy_case("m1025_ratio1", 1025, 0.2, 4102, exact=True)
    c["old_lp"] = c["lp"].copy()
    out.append(c)
    c = _onpolicy_case("m1025_adv0", 1025, 0.1, 4103, exact=True)
    c["adv"] = np.zeros(1025, np.float32)
    out.append(c)
    c = _onpolicy_case("m64_ratio1_adv0", 64, 0.1, 4104, exact=True)
    c["old_lp"], c["adv"] = c["lp"].copy(), np.zeros(64, np.float32)
    out.append(c)
    return out


def a2c_cases():
    return [_onpolicy_case("m%d" % m, m, 0.0, 4500 + i) for i, m in enumerate(ONPOLICY_M)]


def want_ppo(c, dtype=_F64):
    lp, ent, v = [_t(c[k], dtype).requires_grad_(True) for k in ("lp", "ent", "v")]
    old, adv, ret = _t(c["old_lp"], dtype), _t(c["adv"], dtype), _t(c["ret"], dtype)
    pl, vl, kl = L.ppo_losses(lp, ent, v, old, adv, ret, c["clip"], c["ew"])
    g = torch.autograd.grad(pl + vl, [lp, ent, v])
    ratio = _np((lp - old).exp())
    return dict(out=np.array([pl.item(), vl.item(), kl.item()]), g_lp=_np(g[0]), g_ent=_np(g[1]), g_v=_np(g[2]), ratio=ratio,
                margins=dict(clip_gap=np.minimum(np.abs(ratio - (1.0 - c["clip"])), np.abs(ratio - (1.0 + c["clip"])))))


def want_a2c(c, dtype=_F64):
    lp, ent, v = [_t(c[k], dtype).requires_grad_(True) for k in ("lp", "ent", "v")]
    adv, ret = _t(c["adv"], dtype), _t(c["ret"], dtype)
    loss = L.a2c_loss(lp, ent, v, adv, ret, c["ew"], c["vw"])
    g = torch.autograd.grad(loss, [lp, ent, v])
    policy, value, entropy = -(lp * adv).mean(), 0.5 * (ret - v).pow(2).mean(), ent.mean()   # the parts the kernel also returns
    return dict(out=np.array([loss.item(), policy.item(), value.item(), entropy.item()]), g_lp=_np(g[0]), g_ent=_np(g[1]),
                g_v=_np(g[2]), margins={})


# ------------------------------------------------------------------------------------------- per_weights, weighted_mean
def per_cases():
    out = []
    for i, b in enumerate((1, 64, 65, 1024)):
        for alpha, beta in ((0.5, 0.4), (0.6, 1.0)):
            rs = np.random.RandomState(5000 + 10 * i + int(alpha * 10))
            p = rs.rand(b).astype(np.float32) + np.float32(0.05)
            out.append(dict(name="b%d_a%g_b%g" % (b, alpha, beta), B=b, alpha=alpha, beta=beta, eps=0.01, exact=False,
                            loss_vec=np.abs(rs.standard_normal(b)).astype(np.float32), sp=(p / p.sum()).astype(np.float32)))
    return out


def want_per(c, dtype=_F64):
    prio, w, _ = L.per_priorities_and_weights(_t(c["loss_vec"], dtype), _t(c["sp"], dtype), c["eps"], c["alpha"], c["beta"])
    return dict(prio=_np(prio), weights=_np(w), margins={})


def wmean_cases():
    out = []
    for i, n in enumerate((1, 1023, 1025, 100003)):
        rs = np.random.RandomState(5500 + i)     # loss-like (positive) values: the mean is not a cancellation
        out.append(dict(name="n%d" % n, n=n, exact=False, x=(np.abs(rs.standard_normal(n)) + 0.1).astype(np.float32),
                        w=(rs.rand(n) + 0.1).astype(np.float32)))
    return out


def want_wmean(c, weighted, dtype=_F64):
    x = _t(c["x"], dtype)
    return _np(((x * _t(c["w"], dtype)) if weighted else x).sum() / c["n"])


# -------------------------------------------------------------------------------------------------------- categorical
U_BELOW_ONE = np.float32(1.0 - 2.0 ** -24)
_CAT_GRID = ((1, 1), (1, 64), (256, 1), (256, 2), (257, 64), (5000, 2), (5000, 64), (257, 2))


def cat_cases():
    out = []
    for i, (b, a) in enumerate(_CAT_GRID):
        rs = np.random.RandomState(6000 + i)
        logits = (rs.standard_normal((b, a)) * 3).astype(np.float32)
        u = rs.rand(b).astype(np.float32)
        peaked, equal = np.zeros(b, bool), np.zeros(b, bool)
        if b >= 256:
            for k in range(4):      # rows 0..3: one logit 50 above the rest; rows 4..7: all equal
                logits[k] = (rs.standard_normal(a) * 0.5).astype(np.float32)
                logits[k, (k * 21) % a] += 50.0
                logits[4 + k] = np.float32(k - 1.5)
            peaked[:4], equal[4:8] = True, True
            u[[0, 8]], u[1], u[[2, 10]] = 0.0, U_BELOW_ONE, 1.0
            if b >= 5000:
                u[9] = U_BELOW_ONE
        else:
            u[0] = 1.0 if a == 1 else 0.0
        out.append(dict(name="b%da%d" % (b, a), B=b, A=a, exact=False, logits=logits, u=u, peaked=peaked, equal=equal,
                        action=rs.randint(0, a, size=b).astype(np.int64), g_lp=rs.standard_normal(b).astype(np.float32),
                        g_ent=rs.standard_normal(b).astype(np.float32)))
    return out


def categorical_ref(logits, action, g_lp, g_ent, dtype=_F64):
    """Categorical(logits): log-prob of `action`, entropy and d(g_lp . log_pi_a + g_ent . entropy) / d logits, written out
    (network_heads.py:249-254; the host test holds it against torch.distributions in float64)."""
    x = _t(logits, dtype)
    logp = x - torch.logsumexp(x, dim=-1, keepdim=True)
    p = logp.exp()
    ent = -(p * logp).sum(-1)
    a = torch.from_numpy(np.asarray(action, dtype=np.int64))
    onehot = torch.zeros_like(x).scatter_(1, a.unsqueeze(-1), 1.0)
    gl, ge = _t(g_lp, dtype).unsqueeze(-1), _t(g_ent, dtype).unsqueeze(-1)
    dl = gl * (onehot - p) - ge * p * (logp + ent.unsqueeze(-1))
    return dict(p=_np(p), logp=_np(logp), log_pi_a=_np(logp.gather(1, a.unsqueeze(-1)).squeeze(-1)), entropy=_np(ent),
                dlogits=_np(dl))


def inverse_cdf(p, u):
    """First a with float64 cumsum(p)[a] > u; the last action absorbs rounding, and u >= 1 always gives it.  Returns
    (action, margin): margin = the smallest |cum[a] - u| over the boundaries a < A - 1 that decide the draw."""
    p, u = np.asarray(p, dtype=np.float64), np.asarray(u, dtype=np.float64)
    b, a = p.shape
    if a == 1:
        return np.zeros(b, np.int64), np.full(b, np.inf)
    cum = np.cumsum(p, axis=1)
    over = cum[:, :a - 1] > u[:, None]
    act = np.where(over.any(axis=1), over.argmax(axis=1), a - 1)
    act = np.where(u >= 1.0, a - 1, act)
    margin = np.abs(cum[:, :a - 1] - u[:, None]).min(axis=1)
    return act.astype(np.int64), margin


def want_cat(c, dtype=_F64):
    w = categorical_ref(c["logits"], c["action"], c["g_lp"], c["g_ent"], dtype)
    act, margin = inverse_cdf(w["p"], c["u"])
    w.update(sampled=act, strict=c["u"] >= 1.0, margins=dict(cdf_gap=margin))
    return w


# ------------------------------------------------------------------------------------------------------ gumbel_sample
_GOLD = np.uint64(0x9E3779B97F4A7C15)
_GUMBEL_GRID = ((1, 1), (16, 4), (256, 18), (257, 64), (1000, 18), (1000, 4), (1, 64), (16, 1))


def gumbel_cases():
    out = []
    for i, (n, a) in enumerate(_GUMBEL_GRID):
        rs = np.random.RandomState(7000 + i)
        out.append(dict(name="n%da%d" % (n, a), n=n, A=a, exact=False, seed=int(rs.randint(1, 1 << 31)) * 2654435761 + i,
                        step=int(rs.randint(0, 100000)), lo=(0, 3, 64, 1000)[i % 4],
                        logits=(rs.standard_normal((n, a)) * 2).astype(np.float32)))
    return out


def gumbel_full_logits(c):
    """Logits of all lo + n global rows, the case's own rows last: the one-rank call of the rank-invariance check."""
    rs = np.random.RandomState(c["n"] + c["A"])
    return np.concatenate([(rs.standard_normal((c["lo"], c["A"])) * 2).astype(np.float32), c["logits"]], axis=0)


def gumbel_uniforms(seed, step, lo, n, n_actions):
    """The uniforms of gumbel_sample_kernel, float64 [n, A]: base = mix64(seed * GOLD + step); word (row, a) =
    mix64(base + (lo + row) * 64 + a); u = ((word >> 41) + 0.5) * 2^-23 -- 23 bits, exact in float32."""
    with np.errstate(over="ignore"):
        base = mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) * _GOLD + np.uint64(step))
        idx = (np.uint64(lo) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(64) + np.arange(n_actions, dtype=np.uint64)[None, :]
        h = mix64(base + idx)
    return ((h >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_ref(logits, seed, step, lo):
    """(action [n], top-two score gap [n], u [n, A]) with the scores logits - log(-log u) in float64."""
    logits = np.asarray(logits, dtype=np.float64)
    u = gumbel_uniforms(seed, step, lo, *logits.shape)
    score = logits - np.log(-np.log(u))
    return score.argmax(axis=1).astype(np.int64), _top2_gap(score), u


# ---------------------------------------------------------------------------------------------- gae, adv_normalize_
_GAE_GRID = (  # T, N, use_gae, (gamma, tau), masks
    (1, 1, True, (0.99, 0.95), "r01"), (1, 16, False, (0.99, 0.95), "r30"), (2, 3, True, (1.0, 1.0), "ones"),
    (63, 4, True, (0.99, 0.0), "r30"), (64, 5, True, (0.9, 1.0), "r01"), (65, 16, True, (0.99, 0.95), "r30"),
    (65, 3, False, (1.0, 1.0), "zeros"), (64, 4, True, (0.99, 0.95), "zeros"), (63, 5, False, (0.9, 1.0), "r30"),
    (64, 1, True, (1.0, 1.0), "r01"), (700, 5, True, (0.99, 0.95), "r01"), (700, 3, True, (1.0, 1.0), "r01"),
    (2048, 16, True, (0.99, 0.95), "r01"), (2048, 1, False, (0.99, 0.0), "r30"), (2048, 3, True, (1.0, 1.0), "ones"),
    (4096, 3, True, (0.99, 0.95), "r01"), (4096, 5, False, (1.0, 1.0), "r01"), (4096, 4, True, (0.9, 1.0), "ones"),
    (8192, 3, True, (0.99, 0.95), "r01"), (8192, 1, True, (0.99, 0.0), "zeros"), (8192, 5, True, (0.9, 1.0), "r30"),
    (12000, 3, True, (0.99, 0.95), "r01"), (12000, 1, False, (0.99, 0.95), "r30"))


def gae_cases():
    out = []
    for i, (t, n, use_gae, (gamma, tau), mk) in enumerate(_GAE_GRID):
        rs = np.random.RandomState(8000 + i)
        mask = {"r01": lambda: rs.rand(t, n, 1) > 0.01, "r30": lambda: rs.rand(t, n, 1) > 0.30,
                "ones": lambda: np.ones((t, n, 1)), "zeros": lambda: np.zeros((t, n, 1))}[mk]().astype(np.float32)
        out.append(dict(name="t%dn%d%s_g%gt%g_%s" % (t, n, "gae" if use_gae else "", gamma, tau, mk), T=t, N=n, use_gae=use_gae,
                        gamma=gamma, tau=tau, exact=False, reward=rs.standard_normal((t, n, 1)).astype(np.float32), mask=mask,
                        value=rs.standard_normal((t + 1, n, 1)).astype(np.float32)))
    return out


def want_gae(c, dtype=_F64):
    with torch.no_grad():
        adv, ret = L.gae_reverse(_t(c["reward"], dtype), _t(c["mask"], dtype), _t(c["value"], dtype), c["gamma"], c["tau"],
                                 c["use_gae"])
    return dict(adv=_np(adv), ret=_np(ret), margins={})


def advnorm_cases():
    out = []
    for i, n in enumerate((2, 1023, 1024, 1025, 32768, 100003)):
        rs = np.random.RandomState(8500 + i)
        out.append(dict(name="n%d" % n, n=n, exact=False, adv=(rs.standard_normal(n) * 2 + 0.5).astype(np.float32)))
    # mean 1000, std 1, twice.  The first is small and on a 2^-6 grid: every partial sum is exact in float32 in any order, so
    # the float32 oracle can carry it.  The second is what a PPO batch of un-centred returns looks like: one ulp of a float32
    # running sum of 32768 values near 1000 is 2 .. 4, so a float32 accumulation (the float32 oracle included) forms this
    # mean to 1e-5 of the result only by luck of the summation order; the kernel promises float64 accumulation and is held
    # to the float64 oracle all the same.
    # The sample is centred so that the mean is, within 1e-6, the float32 number 1000: the (float) rounding of the mean,
    # which the kernel performs after its float64 sums, then costs nothing.
    rs = np.random.RandomState(8599)
    grid = np.round(rs.standard_normal(128) * 64) / 64
    out.append(dict(name="n128_mean1000_std1_grid", n=128, exact=False, adv=(grid + 1000.0).astype(np.float32)))
    x = rs.standard_normal(32768)
    out.append(dict(name="n32768_mean1000_std1", n=32768, exact=False, needs_fp64_sums=True,
                    adv=(x - x.mean() + 1000.0).astype(np.float32)))
    return out


def advnorm_fp64_sums_fp32_apply(c):
    """What adv_normalize_kernel promises: mean and unbiased std accumulated in float64, rounded to float32, then
    (a - mean) / std in float32."""
    a = c["adv"]
    a64 = a.astype(np.float64)
    fm, fs = np.float32(a64.mean()), np.float32(a64.std(ddof=1))
    return ((a - fm) / fs).astype(np.float32)


def want_advnorm(c, dtype=_F64):
    return _np(L.normalize_advantage(_t(c["adv"], dtype)))


# ------------------------------------------------------------------------------------------- soft_update, copy_f32
FLAT_SIZES = (0, 1, 3, 4, 5, 1023, 1000003)
SOFT_MIXES = (0.001, 0.005, 1.0)
FLAT_PAD = 67     # elements behind n in the allocation, which must stay untouched


def flat_case(n, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n + FLAT_PAD).astype(np.float32), rs.standard_normal(n + FLAT_PAD).astype(np.float32)


def polyak_ref(target, src, mix):
    """target * keep + src * mix with keep = f32(1 - mix) and BOTH products rounded to float32 before the add (optim.hip;
    DDPG_agent.py:26-30): every step is one IEEE float32 operation, so numpy float32 gives the kernel's bits."""
    keep, mix = np.float32(1.0 - mix), np.float32(mix)
    a = (np.asarray(target, dtype=np.float32) * keep).astype(np.float32)
    b = (np.asarray(src, dtype=np.float32) * mix).astype(np.float32)
    return (a + b).astype(np.float32)
