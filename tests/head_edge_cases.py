"""Edge-shape cases and float64 references for the kernels of the n-step DQN, option-critic and Rainbow updates
(csrc/nstep_q.hip dra_nstep_q_loss_bwd, csrc/option_critic.hip dra_oc_loss_bwd, csrc/noisy.hip dra_noisy_linear_fwd / _bwd,
dra_dueling_atoms_fwd / _bwd, dra_per_weights_dev).  NOT a test file: pure numpy on the CPU, imported by
tests/test_head_edge_cases_host.py (which proves on the CPU that the inputs can carry the bar and that every case reaches the
path it is named for) and by tests/test_gpu_head_edges.py (which holds the kernels to them).

Every operation is stated twice: `*_ref` evaluates it in float64 from the float32 operands (scalar hyperparameters first
rounded to float32, as the kernels hold them; out-of-range indices clamped, as the kernels promise), `*_f32` is the float32
transcription of the kernel's own summation order (every operation rounded, no contraction: the library is built with
-ffp-contract=off): the noise floor of the inputs at that order (noisy_f32 says where it is an estimate instead).

Bar (not tuned to the kernels): BAR = 1e-5 of the reference's max-abs per output tensor, the project's fp32 bar; where float64
says a tensor is exactly zero, the kernel's must be exactly zero."""
import numpy as np

BAR = 1e-5
F = np.float32
D = np.float64


def _f(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _clamp(a, n):
    return np.clip(np.asarray(a, dtype=np.int64), 0, n - 1)


def _serial(x):
    """Sum over axis 0 in ascending index order, every partial sum rounded to float32 (one accumulator)."""
    x = np.asarray(x, dtype=np.float32)
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], dtype=np.float32)
    return np.cumsum(x, axis=0, dtype=np.float32)[-1]


NSTEP_SUM_SPANS = (8, 128)         # kNstepSumInner, kNstepSumOuter of csrc/nstep_q.hip


def _tree(x, spans=NSTEP_SUM_SPANS):
    """Sum over axis 0 as a fixed tree of three levels: every span of spans[0] consecutive entries in ascending order, those
    sums in ascending order within every span of spans[1] entries, then the spans of spans[1] in ascending order (entries a
    kernel skips are zeros here: adding +0 changes no sum).  At most 8 + 16 + 16 additions lie between a term and the sum of
    2048 of them."""
    x = np.asarray(x, dtype=np.float32)
    for span in (spans[0], spans[1] // spans[0]):
        n = -(-max(1, x.shape[0]) // span)
        pad = np.zeros((n * span,) + x.shape[1:], dtype=np.float32)
        pad[:x.shape[0]] = x
        x = np.stack([_serial(pad[i * span:(i + 1) * span]) for i in range(n)])
    return _serial(x)


def _returns(reward, mask, boot, gamma, dtype):
    """ret[t] = r[t] + (gamma m[t]) ret[t + 1] backwards from the bootstrap, in `dtype` (the kernels' operation order)."""
    reward, mask, ret = reward.astype(dtype), mask.astype(dtype), boot.astype(dtype)
    g = dtype(F(gamma))
    out = np.zeros(reward.shape, dtype=dtype)
    for t in reversed(range(reward.shape[0])):
        ret = reward[t] + (g * mask[t]) * ret
        out[t] = ret
    return out


def _features(rs, rows):
    """fc4's fused-ReLU output: half the entries exact +0, and -0 sprinkled over them."""
    phi = np.maximum(rs.standard_normal((rows, 512)), 0).astype(np.float32)
    neg = rs.rand(rows, 512) < 0.05
    phi[neg & (phi == 0)] = F(-0.0)
    return phi


def _mask_of(rs, shape, kind):
    if kind == "zeros":
        return np.zeros(shape, dtype=np.float32)
    if kind == "ones":
        return np.ones(shape, dtype=np.float32)
    return (rs.rand(*shape) > 0.25).astype(np.float32)


OUT_OF_RANGE = (-1, None, 2 ** 40)        # None: the count itself (the first index past the end)


def _sprinkle(rs, idx, n):
    """Every eleventh entry replaced by an out-of-range value whose clamp is the entry it replaces or the other end."""
    idx = idx.copy().reshape(-1)
    for i in range(0, idx.size, 11):
        bad = OUT_OF_RANGE[(i // 11) % 3]
        idx[i] = n if bad is None else bad
    return idx


# ================================================================================================ dra_nstep_q_loss_bwd
NSTEP_SHAPES = [(1, 1, 1), (1, 1, 64), (3, 1, 2), (1, 257, 4), (2, 300, 18), (8, 256, 4), (2048, 1, 3), (1, 2048, 64)]
# (shape, variant): every shape plain, and the variants where they bite
NSTEP_VARIANTS = [
    ((2, 300, 18), "unused-action"), ((1, 257, 4), "unused-action"), ((3, 1, 2), "unused-action"),
    ((8, 256, 4), "one-action"), ((2048, 1, 3), "one-action"), ((1, 2048, 64), "one-action"),
    ((3, 1, 2), "clamped"), ((2, 300, 18), "clamped"), ((1, 1, 64), "clamped"),
    ((8, 256, 4), "mask0"), ((8, 256, 4), "mask1"), ((8, 256, 4), "gamma0"), ((8, 256, 4), "gamma1"), ((2048, 1, 3), "mask1"),
]


def nstep_case(shape, variant="plain"):
    t_len, n, a = shape
    rows = t_len * n
    rs = np.random.RandomState(1000 + 7 * t_len + 3 * n + a + sum(map(ord, variant)))
    action = rs.randint(0, a, rows).astype(np.int64)
    unused = None
    if variant == "unused-action":
        unused = a - 1 if a > 2 else 0
        action[action == unused] = (unused + 1) % a
    if variant == "one-action":
        action[:] = a - 1
    if variant == "clamped":
        action = _sprinkle(rs, action, a)
    gamma = {"gamma0": 0.0, "gamma1": 1.0}.get(variant, 0.99)
    return dict(name="T%d-N%d-A%d-%s" % (t_len, n, a, variant), T=t_len, N=n, A=a, R=rows, variant=variant, gamma=gamma,
                unused=unused, action=action.reshape(t_len, n),
                q=rs.standard_normal((t_len, n, a)).astype(np.float32),
                reward=np.sign(rs.standard_normal((t_len, n))).astype(np.float32),
                mask=_mask_of(rs, (t_len, n), {"mask0": "zeros", "mask1": "ones"}.get(variant)),
                boot=rs.standard_normal(n).astype(np.float32), phi=_features(rs, rows),
                w=(rs.standard_normal((a, 512)) * 0.05).astype(np.float32))


def nstep_cases():
    return [nstep_case(s) for s in NSTEP_SHAPES] + [nstep_case(s, v) for s, v in NSTEP_VARIANTS]


def nstep_path(c):
    """What the launch does at this shape: trips of the environment loop, workgroups of the four-row role, rows of the last
    of them, and the length of every action's row list."""
    act = _clamp(c["action"], c["A"]).reshape(-1)
    return dict(env_trips=-(-c["N"] // 256), row_wgs=-(-c["R"] // 4), last_rows=c["R"] - 4 * (-(-c["R"] // 4) - 1),
                lists=np.bincount(act, minlength=c["A"]))


def nstep_ref(c):
    rows, a = c["R"], c["A"]
    act = _clamp(c["action"], a).reshape(-1)
    ret = _returns(c["reward"], c["mask"], c["boot"], c["gamma"], D).reshape(-1)
    diff = _f(c["q"]).reshape(rows, a)[np.arange(rows), act] - ret
    dq = np.zeros((rows, a))
    dq[np.arange(rows), act] = diff / rows
    phi = _f(c["phi"])
    return dict(ret=ret.reshape(c["T"], c["N"]), loss=np.asarray([0.5 * np.mean(diff * diff)]), dw=dq.T @ phi, db=dq.sum(0),
                dphi=(dq @ _f(c["w"])) * (phi > 0))


def nstep_f32(c, weight_sum=_tree):
    """The kernel's order: the returns per environment, the loss one running sum over ascending rows, dW / db one accumulator
    per (action, column) from `weight_sum` over the rows (_tree: the kernel's three levels)."""
    rows, a = c["R"], c["A"]
    act = _clamp(c["action"], a).reshape(-1)
    ret = _returns(c["reward"], c["mask"], c["boot"], c["gamma"], F).reshape(-1)
    diff = c["q"].reshape(rows, a)[np.arange(rows), act] - ret
    g = diff / F(rows)
    dw, db = np.zeros((a, 512), dtype=np.float32), np.zeros(a, dtype=np.float32)
    for k in range(a):
        gk = np.where(act == k, g, F(0))
        if np.any(act == k):
            dw[k], db[k] = weight_sum(gk[:, None] * c["phi"]), weight_sum(gk)
    dphi = np.where(c["phi"] > 0, g[:, None] * c["w"][act], F(0))
    for x in (ret, diff, g, dw, db, dphi):
        assert x.dtype == np.float32
    return dict(ret=ret.reshape(c["T"], c["N"]), loss=np.asarray([F(0.5) * (_serial(diff * diff) / F(rows))]), dw=dw, db=db,
                dphi=dphi)


# ===================================================================================================== dra_oc_loss_bwd
OC_SHAPES = [(1, 1, 1, 1), (1, 1, 8, 18), (3, 1, 2, 3), (1, 257, 4, 6), (2, 300, 2, 18), (8, 256, 8, 4), (2048, 1, 1, 2)]
OC_VARIANTS = [
    ((8, 256, 8, 4), "lists"), ((8, 256, 8, 4), "init1"), ((2, 300, 2, 18), "init1"), ((8, 256, 8, 4), "eps0"),
    ((8, 256, 8, 4), "eps1"), ((2, 300, 2, 18), "ties"), ((1, 1, 8, 18), "ties"), ((2, 300, 2, 18), "ent0"),
    ((2048, 1, 1, 2), "ent0"), ((2, 300, 2, 18), "clamped"), ((3, 1, 2, 3), "clamped"), ((8, 256, 8, 4), "clamped"),
]
OC_LIST_LENGTHS = (0, 1, 255, 256, 257, 258)     # both sides of a compaction trip, of the four-row unroll and of its tail
TERM_REG, ENT_W = 0.01, 0.01


def _lists_of(rs, rows, n_opt):
    """Indices in [0, n_opt) whose counts begin with OC_LIST_LENGTHS (the other rows split over the last two), shuffled."""
    counts = list(OC_LIST_LENGTHS) + [0] * (n_opt - len(OC_LIST_LENGTHS))
    rest = rows - sum(counts)
    counts[-2] += rest // 2
    counts[-1] += rest - rest // 2
    return rs.permutation(np.repeat(np.arange(n_opt), counts)).astype(np.int64)


def oc_case(shape, variant="plain"):
    t_len, n, n_opt, n_act = shape
    rows = t_len * n
    rs = np.random.RandomState(2000 + 7 * t_len + 3 * n + 11 * n_opt + n_act + sum(map(ord, variant)))
    option, prev = (rs.randint(0, n_opt, rows).astype(np.int64) for _ in range(2))
    action = rs.randint(0, n_act, rows).astype(np.int64)
    if variant == "lists":
        option, prev = _lists_of(rs, rows, n_opt), _lists_of(rs, rows, n_opt)[::-1].copy()
    if variant == "clamped":
        option, prev, action = _sprinkle(rs, option, n_opt), _sprinkle(rs, prev[::-1], n_opt), _sprinkle(rs, action, n_act)
    q = rs.standard_normal((t_len, n, n_opt)).astype(np.float32)
    if variant == "ties":
        # every other environment (with two options a tie is v = q[prev]: all rows tied would leave beta_adv the regularizer alone)
        q[:, ::2, -1] = q[:, ::2, :-1].max(-1)      # the maximum twice, the last column among them
        q[::2, ::2, 0] = q[::2, ::2].max(-1)        # ... and, every other step, in the first column too
    logits = rs.standard_normal((t_len, n, n_act)).astype(np.float32)
    lp_row = logits.astype(D) - np.log(np.exp(logits.astype(D)).sum(-1))[..., None]
    a_in = _clamp(action, n_act).reshape(t_len, n)
    # one option: v = q (1 - eps) + q eps cancels against q[prev] and beta_adv is the regularizer alone, so any rounding of v is
    # an error of 1e-7 |q| on a value of 0.01; eps = 0.5 keeps both products exact and the case about its 2048-row list
    eps = np.full(t_len, 0.5) if n_opt == 1 else np.linspace(0.5, 0.4, t_len)
    eps = {"eps0": np.zeros(t_len), "eps1": np.ones(t_len)}.get(variant, eps).astype(np.float32)
    return dict(name="T%d-N%d-O%d-A%d-%s" % (t_len, n, n_opt, n_act, variant), T=t_len, N=n, O=n_opt, A=n_act, R=rows,
                variant=variant, gamma=0.99, term_reg=TERM_REG, ent_w=0.0 if variant == "ent0" else ENT_W,
                option=option.reshape(t_len, n), prev=prev.reshape(t_len, n), action=action.reshape(t_len, n), q=q,
                beta=rs.uniform(0.05, 0.95, (t_len, n, n_opt)).astype(np.float32), logits=logits,
                init=np.ones((t_len, n), dtype=np.float32) if variant == "init1" else (rs.rand(t_len, n) < 0.3).astype(np.float32),
                log_pi_a=np.take_along_axis(lp_row, a_in[..., None], -1)[..., 0].astype(np.float32),
                entropy=(-(np.exp(lp_row) * lp_row).sum(-1)).astype(np.float32),
                reward=np.sign(rs.standard_normal((t_len, n))).astype(np.float32), mask=_mask_of(rs, (t_len, n), None),
                boot=rs.standard_normal(n).astype(np.float32), eps=eps, phi=_features(rs, rows),
                wq=(rs.standard_normal((n_opt, 512)) * 0.05).astype(np.float32),
                wb=(rs.standard_normal((n_opt, 512)) * 0.05).astype(np.float32),
                wp=(rs.standard_normal((n_opt * n_act, 512)) * 0.05).astype(np.float32))


def oc_cases():
    return [oc_case(s) for s in OC_SHAPES] + [oc_case(s, v) for s, v in OC_VARIANTS]


def oc_path(c):
    """Environment-loop trips, compaction trips, and the list length of every fc_q / fc_pi row (by option) and fc_beta row (by
    prev_option)."""
    return dict(env_trips=-(-c["N"] // 256), compaction_trips=-(-c["R"] // 256), row_wgs=-(-c["R"] // 4),
                last_rows=c["R"] - 4 * (-(-c["R"] // 4) - 1),
                by_option=np.bincount(_clamp(c["option"], c["O"]).reshape(-1), minlength=c["O"]),
                by_prev=np.bincount(_clamp(c["prev"], c["O"]).reshape(-1), minlength=c["O"]))


def _oc_rows(c, dtype):
    """The per-row terms of phase A in `dtype`, in the kernel's operation order."""
    rows, n_opt, n_act = c["R"], c["O"], c["A"]
    one = dtype(1)
    o, p, a = (_clamp(c[k], n).reshape(-1) for k, n in (("option", n_opt), ("prev", n_opt), ("action", n_act)))
    r = np.arange(rows)
    ret = _returns(c["reward"], c["mask"], c["boot"], c["gamma"], dtype).reshape(-1)
    q = c["q"].astype(dtype).reshape(rows, n_opt)
    qo = q[r, o]
    diff, adv = qo - ret, ret - qo
    qsum = q[:, 0].copy()
    for j in range(1, n_opt):
        qsum = qsum + q[:, j]
    e_t = np.repeat(c["eps"].astype(dtype), c["N"])
    v = q.max(-1) * (one - e_t) + (qsum / dtype(n_opt)) * e_t
    badv = (q[r, p] - v) + dtype(F(c["term_reg"]))
    bp = c["beta"].astype(dtype).reshape(rows, n_opt)[r, p]
    keep = one - c["init"].astype(dtype).reshape(-1)
    gz = (((bp * (one - bp)) * badv) * keep) / dtype(rows)
    x = c["logits"].astype(dtype).reshape(rows, n_act)
    m = x.max(-1)
    se = np.zeros(rows, dtype=dtype)
    for j in range(n_act):
        se = se + np.exp(x[:, j] - m)
    lse = m + np.log(se)
    lp = x - lse[:, None]
    ent = np.zeros(rows, dtype=dtype)
    for j in range(n_act):
        ent = ent - np.exp(lp[:, j]) * lp[:, j]
    g = diff / dtype(rows)
    ge = -(dtype(F(c["ent_w"])) / dtype(rows))
    onehot = (np.arange(n_act)[None, :] == a[:, None]).astype(dtype)
    dl = g[:, None] * (onehot - np.exp(lp)) - (ge * np.exp(lp)) * (lp + ent[:, None])
    terms = dict(q=dtype(0.5) * (diff * diff),
                 pi=-(c["log_pi_a"].astype(dtype).reshape(-1) * adv) - dtype(F(c["ent_w"])) * c["entropy"].astype(dtype).reshape(-1),
                 beta=(bp * badv) * keep)
    for x_ in (ret, adv, badv, g, gz, dl) + tuple(terms.values()):
        assert x_.dtype == dtype
    return dict(o=o, p=p, a=a, ret=ret, adv=adv, badv=badv, g=g, gz=gz, dl=dl, terms=terms)


def oc_ref(c):
    """OptionCritic_agent.py:95-117 and the heads' backward in plain float64, written apart from _oc_rows (the float32
    transcription's text), so that a slip in one of the two shows on the CPU."""
    t_len, n, n_opt, n_act, rows = c["T"], c["N"], c["O"], c["A"], c["R"]
    gamma, term, ent_w = float(F(c["gamma"])), float(F(c["term_reg"])), float(F(c["ent_w"]))
    option, prev, action = (np.clip(c[k], 0, m - 1) for k, m in (("option", n_opt), ("prev", n_opt), ("action", n_act)))
    ret, nxt = np.zeros((t_len, n)), _f(c["boot"])
    for t in reversed(range(t_len)):
        nxt = _f(c["reward"][t]) + gamma * _f(c["mask"][t]) * nxt
        ret[t] = nxt
    q, eps = _f(c["q"]), _f(c["eps"])[:, None]
    q_o = np.take_along_axis(q, option[..., None], -1)[..., 0]
    adv = ret - q_o
    v = q.max(-1) * (1.0 - eps) + q.mean(-1) * eps
    beta_adv = np.take_along_axis(q, prev[..., None], -1)[..., 0] - v + term
    beta_prev = np.take_along_axis(_f(c["beta"]), prev[..., None], -1)[..., 0]
    not_init = 1.0 - _f(c["init"])
    q_loss = (0.5 * (q_o - ret) ** 2).mean()
    pi_loss = (-_f(c["log_pi_a"]) * adv - ent_w * _f(c["entropy"])).mean()
    beta_loss = (beta_prev * beta_adv * not_init).mean()
    # gradients of the three means with respect to the heads' outputs
    logits = _f(c["logits"]).reshape(rows, n_act)
    log_p = logits - logits.max(-1, keepdims=True)
    log_p = log_p - np.log(np.exp(log_p).sum(-1, keepdims=True))
    p = np.exp(log_p)
    entropy = -(p * log_p).sum(-1, keepdims=True)
    onehot = np.eye(n_act)[action.reshape(-1)]
    # d(-log pi(a) adv)/dlogits = -adv (onehot - p);  d(-ent_w H)/dlogits = ent_w p (log p + H);  both over rows
    dlogits = (-adv.reshape(-1, 1) * (onehot - p) + ent_w * p * (log_p + entropy)) / rows
    opt_1h, prev_1h = np.eye(n_opt)[option.reshape(-1)], np.eye(n_opt)[prev.reshape(-1)]
    dq = opt_1h * ((q_o - ret).reshape(-1, 1) / rows)
    dz = prev_1h * ((beta_prev * (1.0 - beta_prev) * beta_adv * not_init).reshape(-1, 1) / rows)
    dpi = (opt_1h[:, :, None] * dlogits[:, None, :]).reshape(rows, n_opt * n_act)
    phi = _f(c["phi"])
    return dict(ret=ret, adv=adv, beta_adv=beta_adv, loss=np.asarray([pi_loss + q_loss + beta_loss, q_loss, pi_loss, beta_loss]),
                dw_q=dq.T @ phi, db_q=dq.sum(0), dw_pi=dpi.T @ phi, db_pi=dpi.sum(0), dw_beta=dz.T @ phi, db_beta=dz.sum(0),
                dphi=(dq @ _f(c["wq"]) + dpi @ _f(c["wp"]) + dz @ _f(c["wb"])) * (phi > 0))


def _oc_loss_sum(x):
    """The kernel's mean numerator: thread t of 256 adds rows t, t + 256, ... in order, a 64-lane xor butterfly (32, 16, ... 1)
    per wave, then the four waves in order."""
    x = np.asarray(x, dtype=np.float32)
    trips = -(-x.shape[0] // 256)
    pad = np.zeros(trips * 256, dtype=np.float32)
    pad[:x.shape[0]] = x
    v = _serial(pad.reshape(trips, 256)).reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def oc_f32(c):
    rows, n_opt, n_act = c["R"], c["O"], c["A"]
    t = _oc_rows(c, F)
    phi = c["phi"]
    out = dict(dw_q=np.zeros((n_opt, 512), F), db_q=np.zeros(n_opt, F), dw_beta=np.zeros((n_opt, 512), F), db_beta=np.zeros(n_opt, F),
               dw_pi=np.zeros((n_opt * n_act, 512), F), db_pi=np.zeros(n_opt * n_act, F))
    for o in range(n_opt):
        sel = np.nonzero(t["o"] == o)[0]
        out["dw_q"][o], out["db_q"][o] = _serial(t["g"][sel, None] * phi[sel]), _serial(t["g"][sel])
        for a in range(n_act):
            gv = t["dl"][sel, a]
            out["dw_pi"][o * n_act + a], out["db_pi"][o * n_act + a] = _serial(gv[:, None] * phi[sel]), _serial(gv)
        sel = np.nonzero(t["p"] == o)[0]
        out["dw_beta"][o], out["db_beta"][o] = _serial(t["gz"][sel, None] * phi[sel]), _serial(t["gz"][sel])
    vp = np.zeros((rows, 512), dtype=np.float32)
    for a in range(n_act):
        vp = vp + t["dl"][:, a, None] * c["wp"][t["o"] * n_act + a]
    v = (t["g"][:, None] * c["wq"][t["o"]] + vp) + t["gz"][:, None] * c["wb"][t["p"]]
    m = [_oc_loss_sum(t["terms"][k]) / F(rows) for k in ("q", "pi", "beta")]
    shape = (c["T"], c["N"])
    out.update(ret=t["ret"].reshape(shape), adv=t["adv"].reshape(shape), beta_adv=t["badv"].reshape(shape),
               loss=np.asarray([(m[1] + m[0]) + m[2], m[0], m[1], m[2]]), dphi=np.where(phi > 0, v, F(0)))
    for x in out.values():
        assert x.dtype == np.float32
    return out


# ============================================================================================ dra_dueling_atoms_fwd / _bwd
DUELING_SHAPES = [(1, 1, 1), (1, 1, 51), (5, 3, 51), (5, 18, 52), (257, 2, 1)]


def dueling_case(shape):
    b, a, z = shape
    rs = np.random.RandomState(3000 + 100 * b + 10 * a + z)
    return dict(name="B%d-A%d-Z%d" % shape, B=b, A=a, Z=z, wgs=-(-(b * z) // 256), last_wg=b * z - 256 * (-(-(b * z) // 256) - 1),
                value=rs.standard_normal((b, z)).astype(np.float32), adv=rs.standard_normal((b, a, z)).astype(np.float32),
                g=rs.standard_normal((b, a, z)).astype(np.float32))


def dueling_cases():
    return [dueling_case(s) for s in DUELING_SHAPES]


def dueling_ref(c):
    adv, g = _f(c["adv"]), _f(c["g"])
    return dict(logits=_f(c["value"])[:, None, :] + (adv - adv.mean(1, keepdims=True)), d_value=g.sum(1),
                d_adv=g - g.mean(1, keepdims=True))


def dueling_f32(c):
    a = F(c["A"])
    s, sg = _serial(np.moveaxis(c["adv"], 1, 0)), _serial(np.moveaxis(c["g"], 1, 0))
    return dict(logits=c["value"][:, None, :] + (c["adv"] - (s / a)[:, None, :]), d_value=sg, d_adv=c["g"] - (sg / a)[:, None, :])


# ====================================================================================================== dra_per_weights_dev
PER_BATCHES = (1, 63, 64, 65, 1024)
PER_ALPHAS = (0.5, 0.6)
PER_BETAS = (0.0, 0.4, 1.0)
PER_EPS = 0.01


def per_cases():
    """Every batch x alpha x beta; the smallest sampling probability (the largest weight) alternates between the last element
    and the first element of the last wave."""
    out = []
    for b in PER_BATCHES:
        for i, alpha in enumerate(PER_ALPHAS):
            for k, beta in enumerate(PER_BETAS):
                rs = np.random.RandomState(4000 + b + 10 * i + k)
                sp = rs.uniform(0.2, 2.0, b) / b
                where = b - 1 if (i + k) % 2 == 0 else 64 * ((b - 1) // 64)
                sp[where] = 0.05 / b
                out.append(dict(name="B%d-alpha%g-beta%g" % (b, alpha, beta), B=b, alpha=alpha, beta=beta, eps=PER_EPS, argmax=where,
                                sp=sp.astype(np.float32), loss_vec=(rs.standard_normal(b) * 2).astype(np.float32)))
    return out


def per_ref(c):
    prio = (np.abs(_f(c["loss_vec"])) + D(F(c["eps"]))) ** D(F(c["alpha"]))
    w = (_f(c["sp"]) * c["B"] + D(F(1e-6))) ** -D(F(c["beta"]))
    return dict(prio=prio, w=w / w.max())


def per_f32(c):
    ad = np.abs(c["loss_vec"]) + F(c["eps"])
    prio = np.sqrt(ad) if F(c["alpha"]) == F(0.5) else np.power(ad, F(c["alpha"]))
    w = np.power(c["sp"] * F(c["B"]) + F(1e-6), -F(c["beta"]))
    return dict(prio=prio, w=w / w.max())


# ============================================================================================ dra_noisy_linear_fwd / _bwd
NOISY_SHAPES = [(2, 8, 3), (3, 20, 33), (4, 36, 1), (7, 516, 31), (8, 20, 32), (31, 36, 33), (33, 516, 65), (65, 8, 31),
                (1024, 36, 33), (9, 7, 5), (33, 513, 2)]
NOISY_ACTS = ("none", "relu")
NOISY_OFFSET_SHAPES = [(4, 36, 33), (33, 36, 33)]       # K % 4 == 0 at column-kernel rows and at MFMA rows


def noise_f(e):
    e = np.asarray(e)
    return np.copysign(np.sqrt(np.abs(e)), e)


def noisy_case(shape, zero_noise=False):
    rows, k, n = shape
    rs = np.random.RandomState(5003 + 13 * rows + 7 * k + n)
    noise = lambda m: (rs.standard_normal(m) * 0.5).astype(np.float32)
    c = dict(name="rows%d-K%d-N%d%s" % (rows, k, n, "-zero-noise" if zero_noise else ""), rows=rows, K=k, N=n,
             x=rs.standard_normal((rows, k)).astype(np.float32), w_mu=(rs.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32),
             w_sigma=(rs.standard_normal((n, k)) * 0.5 / np.sqrt(k)).astype(np.float32), b_mu=(rs.standard_normal(n) * 0.1).astype(np.float32),
             b_sigma=(rs.standard_normal(n) * 0.1).astype(np.float32), e_in=noise(k), e_out=noise(n), e_b=noise(n),
             g=rs.standard_normal((rows, n)).astype(np.float32), dx_add=rs.standard_normal((rows, k)).astype(np.float32))
    if zero_noise:
        for key in ("e_in", "e_out", "e_b"):
            c[key] = np.where(rs.rand(c[key].size) < 0.5, F(0.0), F(-0.0)).astype(np.float32)
    return c


def noisy_cases():
    return [noisy_case(s) for s in NOISY_SHAPES]


def ceil_div(a, b):
    return -(-a // b)


def noisy_fwd_plan(rows, k, n):
    """fwd_plan of csrc/noisy.hip."""
    rt = 2 if rows > 32 else 1
    col_tiles, row_groups, chunks = ceil_div(n, 32), ceil_div(rows, 32 * rt), ceil_div(k, 32)
    cpw = max(2, ceil_div(chunks, 4 * max(1, 512 // (col_tiles * row_groups))))
    return dict(rt=rt, col_tiles=col_tiles, row_groups=row_groups, chunks=chunks, cpw=cpw, kb=ceil_div(ceil_div(chunks, cpw), 4))


def noisy_bwd_plan(rows, k, n):
    """bwd_plan of csrc/noisy.hip."""
    col_blocks, row_groups = ceil_div(k, 128), ceil_div(rows, 32)
    npw = ceil_div(n, 4 * max(1, 256 // (col_blocks * row_groups)))
    npw = max(2, npw + (npw & 1))
    return dict(col_blocks=col_blocks, row_groups=row_groups, npw=npw, nb=ceil_div(n, 4 * npw))


def noisy_workspace(rows, k, n):
    """(forward, backward) floats dra_noisy_workspace_floats reports."""
    return noisy_fwd_plan(rows, k, n)["kb"] * rows * n, noisy_bwd_plan(rows, k, n)["nb"] * rows * k


def noisy_path(rows, k, n, aligned=True):
    """Which forward / input-gradient kernels a launch with 16-byte aligned (or 4-byte offset) operands selects."""
    vec = k % 4 == 0 and aligned
    fwd = "mfma%d" % noisy_fwd_plan(rows, k, n)["rt"] if rows >= 8 and vec else "col%d-%s" % (1 if rows == 1 else 4, "vec" if vec else "scalar")
    return dict(fwd=fwd, bwd_w="vec" if vec else "scalar", bwd_x="mfma" if vec else "any")


def noisy_ref(c, act, x_relu=False, dx_add=False):
    x, g0 = _f(c["x"]), _f(c["g"])
    fi, fo, fb = noise_f(_f(c["e_in"])), noise_f(_f(c["e_out"])), noise_f(_f(c["e_b"]))
    eps_w = fo[:, None] * fi[None, :]
    w = _f(c["w_mu"]) + _f(c["w_sigma"]) * eps_w
    pre = x @ w.T + (_f(c["b_mu"]) + _f(c["b_sigma"]) * fb)
    dw_mu = g0.T @ x
    dx = g0 @ w
    if dx_add:
        dx = dx + _f(c["dx_add"])
    if x_relu:
        dx = dx * (x > 0)
    return dict(y=np.maximum(pre, 0) if act == "relu" else pre, plain=x @ _f(c["w_mu"]).T + _f(c["b_mu"]), dw_mu=dw_mu,
                dw_sigma=dw_mu * eps_w, db_mu=g0.sum(0), db_sigma=g0.sum(0) * fb, dx=dx)


def noisy_f32(c, act):
    """float32 with ONE accumulator per output over ascending k / n / b.  For dw_* / db_* that is noisy_bwd_w_kernel's own
    order.  For y and dx it is NOT the kernels' order (K / N slices per wave, waves in wave order, slabs in slab order): it is a
    longer chain of additions than any of theirs, used as an upper estimate of the inputs' noise floor."""
    x, g0 = c["x"], c["g"]
    fi, fo, fb = (noise_f(c[k]).astype(np.float32) for k in ("e_in", "e_out", "e_b"))
    am = _serial(x.T[:, :, None] * c["w_mu"].T[:, None, :])
    as_ = _serial((x * fi).T[:, :, None] * c["w_sigma"].T[:, None, :])
    pre = (am + fo * as_) + (c["b_mu"] + c["b_sigma"] * fb)
    dw_mu = _serial(g0[:, :, None] * x[:, None, :])
    dm = _serial(g0.T[:, :, None] * c["w_mu"][:, None, :])
    ds = _serial((g0 * fo).T[:, :, None] * c["w_sigma"][:, None, :])
    db = _serial(g0)
    out = dict(y=np.maximum(pre, F(0)) if act == "relu" else pre, dw_mu=dw_mu, dw_sigma=dw_mu * (fo[:, None] * fi[None, :]), db_mu=db,
               db_sigma=db * fb, dx=dm + fi * ds)
    for v in out.values():
        assert v.dtype == np.float32
    return out


# ===================================================================== rollout heads (rollout_roles.h), Gaussian head
def fold_f32(slabs, bias):
    """fc4's finish in float32, slab 0 first, then + bias, ReLU: the kernels' order (fold_row_slabs_wg); bit-exact."""
    v = slabs[0].copy()
    for s in range(1, slabs.shape[0]):
        v = v + slabs[s]
    return np.maximum(v + bias[None, :], F(0))


def head_f32(phi, w, b):
    """heads_row_outputs_from / heads3_row_outputs_lds per output: lane l of 64 adds its products k = l, l + 64, ... in order,
    a xor butterfly (32, 16, ... 1) over the lanes, + bias."""
    prod = (phi[:, None, :] * w[None, :, :]).reshape(phi.shape[0], w.shape[0], 8, 64)
    v = np.moveaxis(_serial(np.moveaxis(prod, 2, 0)), -1, 0)            # [lane][row][output]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ off]
    return v[0] + (b if b is not None else F(0))


def _head_base(rs, batch):
    return dict(slabs=(rs.standard_normal((28, batch, 512)) * 0.05).astype(np.float32),
                fold_bias=(rs.standard_normal(512) * 0.05).astype(np.float32))


Q_HEAD_A = (1, 7, 8, 9, 63, 64)
Q_HEAD_B = (1, 3, 33)
Q_TIES = ("none", "first", "last")          # first: columns 0, A // 2 and A - 1 tie at the top; last: A // 2 and A - 1
Q_EXPLORE = ("mixed", "all", "none")


def q_head_case(a, batch, ties=None, explore=None, bias=None):
    i = Q_HEAD_A.index(a) + 2 * Q_HEAD_B.index(batch)
    ties = Q_TIES[i % 3] if ties is None else ties
    explore = Q_EXPLORE[(i // 3 + i) % 3] if explore is None else explore
    bias = (i % 2 == 0) if bias is None else bias
    if a < 3 and ties == "last":
        ties = "first"
    rs = np.random.RandomState(6000 + 100 * a + batch)
    c = dict(_head_base(rs, batch), name="A%d-B%d-ties-%s-explore-%s-%s" % (a, batch, ties, explore, "bias" if bias else "nobias"),
             A=a, B=batch, ties=ties, explore_kind=explore, w=(rs.standard_normal((a, 512)) * 0.05).astype(np.float32),
             b=(rs.standard_normal(a) * 0.05).astype(np.float32) if bias else None,
             explore={"all": np.ones(batch), "none": np.zeros(batch)}.get(explore, rs.rand(batch) < 0.4).astype(np.uint8),
             random_action=rs.randint(0, a, batch).astype(np.int64), winner=None)
    if ties != "none":
        tied = sorted({0, a // 2, a - 1} if ties == "first" else {a // 2, a - 1})
        c["w"][tied] = np.abs(c["w"][tied[0]])              # phi >= 0: an all-positive row is the maximum of every sample
        if bias:
            c["b"][tied] = F(0.5)
        c["tied"], c["winner"] = tied, tied[0]
    return c


def q_head_cases():
    return [q_head_case(a, b) for a in Q_HEAD_A for b in Q_HEAD_B]


def q_head_ref(c):
    phi = fold_f32(c["slabs"], c["fold_bias"])
    return dict(phi=phi, q=_f(phi) @ _f(c["w"]).T + (_f(c["b"]) if c["b"] is not None else 0.0))


def q_head_decide(c, q):
    """The head's decisions from float32 scores q [B, A] (the kernel's own): np.argmax's rule, the host-planned exploration."""
    greedy = np.argmax(q, axis=-1)
    return dict(action=np.where(c["explore"] != 0, c["random_action"], greedy).astype(np.int64), max=q[np.arange(q.shape[0]), greedy])


OC_HEAD_OA = ((1, 1), (2, 2), (1, 7), (4, 6), (3, 9), (8, 18))       # 3, 8, 9, 32, 33 and 160 outputs
OC_HEAD_B = (1, 5)
OC_HEAD_EPS = (0.0, 1.0, 0.3)
ALMOST_ONE = float(np.nextafter(F(1), F(0)))
OC_UNIFORMS = ("random",) + tuple("col%d-%s" % (j, v) for j in range(3) for v in ("zero", "almost-one"))
OC_INIT = ("mixed", "all", "none")
OC_PREV = ("in-range", "minus-one", "count")


def oc_head_case(n_opt, n_act, batch, eps, k=None):
    """Case k of the (O, A) x B x eps table; the uniforms / init / prev_option / bias variants cycle with k."""
    if k is None:
        k = (OC_HEAD_OA.index((n_opt, n_act)) * len(OC_HEAD_B) + OC_HEAD_B.index(batch)) * len(OC_HEAD_EPS) + OC_HEAD_EPS.index(eps)
    uni, init, prev, bias = OC_UNIFORMS[k % 7], OC_INIT[(k // 2) % 3], OC_PREV[(k // 3 + k) % 3], k % 4 != 1
    rs = np.random.RandomState(7000 + k)
    c = dict(_head_base(rs, batch), O=n_opt, A=n_act, B=batch, eps=eps, uniforms=uni, init_kind=init, prev_kind=prev, bias=bias,
             name="O%d-A%d-B%d-eps%g-u-%s-init-%s-prev-%s-%s" % (n_opt, n_act, batch, eps, uni, init, prev, "bias" if bias else "nobias"),
             exact=eps in (0.0, 1.0) or uni != "random",
             wq=(rs.standard_normal((n_opt, 512)) * 0.05).astype(np.float32), wb=(rs.standard_normal((n_opt, 512)) * 0.1).astype(np.float32),
             wp=(rs.standard_normal((n_opt * n_act, 512)) * 0.2).astype(np.float32),
             bq=(rs.standard_normal(n_opt) * 0.05).astype(np.float32) if bias else None,
             bb=(rs.standard_normal(n_opt) * 0.05).astype(np.float32) if bias else None,
             bp=(rs.standard_normal(n_opt * n_act) * 0.05).astype(np.float32) if bias else None,
             uniform=rs.rand(batch, 3).astype(np.float32), mask=(rs.rand(batch) > 0.3).astype(np.float32),
             prev_option=rs.randint(0, n_opt, batch).astype(np.int64),
             init={"all": np.ones(batch), "none": np.zeros(batch)}.get(init, np.arange(batch) % 2 == 0).astype(np.uint8))
    if uni != "random":
        c["uniform"][:, int(uni[3])] = F(0.0) if uni.endswith("zero") else F(ALMOST_ONE)
    if prev != "in-range":
        c["prev_option"][::2] = -1 if prev == "minus-one" else n_opt
    return c


def oc_head_cases():
    return [oc_head_case(o, a, b, e) for o, a in OC_HEAD_OA for b in OC_HEAD_B for e in OC_HEAD_EPS]


def oc_head_ref(c):
    """phi (bit-exact float32) and the float64 q, beta and logits [B, O, A] of every option."""
    phi = fold_f32(c["slabs"], c["fold_bias"])
    p64 = _f(phi)
    bias = lambda k: _f(c[k]) if c[k] is not None else 0.0
    return dict(phi=phi, q=p64 @ _f(c["wq"]).T + bias("bq"), beta=1.0 / (1.0 + np.exp(-(p64 @ _f(c["wb"]).T + bias("bb")))),
                logits=(p64 @ _f(c["wp"]).T + bias("bp")).reshape(c["B"], c["O"], c["A"]))


def oc_head_f32(c):
    phi = fold_f32(c["slabs"], c["fold_bias"])
    zb = head_f32(phi, c["wb"], c["bb"])
    return dict(phi=phi, q=head_f32(phi, c["wq"], c["bq"]), beta=F(1) / (F(1) + np.exp(-zb)),
                logits=head_f32(phi, c["wp"], c["bp"]).reshape(c["B"], c["O"], c["A"]))


def inv_cdf_f32(p, u):
    """inv_cdf_row: the row divided by its float32 sum (index order), then the first k whose running float32 sum exceeds u,
    the last index when none does.  Returns (k, the running sums)."""
    p = np.asarray(p, dtype=np.float32)
    s = F(0)
    for x in p:
        s = s + x
    cum, cums = F(0), []
    for x in p / s:
        cum = cum + x
        cums.append(cum)
    hit = [k for k, v in enumerate(cums) if v > F(u)]
    return (hit[0] if hit else len(p) - 1), np.asarray(cums, dtype=np.float32)


def categorical_f32(x, u):
    """categorical_row of common.h on float32 logits x at the uniform u -> action, log pi(a), entropy, the running sums."""
    x = np.asarray(x, dtype=np.float32)
    m = x.max()
    se = F(0)
    for v in x:
        se = se + np.exp(v - m)
    lse = m + np.log(se)
    ent, cum, cums, act = F(0), F(0), [], None
    for k, v in enumerate(x):
        lp = v - lse
        p = np.exp(lp)
        ent = ent - p * lp
        cum = cum + p
        cums.append(cum)
        if act is None and cum > F(u):
            act = k
    act = len(x) - 1 if act is None else act
    return act, x[act] - lse, ent, np.asarray(cums, dtype=np.float32)


def boundary_margin(cums, u):
    """Distance of u from the nearest boundary between two DIFFERENT outcomes (the last running sum separates the last index
    from itself: it decides nothing)."""
    return float(np.abs(cums[:-1].astype(np.float64) - float(u)).min()) if len(cums) > 1 else 1.0


def oc_head_decide(c, q, beta, logits_of):
    """The head's decisions from its own float32 q / beta [B, O] (sample_option in the kernel's float32 order: exact) and, per
    row, the float32 logits of the option it chose (logits_of(row, option) -> [A]).  Returns option, action, log_pi_a, entropy
    and the action's boundary margin per row."""
    n_opt, e = c["O"], F(c["eps"])
    out = dict(option=[], action=[], log_pi_a=[], entropy=[], margin=[])
    for r in range(c["B"]):
        g = int(np.argmax(q[r]))
        base, top = e / F(n_opt), (F(1) - e) + e / F(n_opt)
        pi_opt = np.full(n_opt, base, dtype=np.float32)
        pi_opt[g] = top
        prev = int(min(max(int(c["prev_option"][r]), 0), n_opt - 1))
        keep = (np.arange(n_opt) == prev).astype(np.float32)
        pi_hat = (F(1) - beta[r]) * keep + beta[r] * pi_opt
        fresh, continued = inv_cdf_f32(pi_opt, c["uniform"][r, 0])[0], inv_cdf_f32(pi_hat, c["uniform"][r, 1])[0]
        option = fresh if c["init"][r] else continued
        act, lp, ent, cums = categorical_f32(logits_of(r, option), c["uniform"][r, 2])
        for k, v in zip(("option", "action", "log_pi_a", "entropy", "margin"), (option, act, lp, ent, boundary_margin(cums, c["uniform"][r, 2]))):
            out[k].append(v)
    return {k: np.asarray(v) for k, v in out.items()}


GAUSS_N = (255, 257, 1025)
GAUSS_A = (1, 64)                                   # kHeadMaxA of csrc/a2c_mlp.hip
GAUSS_STD = (-8.0, 0.0, 3.0, 19.9, 20.1, 30.0)     # both sides of softplus's threshold; scale from 3e-4 to 30


def gauss_case(n, a):
    rs = np.random.RandomState(8000 + 100 * n + a)
    std = np.asarray([GAUSS_STD[(i + n) % len(GAUSS_STD)] for i in range(a)], dtype=np.float32)
    z = rs.randn(n, a) * 1.5
    z = np.where(rs.rand(n, a) < 0.4, np.sign(z) * rs.uniform(3.0, 9.0, size=(n, a)), z).astype(np.float32)      # saturated tanh
    scale = np.where(std > 20.0, std, np.log1p(np.exp(np.minimum(std, 20.0)))).astype(np.float64)
    k = rs.uniform(-6.0, 6.0, size=(n, a))
    k.flat[0], k.flat[-1] = 6.0, -6.0                # up to 6 sigma from the mean
    return dict(name="n%d-A%d" % (n, a), n=n, A=a, z=z, std=std, action=(np.tanh(z.astype(np.float64)) + k * scale).astype(np.float32),
                g_lp=rs.randn(n, 1).astype(np.float32), g_ent=rs.randn(n, 1).astype(np.float32))


def gauss_cases():
    return [gauss_case(n, a) for n in GAUSS_N for a in GAUSS_A]
