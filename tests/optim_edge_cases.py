"""Edge-shape cases and float64 references for the clip-and-step optimizer kernels (csrc/optim.hip: dra_grad_sqnorm,
dra_grad_sqnorm_segs, dra_rmsprop_step(_copy), dra_adam_step(_dev), dra_adam_step_counter, dra_clip_step_late).  NOT a test
file: pure numpy on the CPU, imported by tests/test_optim_edge_cases_host.py (which proves on the CPU that these inputs can
carry the bar, and that every case reaches the path it is named for) and by tests/test_gpu_optim_edges.py (which holds the
kernels to them).

References are PER STEP: given the float32 parameters / gradient / optimizer state a step starts from, `ref_step` evaluates
the norm, the clip coefficient min(1, max_norm / (norm + 1e-6)), the new states and the APPLIED STEP p_old - p_new in float64
(hyperparameters first rounded to float32, as the kernels hold them).  The next step restarts from the float32 state the
implementation under test produced, so no error compounds.  `f32_step` is the float32 transcription of the same formulas (every
operation rounded, no contraction: the library is built with -ffp-contract=off): the noise floor of the inputs.

Inputs: lr = 1e-2, parameters ~ N(0, 0.1^2), three steps per case with FRESH gradients whose scale is a seeded permutation of
{0.01, 1, 30}; max_norm is 0.1 x the norm a unit-scale gradient has, so the 0.01 step is not clipped and the other two are.
(At the golden fixture's lr = 2.5e-4 a step is ~3e-5 of a parameter and float32 rounding of the parameter hides a step that is
wrong by a percent; here max |p| <= 80 max |step|, which the host test asserts.)

Bar (not tuned to the kernels): BAR = 1e-5 of the reference's max-abs per tensor, the project's contraction bar."""
import numpy as np

BAR = 1e-5
LR = 1e-2
SCALES = (0.01, 1.0, 30.0)
STEPS = 3
F = np.float32

KINDS = {
    "rmsprop_centered": dict(opt="rmsprop", centered=True, lr=LR, alpha=0.95, eps=0.01),
    "rmsprop_plain": dict(opt="rmsprop", centered=False, lr=LR, alpha=0.99, eps=1e-5),
    "adam": dict(opt="adam", centered=False, lr=LR, beta1=0.9, beta2=0.999, eps=0.01 / 32),
}


def hyper(kind):
    """The kind's hyperparameters, rounded to float32 (what the kernels hold)."""
    return {k: (F(v) if isinstance(v, float) else v) for k, v in KINDS[kind].items()}


# ------------------------------------------------------------------------------------------------- the step, twice
def adam_hyper(lr, beta1, beta2, t):
    """dra_adam_hyper: {lr / (1 - b1^t), 1 / sqrt(1 - b2^t)} formed in float64 from the float32 hyperparameters."""
    lr, beta1, beta2 = float(F(lr)), float(F(beta1)), float(F(beta2))
    return lr / (1.0 - beta1 ** float(t)), 1.0 / np.sqrt(1.0 - beta2 ** float(t))


def ref_step(kind, p, g, s1, s2, sqsum, max_norm, t=1):
    """float64 step from float32 operands.  sqsum: the float64 sum of squares the norm is taken from.  Returns norm, coef,
    s1, s2 (None where the optimizer has none) and step = p_old - p_new."""
    g, s1, s2 = (None if x is None else np.asarray(x, dtype=np.float32).astype(np.float64) for x in (g, s1, s2))
    return ref_formulas(kind, g, s1, s2, sqsum, max_norm, t)


def ref_formulas(kind, g, s1, s2, sqsum, max_norm, t=1):
    """The float64 formulas of ref_step on float64 operands as they are."""
    hp = hyper(kind)
    norm = float(np.sqrt(np.float64(sqsum)))
    coef = min(1.0, float(F(max_norm)) / (norm + 1e-6)) if max_norm and max_norm > 0 else 1.0
    gk = g * coef
    if hp["opt"] == "rmsprop":
        alpha, eps, lr = float(hp["alpha"]), float(hp["eps"]), float(hp["lr"])
        s1n = alpha * s1 + (1.0 - alpha) * gk * gk
        if hp["centered"]:
            s2n = alpha * s2 + (1.0 - alpha) * gk
            avg = np.sqrt(s1n - s2n * s2n) + eps
        else:
            s2n, avg = None, np.sqrt(s1n) + eps
        step = lr * gk / avg
    else:
        b1, b2, eps = float(hp["beta1"]), float(hp["beta2"]), float(hp["eps"])
        step_size, inv_sqrt_bc2 = adam_hyper(hp["lr"], hp["beta1"], hp["beta2"], t)
        s1n = b1 * s1 + (1.0 - b1) * gk
        s2n = b2 * s2 + (1.0 - b2) * gk * gk
        step = step_size * s1n / (np.sqrt(s2n) * inv_sqrt_bc2 + eps)
    return dict(norm=norm, coef=coef, s1=s1n, s2=s2n, step=step)


def f32_step(kind, p, g, s1, s2, sqsum, max_norm, t=1):
    """The same step as the kernels write it, in float32 numpy (rmsprop_elem of common.h; the Adam element of
    adam_step_kernel): norm rounded to float32, coef = max_norm / (norm + 1e-6f) clamped to 1, every product and sum
    rounded.  Returns the float32 p, s1, s2, norm, coef and step = float64(p_old) - float64(p_new)."""
    hp = hyper(kind)
    p, g, s1 = (np.asarray(x, dtype=np.float32) for x in (p, g, s1))
    norm = F(np.sqrt(np.float64(sqsum)))
    coef = F(1.0)
    if max_norm and max_norm > 0:
        coef = F(max_norm) / (norm + F(1e-6))
        if coef > F(1.0):
            coef = F(1.0)
    gk = g * coef
    if hp["opt"] == "rmsprop":
        alpha, eps, lr = hp["alpha"], hp["eps"], hp["lr"]
        oma = F(1.0) - alpha
        s1n = s1 * alpha + (oma * gk) * gk
        if hp["centered"]:
            s2n = np.asarray(s2, dtype=np.float32) * alpha + oma * gk
            avg = np.sqrt(s1n - s2n * s2n) + eps
        else:
            s2n, avg = None, np.sqrt(s1n) + eps
        pn = p - lr * (gk / avg)
    else:
        b1, b2, eps = hp["beta1"], hp["beta2"], hp["eps"]
        step_size, inv_sqrt_bc2 = (F(x) for x in adam_hyper(hp["lr"], b1, b2, t))
        omb1, omb2 = F(1.0) - b1, F(1.0) - b2
        s1n = s1 * b1 + omb1 * gk
        s2n = np.asarray(s2, dtype=np.float32) * b2 + (omb2 * gk) * gk
        pn = p - step_size * (s1n / (np.sqrt(s2n) * inv_sqrt_bc2 + eps))
    for x in (pn, s1n) + (() if s2n is None else (s2n,)):
        assert x.dtype == np.float32
    return dict(p=pn, s1=s1n, s2=s2n, norm=norm, coef=coef, step=p.astype(np.float64) - pn.astype(np.float64))


def sqsum64(g):
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    return float((g * g).sum())


# ------------------------------------------------------------------------------------------------------ fold orders
def fold_grouped(slabs, n_groups):
    """The fold workgroups' order: group g adds slabs g, g + n_groups, ... (from zero), then the groups are added in order
    0 .. n_groups - 1.  fold_norm_kernel: n_groups = 16; late_step_kernel: late_groups(n_slabs)."""
    slabs = np.asarray(slabs, dtype=np.float32)
    groups = []
    for g in range(n_groups):
        acc = np.zeros(slabs.shape[1], dtype=np.float32)
        for s in range(g, slabs.shape[0], n_groups):
            acc = acc + slabs[s]
        groups.append(acc)
    r = groups[0].copy()
    for g in range(1, n_groups):
        r = r + groups[g]
    return r


def late_groups(n_slabs):
    return 4 if n_slabs <= 64 else 16


def fold_in_order(slabs):
    """grad_sqnorm_kernel: slab 0, then + slab 1, + slab 2, ..."""
    slabs = np.asarray(slabs, dtype=np.float32)
    r = slabs[0].copy()
    for s in range(1, slabs.shape[0]):
        r = r + slabs[s]
    return r


def padded_slabs(rs, n_slabs, count, stride, scale=1.0):
    """[n_slabs, stride] float32, N(0, scale^2 / n_slabs) in the first `count` columns and NaN in the padding."""
    sl = np.full((n_slabs, stride), np.nan, dtype=np.float32)
    sl[:, :count] = (rs.standard_normal((n_slabs, count)) * (scale / np.sqrt(n_slabs))).astype(np.float32)
    return sl


# ----------------------------------------------------------------------------------------- launcher arithmetic
def step_blocks(n):
    """step_blocks() of optim.hip: one thread slot per float4, 2 float4 per thread, 256 threads."""
    return max(1, -(-(n >> 2) // 512))


def step_path(n):
    """What the 2-float4 step kernels do at n floats: workgroups, float4s in slot 0 / slot 1 of the LAST workgroup, tail."""
    n4, b = n >> 2, step_blocks(n)
    last = n4 - 512 * (b - 1)
    return dict(blocks=b, last_slot0=min(last, 256), last_slot1=max(0, last - 256), tail=n - 4 * n4)


def sqnorm_path(n):
    """grad_sqnorm_kernel: 512 workgroups x 256 threads, one float4 per thread and trip."""
    n4 = n >> 2
    return dict(trips=-(-n4 // (512 * 256)), tail=n - 4 * n4)


def adam_path(n):
    """adam_step_kernel: scalar grid-stride over min(2048, ceil(n / 256)) workgroups."""
    b = min(2048, -(-n // 256))
    return dict(blocks=b, trips=-(-n // (b * 256)))


def segs_path(counts, n_slabs, tail):
    """make_fold_plan: fold workgroups (64 float4 each up to 32 slabs, 16 above), plain workgroups (1024 float4 per
    stride) and the strides a plain workgroup walks when 4096 partials do not hold one workgroup per stride."""
    fold = sum(-(-(c >> 2) // (64 if ns <= 32 else 16)) for c, ns in zip(counts, n_slabs))
    pb, iters, room = -(-(tail >> 2) // 1024), 1, 4096 - fold
    if pb > room:
        iters = -(-pb // room)
        pb = -(-pb // iters)
    return dict(fold_blocks=fold, plain_blocks=pb, plain_iters=iters, partials=fold + pb)


def late_path(count, n_slabs, n):
    """clip_step_late_impl: fold workgroups of 256 / NG float4, plain workgroups of 3 x 256 float4, the tail."""
    ng = late_groups(n_slabs)
    epb = 256 // ng
    c4, n4 = count >> 2, n >> 2
    fold = -(-c4 // epb)
    plain = -(-(n4 - c4) // 768)
    return dict(ng=ng, fold_blocks=fold, last_fold=c4 - epb * (fold - 1), plain_blocks=plain,
                last_plain=(n4 - c4) - 768 * (plain - 1) if plain else 0, tail=n - 4 * n4)


# ------------------------------------------------------------------------------------------------------------ cases
def _scales(rs):
    return [float(s) for s in rs.permutation(SCALES)]


def _unit_max_norm(unit_norm):
    return float(F(0.1 * unit_norm))


# dra_rmsprop_step(_copy) centered / plain and dra_adam_step_counter: 2048 floats per workgroup
STEP_SHAPES = [
    (4, dict(blocks=1, last_slot0=1, last_slot1=0, tail=0)),            # the minimum
    (7, dict(blocks=1, last_slot0=1, last_slot1=0, tail=3)),            # one float4 plus a tail of 3
    (1027, dict(blocks=1, last_slot0=256, last_slot1=0, tail=3)),       # slot 0 full plus a tail
    (1028, dict(blocks=1, last_slot0=256, last_slot1=1, tail=0)),       # the first float4 of slot 1
    (2048, dict(blocks=1, last_slot0=256, last_slot1=256, tail=0)),     # exactly one workgroup
    (2052, dict(blocks=2, last_slot0=1, last_slot1=0, tail=0)),         # a second workgroup that holds one float4
    (6151, dict(blocks=4, last_slot0=1, last_slot1=0, tail=3)),         # four workgroups, the last partial, a tail in block 0
]


def _opt_case(name, kind, n, seed, expect, **extra):
    rs = np.random.RandomState(seed)
    scales = _scales(rs)
    return dict(name=name, kind=kind, n=n, expect=expect, scales=scales, max_norm=_unit_max_norm(np.sqrt(n)),
                p0=(rs.standard_normal(n) * 0.1).astype(np.float32),
                grads=[(rs.standard_normal(n) * s).astype(np.float32) for s in scales], **extra)


def step_cases():
    out = []
    for k, kind in enumerate(KINDS):
        for n, expect in STEP_SHAPES:
            out.append(_opt_case("%s-n%d" % (kind, n), kind, n, 1000 * (k + 1) + n, expect))
    return out


# dra_adam_step / dra_adam_step_dev: scalar grid-stride, no alignment requirement
ADAM_SHAPES = [
    (1, 0, dict(blocks=1, trips=1)),
    (3, 0, dict(blocks=1, trips=1)),
    (257, 0, dict(blocks=2, trips=1)),
    (257, 1, dict(blocks=2, trips=1)),                  # on a view offset by one float
    (524288 + 77, 0, dict(blocks=2048, trips=2)),       # a second grid-stride trip
]


def adam_cases():
    return [_opt_case("adam-n%d%s" % (n, "-offset1" if off else ""), "adam", n, 4000 + n % 1000 + off, expect, offset=off)
            for n, off, expect in ADAM_SHAPES]


# dra_grad_sqnorm: 512 x 256 x 4 floats per trip
SQNORM_SHAPES = [
    (1, dict(trips=0, tail=1)),
    (3, dict(trips=0, tail=3)),                         # tail only
    (194, dict(trips=1, tail=2)),
    (524288 + 8 + 3, dict(trips=2, tail=3)),            # a second trip plus a tail
]
SQNORM_SLABS = (0, 1, 2, 7)


def sqnorm_cases():
    out = []
    for n, expect in SQNORM_SHAPES:
        for ns in SQNORM_SLABS:
            rs = np.random.RandomState(5000 + n % 1000 + ns)
            stride = (n + 3) // 4 * 4 + 8                # larger than n, a multiple of 4; the padding is NaN
            out.append(dict(name="n%d-slabs%d" % (n, ns), n=n, n_slabs=ns, stride=stride, expect=expect,
                            grad=rs.standard_normal(n).astype(np.float32),
                            slabs=padded_slabs(rs, ns, n, stride) if ns else None))
    return out


# clip_coef_from_partials through rmsprop_step at n = 2052 (two workgroups), partials written by the test
COEF_PARTIALS = (1, 255, 256, 257, 512, 4095, 4096)
COEF_N = 2052


def coef_cases():
    out = []
    for npart in COEF_PARTIALS:
        rs = np.random.RandomState(6000 + npart)
        partials = 10.0 ** rs.uniform(-6.0, 6.0, size=npart)        # twelve orders of magnitude
        out.append(dict(name="partials%d" % npart, kind="rmsprop_centered", n=COEF_N, n_partials=npart, partials=partials,
                        sqsum=float(partials.sum()), max_norm=float(F(0.25 * np.sqrt(partials.sum()))),
                        p0=(rs.standard_normal(COEF_N) * 0.1).astype(np.float32),
                        grad=(rs.standard_normal(COEF_N) * 0.1).astype(np.float32)))
    return out


# dra_grad_sqnorm_segs: the layouts of tests/test_clip_step_emulation.py that never ran on a GPU, a padded stride, and
# the layout whose plain workgroups walk two strides
SEGS_LAYOUTS = [
    dict(name="narrow-wide-two-pass", counts=[260, 68, 1028], slabs=[5, 33, 200], tail=8, pad=0,
         expect=dict(fold_blocks=2 + 2 + 17, plain_blocks=1, plain_iters=1, partials=22)),
    dict(name="one-unit-segments", counts=[64, 4], slabs=[16, 1], tail=0, pad=0,
         expect=dict(fold_blocks=2, plain_blocks=0, plain_iters=1, partials=2)),
    dict(name="plain-only", counts=[], slabs=[], tail=5000, pad=0,
         expect=dict(fold_blocks=0, plain_blocks=2, plain_iters=1, partials=2)),
    dict(name="161-slabs", counts=[1300], slabs=[161], tail=4108, pad=0,
         expect=dict(fold_blocks=21, plain_blocks=2, plain_iters=1, partials=23)),
    dict(name="padded-stride", counts=[132, 516], slabs=[3, 40], tail=12, pad=12,
         expect=dict(fold_blocks=1 + 9, plain_blocks=1, plain_iters=1, partials=11)),
    dict(name="plain-two-strides", counts=[256000], slabs=[33], tail=97 * 4096 + 4, pad=0,
         expect=dict(fold_blocks=4000, plain_blocks=49, plain_iters=2, partials=4049)),
]


def segs_case(layout):
    """Materialises one layout (the largest holds 34 MB of slabs: built when a test asks for it, not at import)."""
    rs = np.random.RandomState(7000 + sum(layout["counts"]) % 1000 + layout["tail"] % 100)
    n = sum(layout["counts"]) + layout["tail"]
    c = dict(layout, n=n, kind="rmsprop_centered", grad=rs.standard_normal(n).astype(np.float32), seg_slabs=[], want=None,
             p0=(rs.standard_normal(n) * 0.1).astype(np.float32))
    want, off = c["grad"].copy(), 0
    for cnt, ns in zip(layout["counts"], layout["slabs"]):
        sl = padded_slabs(rs, ns, cnt, cnt + layout["pad"])
        c["seg_slabs"].append(sl)
        want[off:off + cnt] = fold_grouped(sl[:, :cnt], 16)
        off += cnt
    c["want"] = want
    c["max_norm"] = _unit_max_norm(np.sqrt(sqsum64(want)))
    return c


# dra_clip_step_late: (segment floats, slabs) x floats behind the segment x partials of earlier launches
LATE_SEGS = [(516, 1), (516, 3), (516, 64), (65536, 2), (132, 65), (132, 160)]
LATE_EXTRA = (0, 3, 3072 + 4 + 3)
LATE_PRIOR = (0, 1, 1024, 1025, "max")          # "max": 4096 - fold_blocks
LATE_FOLD_BLOCKS = {(516, 1): 3, (516, 3): 3, (516, 64): 3, (65536, 2): 256, (132, 65): 3, (132, 160): 3}
LATE_PLAIN = {0: dict(plain_blocks=0, last_plain=0, tail=0), 3: dict(plain_blocks=0, last_plain=0, tail=3),
              3079: dict(plain_blocks=2, last_plain=1, tail=3)}


def late_cases():
    """Every (segment, optimizer kind) pair once, with the floats behind the segment and the earlier partials cycling so
    that all eight instantiations (RMSprop / Adam x 4 / 16 groups x 4 / 16 earlier partials per thread), every extra and
    every n_prior occur (tests/test_optim_edge_cases_host.py asserts the coverage)."""
    out = []
    for i, (count, ns) in enumerate(LATE_SEGS):
        for k, kind in enumerate(KINDS):
            extra = LATE_EXTRA[(i + k) % 3]
            prior = LATE_PRIOR[(2 * i + 3 * k) % 5]
            fold_blocks = LATE_FOLD_BLOCKS[(count, ns)]
            n_prior = 4096 - fold_blocks if prior == "max" else prior
            n = count + extra
            rs = np.random.RandomState(8000 + 100 * i + 10 * k)
            scales = _scales(rs)
            stride = count + 4 * (i % 2)                                           # every other segment with a padded stride
            slabs = [padded_slabs(rs, ns, count, stride, s) for s in scales]       # fresh per step
            unit_prior = rs.rand(STEPS, n_prior) * (1.5 * count / max(1, n_prior))   # ~40 % of the squared norm
            expect = dict(ng=late_groups(ns), fold_blocks=fold_blocks, last_fold=1 if count != 65536 else 64, **LATE_PLAIN[extra])
            out.append(dict(name="%s-seg%dx%d-extra%d-prior%d" % (kind, count, ns, extra, n_prior), kind=kind, n=n,
                            count=count, n_slabs=ns, stride=stride, extra=extra, n_prior=n_prior, expect=expect,
                            scales=scales, max_norm=_unit_max_norm(np.sqrt(count + (1.5 * count if n_prior else 0.0))),
                            slabs=slabs, unit_prior=unit_prior, p0=(rs.standard_normal(n) * 0.1).astype(np.float32),
                            rest=[(rs.standard_normal(extra) * s).astype(np.float32) for s in scales]))
    return out


def late_step_inputs(c, k):
    """Step k of a late case: the slabs and the earlier partials at that step's gradient scale, the NG-ordered fold and the
    whole gradient after the fold (the floats behind the segment are not slabs), and the float64 squared norm."""
    s = c["scales"][k]
    slabs = c["slabs"][k]
    prior = c["unit_prior"][k] * (s * s)
    fold = fold_grouped(slabs[:, :c["count"]], late_groups(c["n_slabs"]))
    grad = np.concatenate([fold, c["rest"][k]])
    return dict(slabs=slabs, prior=prior, fold=fold, grad=grad, seg_sq=sqsum64(fold), sqsum=sqsum64(fold) + float(prior.sum()))
