"""Edge-batch cases of the Nature-CNN conv kernels (csrc/conv_v2.hip dra_conv_fwd_koc, dra_conv1_fwd_koc_ring, dra_transpose_f32;
csrc/fused.hip dra_conv_bwd_fused, dra_conv_wgrad_slabs with the roles of oneshot.h, oneshot_lin.h, dgrad_scatter.h): the case
tables, a restatement of every dispatch decision the launchers make, float64 references and the operand sets.  CPU only;
tests/test_conv_edge_cases_host.py proves the tables (each case reaches the path and share shape it is named for, together they
cover COVERAGE, the inputs carry the bar), tests/test_gpu_conv_edges.py holds the kernels to them.

The layer geometry is fixed, so a kernel is selected by batch, input type, net count nz and the variant bits alone; whatever depends
on the compute-unit count takes n_cu as an argument (the host test uses 256, the GPU test the device's own count).

Operand sets, per case:
  random   the generators of tests/test_gpu_kernels.py: weights normal / sqrt(K), biases at 0.1 scale, layer 2 / 3 inputs
           max(normal, 0), uint8 frames uniform in 0..255 with u8_coef = 1 / 255, upstream gradients normal
  integer  uint8 frames (or float inputs) in 0..3 with u8_coef = 1, weights and biases in -2..2, upstream gradients in -1..1, drawn
           independently per element (no tiled block: a swap of two samples, channels or taps changes the sums): every product and
           partial sum is an integer below 2^24 (int_bounds), so ANY correct summation order gives the integer result bit for bit.
           The integer reference is the float64 contraction, itself exact here (every partial sum is below 2^53), cast to int64.
References: float64 F.conv2d and its autograd on the float32 operand values.  The backward entry points take the gradient of the
layer's PRE-activation, so no ReLU gate lies between the upstream gradient and the reference; the input-gradient mask is
(xact > 0) of the given float32 xact, which is exact.  Forward references of large conv1 batches are computed on kept_samples.

Bar (not tuned to the kernels): BAR = 1e-5 of the reference's max-abs per output tensor, the project's contraction bar
(tests/test_gpu_kernels.py _scale_close).  BAR_OVERRIDES is where a tensor whose INPUTS cannot carry 1e-5 would get
max(1e-5, 4 x the error of the float32 CPU run of the same reference), with both figures beside it.  It is empty."""
import functools
import zlib

import numpy as np

BAR = 1e-5
# (case name, tensor key) -> (bar, error / scale of the float32 CPU run of the reference on the same inputs)
BAR_OVERRIDES = {}
F, D = np.float32, np.float64
MAX_Z = 4                                     # DRA_MAX_Z (include/deeprl_amd.h:27)
MAX_BATCH = 1025
GEOM = {1: (4, 84, 32, 8, 4), 2: (32, 20, 64, 4, 2), 3: (64, 9, 64, 3, 1)}      # C, H, OC, KH, S (ops._CONV_GEOM)
# variant bits (include/deeprl_amd.h:327-330, :356)
FUSED, ODGRAD, OWGRAD, SCATTER = 1, 2, 8, 262144
OO = ODGRAD | OWGRAD
VARIANTS = {"oo": OO, "oo-f": OO | FUSED, "oo-s": OO | SCATTER, "oo-fs": OO | FUSED | SCATTER, "fd": FUSED | ODGRAD}
KSPLIT = 16                                   # slabs of the split-K weight gradient (what nets._ConvKocFn passes)


def bar(name, key):
    return BAR_OVERRIDES.get((name, key), (BAR,))[0]


def out_hw(layer):
    c, h, oc, k, s = GEOM[layer]
    return (h - k) // s + 1


def positions(layer):
    return out_hw(layer) ** 2


def k_of(layer):
    c, h, oc, k, s = GEOM[layer]
    return c * k * k


def slab_stride(layer):
    """Floats per slab: dWt [K][OC] then db [OC], rounded up to whole float4s (ops.conv_bwd_fused)."""
    n = GEOM[layer][2] * k_of(layer) + GEOM[layer][2]
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------- dispatch, restated
TILES_PER_SAMPLE = {l: (positions(l) + 31) // 32 for l in GEOM}               # V2Geom::TPS (conv_v2.hip:40): 13, 3, 2
PTBIG = {1: 2, 2: 3, 3: 2}                                                    # conv_v2.hip:1689-1691
GROUPS_PER_SAMPLE = {l: (TILES_PER_SAMPLE[l] + PTBIG[l] - 1) // PTBIG[l] for l in GEOM}   # V2Tile::TPG (conv_v2.hip:157): 7, 1, 1
PT_BATCH, NW8_MAX_BATCH, CONV1_TP_BATCH = 128, 16, 384                        # conv_v2.hip:1644, :1638, :1656
# workgroups per CU the persistent conv1 kernel can have at most: its launch bound and its 49 KB of LDS (conv_v2.hip:1658-1660)
CONV1_PERSIST_WG_PER_CU_MAX = 3


def conv1_tp_shape(batch, nz, n_cu):
    """launch_conv1_u8_tp (conv_v2.hip:1451-1473) -> dict(per, spg, tp, n_groups, nwg, last_group_samples)."""
    per = max(1, (2 * n_cu) // nz)                                                         # :1459, :1464
    spg = 2 if batch >= 2 * per else 1                                                     # :1465
    tp = 1 if (spg == 2 or batch >= per) else (2 if 2 * batch >= per else 4)               # :1466
    n_groups = ((batch + spg - 1) // spg) * tp                                             # :1467
    return dict(per=per, spg=spg, tp=tp, n_groups=n_groups, nwg=min(n_groups, per),        # :1468
                last_group_samples=batch - spg * ((batch + spg - 1) // spg - 1))           # :1377 (ns of the last group)


def fwd_path(layer, u8, batch, nz, n_cu):
    """dra_conv_fwd_koc -> launch_conv_v2 (conv_v2.hip:1640-1674, DRA_CONV_PT_BATCH unset) ->
      ("latency eight-wave",)            :1672   batch <= 16
      ("latency four-wave",)             :1673   17 .. 127
      ("conv1-u8-tp", spg, tp)           :1656   uint8 conv1 from 384
      ("persistent conv1",)              :1660   uint8 conv1 128 .. 383
      ("persistent conv2" | "conv3",)    :1663, :1665
      ("two-tile conv1-f32",)            :1667   float conv1 from 128: `U8 || G::H <= 32` (:1651) is false for 84 x 84 float frames,
                                                 so this is the plain two-tiles-per-workgroup grid, NOT a persistent kernel"""
    if (layer != 1 and u8) or layer not in GEOM:                                           # :1690-1693
        return ("refused",)
    if batch >= PT_BATCH:                                                                  # :1646
        if layer == 1 and not u8:                                                          # :1651 -> :1667
            return ("two-tile conv1-f32",)
        if layer == 1 and batch >= CONV1_TP_BATCH:                                         # :1656
            t = conv1_tp_shape(batch, nz, n_cu)
            return ("conv1-u8-tp", t["spg"], t["tp"])
        return ("persistent conv%d" % layer,)
    if batch <= NW8_MAX_BATCH:                                                             # :1672
        return ("latency eight-wave",)
    return ("latency four-wave",)


def tp4_reachable(n_cu):
    """Is there any (batch >= 384, nz in 1..MAX_Z) that gives tp = 4?  It needs 2 * batch < per = 2 * n_cu / nz, i.e.
    n_cu > 384 * nz: never on 256 compute units."""
    return any(conv1_tp_shape(b, nz, n_cu)["tp"] == 4 for nz in range(1, MAX_Z + 1) for b in range(CONV1_TP_BATCH, 2 * n_cu + 2))


def first_sample_of_last_iteration(layer, u8, batch, nz, n_cu):
    """The first sample a workgroup touches in its LAST trip of the walk g = blockIdx.x, + gridDim.x, ... (conv_v2.hip:1376,
    :840), or `batch` where a workgroup has one tile group only.  For the persistent kernel the grid depends on the occupancy the
    runtime reports; with the largest possible grid the answer is the earliest possible sample, a superset of the real trip."""
    path = fwd_path(layer, u8, batch, nz, n_cu)
    if path[0] == "conv1-u8-tp":
        t = conv1_tp_shape(batch, nz, n_cu)
        g0 = ((t["n_groups"] - 1) // t["nwg"]) * t["nwg"]
        return (g0 // t["tp"]) * t["spg"]                                                  # :1377
    if path[0] == "persistent conv1":
        n_groups = GROUPS_PER_SAMPLE[1] * batch                                            # :1295
        per = max(1, (CONV1_PERSIST_WG_PER_CU_MAX * n_cu) // ((GEOM[1][2] // 32) * nz))    # :1305-1308
        return max(0, n_groups - min(n_groups, per)) // GROUPS_PER_SAMPLE[1]
    return batch


def kept_samples(layer, u8, batch, nz, n_cu, last_share=0):
    """Samples a large-batch forward reference is computed on: everything up to 160 samples; beyond, the first and last 40, every
    sample of the last workgroup iteration and the last `last_share` samples (a ragged last group or share)."""
    if batch <= 160:
        return np.arange(batch)
    keep = set(range(40)) | set(range(batch - 40, batch))
    keep |= set(range(first_sample_of_last_iteration(layer, u8, batch, nz, n_cu), batch))
    keep |= set(range(batch - last_share, batch))
    return np.array(sorted(keep))


# weight-gradient roles: name -> (shares, slabs per sample where there are no shares, samples per iteration)
WG_ROLES = {
    "WG1u": (0, 5, 1), "WG1f": (0, 5, 1),            # fused.hip:48-49: ConvWgradOne<G1, 4 rows ..>: NCHUNK = 20 / 4 (oneshot.h:473)
    "WG1up": (256, 0, 1), "WG1fp": (256, 0, 1),      # fused.hip:53-54
    "WG1uq": (512, 0, 1), "WG1fq": (512, 0, 1),      # fused.hip:55-56
    "WG2l": (0, 1, 1), "WG3l": (0, 1, 1),            # fused.hip:63-64, oneshot_lin.h:207
    "WG2p": (128, 0, 1), "WG3p": (85, 0, 2),         # fused.hip:67-68
}
CONV1_PERSIST_BATCH, CONV1_Q_BATCH = 128, 512        # fused.hip:57, :264
PERSIST_FROM = {2: 768, 3: 128}                      # fused.hip:76-77
ONE_LAUNCH = {2: False, 3: True}
SCATTER_FROM = 256                                   # fused.hip:73


def role_slabs(role, batch):
    """The closed forms in the headers: ConvWgradOne::n_slabs (oneshot.h:497-499), ConvWgradLin::n_slabs (oneshot_lin.h:207),
    ConvWgradPers::n_slabs (oneshot_lin.h:458-459).  -> (n_slabs, spw, samples in the last share)"""
    shares, per_sample, _ = WG_ROLES[role]
    if not shares:
        return batch * per_sample, 1, 1
    spw = (batch + shares - 1) // shares
    n = (batch + spw - 1) // spw
    return n, spw, batch - (n - 1) * spw


def wgrad_slabs(layer, batch, ksplit, variant):
    """dra_conv_wgrad_slabs (fused.hip:79-90), or None where it refuses."""
    if batch < 1 or ksplit < 1 or layer not in GEOM:                                       # :80
        return None
    if not variant & OWGRAD:                                                               # :81
        return ksplit
    if layer == 1:                                                                         # :85
        role = "WG1uq" if batch >= 512 else "WG1up" if batch >= CONV1_PERSIST_BATCH else "WG1u"
    else:                                                                                  # :82-83, :86-87
        pers = batch >= PERSIST_FROM[layer] and bool(variant & ODGRAD)
        role = "WG%d%s" % (layer, "p" if pers else "l")
    return role_slabs(role, batch)[0]


def bwd_path(layer, u8, batch, variant, ksplit=KSPLIT):
    """dra_conv_bwd_fused (fused.hip:254-294) with conv_bwd_fused_t (:180-249) and conv_bwd_scatter_t (:147-177) ->
    dict(launches: a tuple of launches, each a tuple of role names in grid order; wgrad: the weight-gradient role; n_slabs, spw,
    last_share: from the ROLE's own closed form -- the host test holds them against wgrad_slabs).  Role names:
      WG..                       the weight-gradient roles of WG_ROLES; "wgrad-igemm" the split-K GEMM (ksplit slabs)
      dgrad-lin-PTn              ConvDgradLin<G, n position tiles per workgroup> (oneshot_lin.h:38)
      dgrad-scat-NSn[-alone]     ConvDgradScat<G, n samples per workgroup[, a launch to itself]> (dgrad_scatter.h:43)
      dgrad-igemm                ConvDgradKoc, the K-chunked GEMM
    a launch is marked "tp" where it goes through launch_multi_tp (three waves per SIMD)."""
    if batch < 1 or ksplit < 1 or layer not in GEOM or (layer != 1 and u8):                # :257-258
        return None
    ow, od = bool(variant & OWGRAD), bool(variant & ODGRAD)

    def out(launches, wg):
        n, spw, last = (ksplit, None, None) if wg == "wgrad-igemm" else role_slabs(wg, batch)
        return dict(launches=tuple(launches), wgrad=wg, n_slabs=n, spw=spw, last_share=last)

    if layer == 1:                                                                         # :262-287
        if not ow:
            return out([("wgrad-igemm",)], "wgrad-igemm")                                  # :287
        t = "u" if u8 else "f"
        if batch >= CONV1_Q_BATCH:                                                         # :264
            return out([("tp", "WG1%sq" % t)], "WG1%sq" % t)
        if batch >= CONV1_PERSIST_BATCH:                                                   # :272
            return out([("tp", "WG1%sp" % t)], "WG1%sp" % t)
        return out([("WG1" + t,)], "WG1" + t)                                              # :280-285
    one, pers = "WG%dl" % layer, "WG%dp" % layer
    pt = 2 if layer == 2 else 1                                                            # DgradTiles (:102)
    if od and ow:                                                                          # :186
        if variant & SCATTER and batch >= SCATTER_FROM:                                    # :189
            ns = 2 if (layer == 3 and batch >= 512) else 1                                 # :191-194, ScatSamples (:74-75)
            scat = "dgrad-scat-NS%d" % ns
            if batch >= PERSIST_FROM[layer]:                                               # :158
                if variant & FUSED and ONE_LAUNCH[layer]:                                  # :164
                    return out([(pers, scat)], pers)
                return out([(pers,), (scat + "-alone",)], pers)                            # :165-166
            if variant & FUSED:                                                            # :174
                return out([(scat, one)], one)
            return out([("tp", one), (scat + "-alone",)], one)                             # :175-176
        if batch >= PERSIST_FROM[layer]:                                                   # :196
            if layer == 3 and batch < 512:                                                 # :202
                return out([("tp", pers, "dgrad-lin-PT1")], pers)                          # :210
            big = "dgrad-lin-PT%d" % (2 if layer == 2 else 3)                              # :212
            if not ONE_LAUNCH[layer]:                                                      # :213
                return out([(pers,), ("tp", big)], pers)                                   # :216-217
            return out([("tp", pers, big)], pers)                                          # :221
        lin = "dgrad-lin-PT%d" % pt
        if batch >= 128:                                                                   # :230
            return out([("tp", lin, one)], one)
        return out([(lin, one)], one)                                                      # :231
    if od:                                                                                 # :235-238
        return out([("dgrad-lin-PT%d" % pt, "wgrad-igemm")], "wgrad-igemm")
    if ow:                                                                                 # :242-244
        return out([("dgrad-igemm", one)], one)
    return out([("dgrad-igemm", "wgrad-igemm")], "wgrad-igemm")                            # :246-247


def dgrad_role(path):
    return next((r for l in path["launches"] for r in l if r.startswith("dgrad")), None)


# ------------------------------------------------------------------------------------------------------- case tables
def _fwd(layer, u8, batch, nz, act, n_cu):
    name = "fwd-L%d-%s-b%d%s-%s" % (layer, "u8" if u8 else "f32", batch, "-nz%d" % nz if nz > 1 else "", act or "none")
    return dict(name=name, layer=layer, u8=u8, batch=batch, nz=nz, act=act, reaches=fwd_path(layer, u8, batch, nz, n_cu))


def conv1_tp_batches(n_cu):
    """The conv1-u8-tp cases, from per = 2 * n_cu / nz: at nz = 1 per - 1, per, 2 per - 1, 2 per; at nz = 2 384 and 2 per; each
    clipped to 384 .. MAX_BATCH.  -> [(batch, nz)]"""
    clip = lambda b: max(CONV1_TP_BATCH, min(MAX_BATCH, b))
    per1, per2 = 2 * n_cu, n_cu
    out = [(clip(b), 1) for b in (per1 - 1, per1, 2 * per1 - 1, 2 * per1)] + [(CONV1_TP_BATCH, 2), (clip(2 * per2), 2)]
    return sorted(set(out))


def fwd_cases(n_cu=256):
    A = ("relu", None)
    cases = []
    for layer in (1, 2, 3):
        u8 = layer == 1
        # both sides of eight-wave | four-wave and of latency | throughput; relu and none on every path
        for b, act in ((16, "relu"), (16, None), (17, "relu"), (127, None), (128, "relu"), (131, None)):
            cases.append(_fwd(layer, u8, b, 1, act, n_cu))
        for b in (128, 131):
            for nz in (2, 3):
                cases.append(_fwd(layer, u8, b, nz, A[(nz + b) % 2], n_cu))
    # conv1 uint8: persistent | its own throughput kernel, and that kernel's (spg, tp) combinations
    cases += [_fwd(1, True, 383, 1, None, n_cu), _fwd(1, True, 384, 1, "relu", n_cu), _fwd(1, True, 1025, 1, None, n_cu)]
    seen = {}
    for b, nz in conv1_tp_batches(n_cu):                 # relu and none alternate within each (spg, tp)
        shape = fwd_path(1, True, b, nz, n_cu)
        seen[shape] = seen.get(shape, 0) + 1
        cases.append(_fwd(1, True, b, nz, A[seen[shape] % 2], n_cu))
    # conv1 on float frames
    cases += [_fwd(1, False, 17, 1, None, n_cu), _fwd(1, False, 127, 1, "relu", n_cu), _fwd(1, False, 128, 1, None, n_cu),
              _fwd(1, False, 131, 1, "relu", n_cu), _fwd(1, False, 384, 1, "relu", n_cu), _fwd(1, False, 1025, 1, None, n_cu)]
    seen, out = set(), []
    for c in cases:
        if c["name"] not in seen:
            seen.add(c["name"])
            out.append(c)
    return out


def _bwd(layer, u8, batch, vname):
    name = "bwd-L%d-%s-b%d-%s" % (layer, "u8" if u8 else "f32", batch, vname)
    return dict(name=name, layer=layer, u8=u8, batch=batch, vname=vname, variant=VARIANTS[vname],
                reaches=bwd_path(layer, u8, batch, VARIANTS[vname]))


BWD_CASES = (
    # conv1: slabs per chunk | 256 shares | 512 shares; spw stepping at 257 and 513; float frames on every role
    [_bwd(1, True, b, "oo") for b in (127, 128, 257, 511, 512, 513)] + [_bwd(1, False, b, "oo") for b in (127, 128, 257, 512)] +
    # conv2: three waves per SIMD from 128; the scatter form from 256 (one launch and two); persistent weight gradient from 768
    [_bwd(2, False, b, "oo") for b in (127, 128)] +
    [_bwd(2, False, 255, "oo-fs"), _bwd(2, False, 256, "oo"), _bwd(2, False, 256, "oo-s"), _bwd(2, False, 256, "oo-fs")] +
    [_bwd(2, False, 767, "oo"), _bwd(2, False, 767, "oo-fs"), _bwd(2, False, 768, "oo"), _bwd(2, False, 768, "oo-s"),
     _bwd(2, False, 768, "oo-fs"), _bwd(2, False, 769, "oo")] +
    # conv3: persistent weight gradient from 128 (85 shares, two samples per iteration: spw 2 -> 3 at 171); scatter from 256;
    # one -> three position tiles (no scatter) and one -> two samples (scatter) per workgroup at 512
    [_bwd(3, False, b, "oo") for b in (127, 128, 170, 171)] +
    [_bwd(3, False, 255, "oo-fs"), _bwd(3, False, 256, "oo"), _bwd(3, False, 256, "oo-s"), _bwd(3, False, 256, "oo-fs")] +
    [_bwd(3, False, 511, "oo"), _bwd(3, False, 511, "oo-fs"), _bwd(3, False, 512, "oo"), _bwd(3, False, 512, "oo-s"),
     _bwd(3, False, 512, "oo-fs")] +
    # above nets._ONESHOT_WGRAD_MAX_BATCH: split-K weight gradient beside the one-pass input gradient
    [_bwd(2, False, 1025, "fd"), _bwd(3, False, 1025, "fd")]
)

# what bwd_path gives at the batches the issue works out: name -> (weight-gradient role, n_slabs, spw, last share)
BWD_SHARES = {
    "bwd-L1-u8-b127-oo": ("WG1u", 635, 1, 1), "bwd-L1-u8-b128-oo": ("WG1up", 128, 1, 1), "bwd-L1-u8-b257-oo": ("WG1up", 129, 2, 1),
    "bwd-L1-u8-b511-oo": ("WG1up", 256, 2, 1), "bwd-L1-u8-b512-oo": ("WG1uq", 512, 1, 1), "bwd-L1-u8-b513-oo": ("WG1uq", 257, 2, 1),
    "bwd-L1-f32-b127-oo": ("WG1f", 635, 1, 1), "bwd-L1-f32-b128-oo": ("WG1fp", 128, 1, 1), "bwd-L1-f32-b257-oo": ("WG1fp", 129, 2, 1),
    "bwd-L1-f32-b512-oo": ("WG1fq", 512, 1, 1),
    "bwd-L2-f32-b767-oo": ("WG2l", 767, 1, 1), "bwd-L2-f32-b768-oo": ("WG2p", 128, 6, 6), "bwd-L2-f32-b769-oo": ("WG2p", 110, 7, 6),
    "bwd-L3-f32-b127-oo": ("WG3l", 127, 1, 1), "bwd-L3-f32-b128-oo": ("WG3p", 64, 2, 2), "bwd-L3-f32-b170-oo": ("WG3p", 85, 2, 2),
    "bwd-L3-f32-b171-oo": ("WG3p", 57, 3, 3), "bwd-L3-f32-b511-oo": ("WG3p", 73, 7, 7), "bwd-L3-f32-b512-oo": ("WG3p", 74, 7, 1),
    "bwd-L2-f32-b1025-fd": ("wgrad-igemm", 16, None, None), "bwd-L3-f32-b1025-fd": ("wgrad-igemm", 16, None, None),
}

# batch independence: the smallest batch that reaches each forward path (generated per n_cu) and each input-gradient form
BWD_INDEPENDENCE = [(3, 3, OO, "dgrad-lin-PT1"), (2, 3, OO, "dgrad-lin-PT2"), (3, 512, OO, "dgrad-lin-PT3"),
                    (2, 256, OO | FUSED | SCATTER, "dgrad-scat-NS1"), (2, 256, OO | SCATTER, "dgrad-scat-NS1-alone"),
                    (3, 256, OO | FUSED | SCATTER, "dgrad-scat-NS1"), (3, 512, OO | FUSED | SCATTER, "dgrad-scat-NS2"),
                    (3, 512, OO | SCATTER, "dgrad-scat-NS2-alone"), (3, 3, FUSED, "dgrad-igemm"), (2, 3, FUSED, "dgrad-igemm")]


def fwd_independence(n_cu=256):
    """(layer, u8, batch, nz): the smallest batch that reaches each forward path."""
    out = [(l, l == 1, b, 1) for l in (1, 2, 3) for b in (2, 17, 128)] + [(1, False, 128, 1)]
    shapes = {}
    for b in range(CONV1_TP_BATCH, MAX_BATCH + 1):
        shapes.setdefault(fwd_path(1, True, b, 1, n_cu), b)
    return out + [(1, True, b, 1) for b in sorted(shapes.values())]


RING_CAPACITY = 7
RING_CASES = [(newest, age) for newest in (0, 2, 6) for age in (None, 3, 1, 0)]
TRANSPOSE_SHAPES = [(1, 1), (1, 513), (513, 1), (31, 33), (3136, 512)]
# u8 against float conv1, and the batches whose prefix / suffix is held against the four-wave latency shape
U8_F32_BATCHES = (17, 128, 384, 1025)
PREFIX_CASES = [(1, True, 128), (1, False, 128), (2, False, 128), (3, False, 128), (1, True, 383), (1, True, 384), (1, True, 1025)]


def ring_stack_slots(newest, age, capacity=RING_CAPACITY, channels=4):
    """conv_v2.hip:368-371: channel c is the frame min(C - 1 - c, age) slots back from the newest one, wrapping below slot 0;
    a null stack_age is C - 1 (:341)."""
    age = channels - 1 if age is None else age
    return [(newest - min(channels - 1 - c, age)) % capacity for c in range(channels)]


def _fwd_any(cases, pred):
    return any(pred(c, c["reaches"]) for c in cases)


def coverage(cases=None, n_cu=256):
    """name -> predicate over the tables: what they must reach, taken together."""
    cases = fwd_cases(n_cu) if cases is None else cases
    fa = lambda pred: (lambda: _fwd_any(cases, pred))
    ba = lambda pred: (lambda: any(pred(c, c["reaches"]) for c in BWD_CASES))
    cov = {}
    for l in (1, 2, 3):
        u8 = l == 1
        for b, p in ((16, "latency eight-wave"), (17, "latency four-wave"), (127, "latency four-wave")):
            cov["fwd conv%d batch %d: %s" % (l, b, p)] = fa(lambda c, r, l=l, b=b, p=p: (c["layer"], c["batch"], c["u8"]) == (l, b, l == 1) and r == (p,))
        cov["fwd conv%d batch 128: persistent" % l] = fa(lambda c, r, l=l: (c["layer"], c["batch"], c["nz"], c["u8"]) == (l, 128, 1, l == 1) and
                                                          r == ("persistent conv%d" % l,))
        cov["fwd conv%d batch 131, one net (what the nz cases are held against)" % l] = fa(
            lambda c, r, l=l: (c["layer"], c["batch"], c["nz"], c["u8"]) == (l, 131, 1, l == 1) and r == ("persistent conv%d" % l,))
        for b in (128, 131):
            for nz in (2, 3):
                cov["fwd conv%d batch %d, nz %d" % (l, b, nz)] = fa(lambda c, r, l=l, b=b, nz=nz: (c["layer"], c["batch"], c["nz"]) == (l, b, nz) and
                                                                    r == ("persistent conv%d" % l,))
        for p in ("latency eight-wave", "latency four-wave", "persistent conv%d" % l):
            for a in ("relu", None):
                cov["fwd conv%d %s, act %s" % (l, p, a)] = fa(lambda c, r, l=l, p=p, a=a: c["layer"] == l and c["u8"] == (l == 1) and r == (p,) and c["act"] == a)
    cov["fwd conv1 u8 batch 383: persistent"] = fa(lambda c, r: c["u8"] and c["batch"] == 383 and r == ("persistent conv1",))
    cov["fwd conv1 u8 batch 384: its own throughput kernel"] = fa(lambda c, r: c["u8"] and c["batch"] == 384 and c["nz"] == 1 and r[0] == "conv1-u8-tp")
    for spg, tp, what in ((1, 2, "tp = 2"), (1, 1, "tp = 1, spg = 1"), (2, 1, "spg = 2")):
        cov["fwd conv1-u8-tp %s" % what] = fa(lambda c, r, spg=spg, tp=tp: r == ("conv1-u8-tp", spg, tp) and c["nz"] == 1)
        cov["fwd conv1-u8-tp %s, act none" % what] = fa(lambda c, r, spg=spg, tp=tp: r == ("conv1-u8-tp", spg, tp) and c["act"] is None)
    cov["fwd conv1-u8-tp spg = 2, even batch"] = fa(lambda c, r: r == ("conv1-u8-tp", 2, 1) and c["batch"] % 2 == 0 and c["nz"] == 1)
    cov["fwd conv1-u8-tp spg = 2, last group of one sample"] = fa(lambda c, r: r == ("conv1-u8-tp", 2, 1) and c["batch"] % 2 == 1)
    cov["fwd conv1-u8-tp spg = 1, nz 2"] = fa(lambda c, r: r == ("conv1-u8-tp", 1, 1) and c["nz"] == 2)
    cov["fwd conv1-u8-tp spg = 2, nz 2"] = fa(lambda c, r: r == ("conv1-u8-tp", 2, 1) and c["nz"] == 2)
    cov["fwd conv1-u8-tp one below and at per, one below and at 2 per"] = lambda: all(
        any(c["u8"] and c["layer"] == 1 and (c["batch"], c["nz"]) == bz for c in cases) for bz in conv1_tp_batches(n_cu))
    for b in (128, 131, 384, 1025):
        cov["fwd conv1 f32 batch %d" % b] = fa(lambda c, r, b=b: not c["u8"] and c["layer"] == 1 and c["batch"] == b and r == ("two-tile conv1-f32",))
    cov["fwd conv1 f32 batch 127 | 128"] = fa(lambda c, r: not c["u8"] and c["layer"] == 1 and c["batch"] == 127 and r == ("latency four-wave",))
    cov["fwd conv1 f32 two-tile, act none"] = fa(lambda c, r: r == ("two-tile conv1-f32",) and c["act"] is None)
    cov["fwd conv1 f32 two-tile, act relu"] = fa(lambda c, r: r == ("two-tile conv1-f32",) and c["act"] == "relu")
    for b in U8_F32_BATCHES:
        cov["fwd conv1 u8 and f32 at %d" % b] = lambda b=b: {c["u8"] for c in cases if c["layer"] == 1 and c["batch"] == b and c["nz"] == 1} == {True, False}
    # backward
    for t, u8, batches in (("u8", True, ((127, ""), (128, "p"), (511, "p"), (512, "q"))), ("f32", False, ((127, ""), (128, "p"), (257, "p"), (512, "q")))):
        for b, suffix in batches:
            role = "WG1" + t[0] + suffix
            cov["bwd conv1 %s batch %d: %s" % (t, b, role)] = ba(lambda c, r, role=role, u8=u8, b=b: c["layer"] == 1 and c["u8"] == u8 and c["batch"] == b and
                                                                  r["wgrad"] == role)
    cov["bwd conv1 u8 257: 129 slabs, last share of one"] = ba(lambda c, r: c["layer"] == 1 and c["u8"] and c["batch"] == 257 and(r["n_slabs"], r["spw"], r["last_share"]) == (129, 2, 1))
    cov["bwd conv1 513: 257 slabs"] = ba(lambda c, r: c["layer"] == 1 and c["batch"] == 513 and (r["n_slabs"], r["spw"], r["last_share"]) == (257, 2, 1))
    for b, role in ((767, "WG2l"), (768, "WG2p"), (769, "WG2p")):
        cov["bwd conv2 batch %d: %s, two launches" % (b, role)] = ba(lambda c, r, b=b, role=role: c["layer"] == 2 and c["batch"] == b and c["vname"] == "oo" and r["wgrad"] == role)
    cov["bwd conv2 769: spw 7, 110 slabs, last share of 6"] = ba(lambda c, r: c["layer"] == 2 and c["batch"] == 769 and (r["n_slabs"], r["spw"], r["last_share"]) == (110, 7, 6))
    for b in (767, 768):
        cov["bwd conv2 batch %d with the scatter bit, one launch asked" % b] = ba(lambda c, r, b=b: c["layer"] == 2 and c["batch"] == b and c["vname"] == "oo-fs")
    cov["bwd conv2 persistent + scatter without FUSED_BWD"] = ba(lambda c, r: c["layer"] == 2 and c["batch"] == 768 and c["vname"] == "oo-s")
    for b, role in ((127, "WG3l"), (128, "WG3p")):
        cov["bwd conv3 batch %d: %s" % (b, role)] = ba(lambda c, r, b=b, role=role: c["layer"] == 3 and c["batch"] == b and r["wgrad"] == role)
    cov["bwd conv3 170: spw 2"] = ba(lambda c, r: c["layer"] == 3 and c["batch"] == 170 and (r["n_slabs"], r["spw"], r["last_share"]) == (85, 2, 2))
    cov["bwd conv3 171: spw 3, an odd share walked two samples at a time"] = ba(lambda c, r: c["layer"] == 3 and c["batch"] == 171 and (r["n_slabs"], r["spw"], r["last_share"]) == (57, 3, 3))
    cov["bwd conv3 511 without scatter: one position tile"] = ba(lambda c, r: c["layer"] == 3 and c["batch"] == 511 and dgrad_role(r) == "dgrad-lin-PT1" and r["wgrad"] == "WG3p")
    cov["bwd conv3 512 without scatter: three position tiles"] = ba(lambda c, r: c["layer"] == 3 and c["batch"] == 512 and dgrad_role(r) == "dgrad-lin-PT3")
    cov["bwd conv3 511 | 512 with scatter: one | two samples"] = lambda: {dgrad_role(c["reaches"]) for c in BWD_CASES if c["layer"] == 3 and c["batch"] in (511, 512) and
                                                                           c["vname"] == "oo-fs"} == {"dgrad-scat-NS1", "dgrad-scat-NS2"}
    for l in (2, 3):
        cov["bwd conv%d 255 with the scatter bit: the gather form" % l] = ba(lambda c, r, l=l: c["layer"] == l and c["batch"] == 255 and c["variant"] & SCATTER and
                                                                             dgrad_role(r).startswith("dgrad-lin"))
        cov["bwd conv%d 256 scatter, one launch" % l] = ba(lambda c, r, l=l: c["layer"] == l and c["batch"] == 256 and c["vname"] == "oo-fs" and len(r["launches"]) == 1 and
                                                           dgrad_role(r) == "dgrad-scat-NS1")
        cov["bwd conv%d 256 scatter, two launches" % l] = ba(lambda c, r, l=l: c["layer"] == l and c["batch"] == 256 and c["vname"] == "oo-s" and len(r["launches"]) == 2 and
                                                             dgrad_role(r) == "dgrad-scat-NS1-alone")
        cov["bwd conv%d one-pass pair without scatter at >= 128" % l] = ba(lambda c, r, l=l: c["layer"] == l and c["batch"] == 256 and c["vname"] == "oo")
        cov["bwd conv%d FUSED_BWD | ONESHOT_DGRAD at 1025" % l] = ba(lambda c, r, l=l: c["layer"] == l and c["batch"] == 1025 and c["vname"] == "fd" and
                                                                     r["wgrad"] == "wgrad-igemm" and dgrad_role(r).startswith("dgrad-lin"))
    cov["bwd conv2 127 | 128: three waves per SIMD"] = lambda: [c["reaches"]["launches"][0][0] == "tp" for c in BWD_CASES if c["layer"] == 2 and c["batch"] in (127, 128)] == [False, True]
    cov["bwd conv3 persistent + two-sample scatter, one launch and two"] = lambda: {len(c["reaches"]["launches"]) for c in BWD_CASES if c["layer"] == 3 and c["batch"] == 512 and
                                                                                    c["variant"] & SCATTER} == {1, 2}
    return cov


# ------------------------------------------------------------------------------------------------ operands, references
def _rs(*key):
    return np.random.RandomState(zlib.crc32(("/".join(str(k) for k in key)).encode()) & 0x7FFFFFFF)


def normalize(x_u8, coef):
    """f32(f64(v) * coef): the kernels' normalisation table (conv_v2.hip:381, :1372)."""
    return (x_u8.astype(D) * coef).astype(F)


def draw_weights(rs, layer, kind):
    c, h, oc, k, s = GEOM[layer]
    if kind == "integer":
        return rs.randint(-2, 3, size=(oc, c, k, k)).astype(F), rs.randint(-2, 3, size=oc).astype(F)
    return (rs.standard_normal((oc, c, k, k)) / np.sqrt(c * k * k)).astype(F), (rs.standard_normal(oc) * 0.1).astype(F)


def draw_input(rs, layer, batch, kind):
    """-> (uint8 frames or None, float32 input, u8_coef).  Layer 1 draws uint8 frames; its float cases run on their normalised values."""
    c, h, oc, k, s = GEOM[layer]
    if layer == 1:
        x8 = rs.randint(0, 4 if kind == "integer" else 256, size=(batch, c, h, h)).astype(np.uint8)
        coef = 1.0 if kind == "integer" else 1.0 / 255
        return x8, normalize(x8, coef), coef
    if kind == "integer":
        return None, rs.randint(0, 4, size=(batch, c, h, h)).astype(F), 1.0
    return None, np.maximum(rs.standard_normal((batch, c, h, h)), 0).astype(F), 1.0


def to_koc(w):
    """[OC, C, KH, KW] -> [K = (c, kh, kw)][OC] (ops.to_koc)."""
    return np.ascontiguousarray(w.transpose(1, 2, 3, 0)).reshape(-1, w.shape[0])


def from_koc(wt, layer):
    c, h, oc, k, s = GEOM[layer]
    return np.ascontiguousarray(wt.reshape(c, k, k, oc).transpose(3, 0, 1, 2))


def act64(v, act):
    return np.maximum(v, 0.0) if act == "relu" else v


def conv_ref(x, w, b, layer, dtype=D):
    """F.conv2d in `dtype` on the float32 operand values -> numpy pre-activations."""
    import torch
    import torch.nn.functional as TF
    dt = torch.float64 if dtype == D else torch.float32
    with torch.no_grad():
        return TF.conv2d(torch.tensor(x, dtype=dt), torch.tensor(w, dtype=dt), torch.tensor(b, dtype=dt), stride=GEOM[layer][4]).numpy()


@functools.lru_cache(maxsize=2)
def fwd_operands(layer, batch, nz, kind, n_cu=256):
    """Operands and references of a forward case; the uint8 and float conv1 cases of a batch share them (same seed).
    -> dict(x8: nz uint8 arrays or None, x: nz float32 arrays, coef, w, b: nz arrays, keep: indices (the union of what the uint8
    and the float case keep), pre: nz float64 pre-activations of the kept samples)"""
    rs = _rs("fwd", layer, batch, nz, kind)
    ws, bs, x8s, xs, pres = [], [], [], [], []
    keep = kept_samples(layer, layer == 1, batch, nz, n_cu)
    coef = 1.0
    for z in range(nz):
        w, b = draw_weights(rs, layer, kind)
        x8, x, coef = draw_input(rs, layer, batch, kind)
        ws.append(w), bs.append(b), x8s.append(x8), xs.append(x)
        pres.append(conv_ref(x[keep], w, b, layer))
    return dict(x8=x8s if layer == 1 else None, x=xs, coef=coef, w=ws, b=bs, keep=keep, pre=pres)


@functools.lru_cache(maxsize=2)
def bwd_operands(layer, batch, kind):
    """Operands and float64 autograd references of a backward case (every variant and input type of a (layer, batch) shares them).
    dy is the gradient of the layer's pre-activation.  -> dict(x8, x, coef, w, dy, dw [OC, C, KH, KW], db, dx (layers 2, 3:
    unmasked; the masked one is dx * (x > 0)))"""
    import torch
    import torch.nn.functional as TF
    rs = _rs("bwd", layer, batch, kind)
    c, h, oc, k, s = GEOM[layer]
    w, _ = draw_weights(rs, layer, kind)
    x8, x, coef = draw_input(rs, layer, batch, kind)
    o = out_hw(layer)
    dy = rs.randint(-1, 2, size=(batch, oc, o, o)).astype(F) if kind == "integer" else rs.standard_normal((batch, oc, o, o)).astype(F)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=layer > 1)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(oc, dtype=torch.float64, requires_grad=True)
    TF.conv2d(xt, wt, bt, stride=s).backward(torch.tensor(dy, dtype=torch.float64))
    return dict(x8=x8, x=x, coef=coef, w=w, dy=dy, dw=wt.grad.numpy(), db=bt.grad.numpy(), dx=xt.grad.numpy() if layer > 1 else None)


def int_bounds(layer, batch):
    """Largest |partial sum| any summation order can meet on the integer set (inputs <= 3, weights and biases <= 2 in magnitude,
    gradients <= 1): forward K terms of 6 and the bias; weight gradient batch x positions terms of 3; bias gradient batch x
    positions terms of 1; input gradient at most OC x taps terms of 2; the slab fold adds nothing the weight gradient has not.
    All must stay below 2^24."""
    c, h, oc, k, s = GEOM[layer]
    return dict(fwd=6 * k_of(layer) + 2, dw=3 * batch * positions(layer), db=batch * positions(layer), dx=2 * oc * k * k,
                fold=3 * batch * positions(layer))
