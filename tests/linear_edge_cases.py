"""Edge-shape cases of the generic linear-layer kernels behind nets.linear (csrc/igemm.hip dra_linear_fwd, dra_linear_fwd_slabs,
dra_linear_bwd_w, dra_linear_bwd_x, dra_act_bwd; csrc/fused.hip dra_linear_fwd_slabs_one, dra_linear_bwd_xw_one512): the case
tables, a restatement of every dispatch decision the launchers make, float64 references and the operand sets.  CPU only;
tests/test_linear_edge_cases_host.py proves the tables (each case reaches the path it is named for, together they cover COVERAGE,
the inputs carry the bar), tests/test_gpu_linear_edges.py holds the kernels to them.

Operand sets, per case:
  random   standard normals, W scaled by 1 / sqrt(K), biases at 0.1 scale
  integer  values in [-4, 4]: every product and every partial sum is an integer below 2^24 (int_bound), so ANY correct summation
           order gives the int64 result bit for bit -- an index or ownership error shows whatever the tolerance.  act = None only.
References: every contraction in float64 from the float32 operand values, activations applied in float64; the input-gradient
mask from the given xact ((xact > 0) for ReLU, 1 - xact^2 for tanh).

Bar (not tuned to the kernels): BAR = 1e-5 of the reference's max-abs per output tensor, the project's contraction bar
(tests/test_gpu_kernels.py _scale_close).  BAR_OVERRIDES is where a tensor whose INPUTS cannot carry 1e-5 would get
max(1e-5, 4 x the error of the float32 CPU run of the same reference), with both figures beside it.  It is empty: the float32
CPU run of every random-operand case stays within the bar (the host test measures it: the largest figure is 1.9e-6, the float32
tanh of fwd-33x3136x512-w-off)."""
import functools
import zlib

import numpy as np

BAR = 1e-5
# (case name, tensor key) -> (bar, error / scale of the float32 CPU run of the reference on the same inputs)
BAR_OVERRIDES = {}
F, D = np.float32, np.float64
ACTS = (None, "relu", "tanh")
MAX_Z = 4                       # kMaxZ (csrc/igemm.h:42)
ACT_BWD_STRIDE = 2048 * 256     # dra_act_bwd's grid: at most 2048 workgroups of 256 (csrc/igemm.hip:688-689)


def bar(name, key):
    return BAR_OVERRIDES.get((name, key), (BAR,))[0]


# ------------------------------------------------------------------------------------------------- dispatch, restated
def fwd_path(B, K, O, nz, aligned, workspace_floats, x_aligned=None):
    """dra_linear_fwd's choice of kernel (csrc/igemm.hip:547-637).  aligned: every x[z] and w[z] on a 16-byte boundary
    (x_aligned: the x pointers alone, where they differ -- the gemv staging looks at x only); workspace_floats None: a null
    workspace.  ->
      ("gemv", KV, vector_staging, row_blocks, last_block_rows)   igemm.hip:553-567, staging branch igemm.hip:158
      ("rows", R)                                                 igemm.hip:569-584
      ("slabs_one", 8)                                            igemm.hip:586-607
      ("igemm", ksplit)                                           igemm.hip:609-636"""
    x_aligned = aligned if x_aligned is None else x_aligned
    if K <= 512 and B <= 128 and B * O <= 65536:                                    # :553
        kv = (K + 63) // 64                                                         # :561
        KV = 1 if kv <= 1 else 2 if kv <= 2 else 4 if kv <= 4 else 8                # :562-565
        # the staging source of row block z is x + 32 z K floats: with K % 4 == 0 every block has the alignment of x (:157-158)
        vector = K % 4 == 0 and x_aligned
        blocks = (B + 31) // 32                                                     # :559
        return ("gemv", KV, vector, blocks, B - 32 * (blocks - 1))
    if 512 < K <= 4096 and K % 4 == 0 and B <= 32 and aligned:                      # :569, :575-577
        rq = ((((K >> 2) + 3) >> 2) + 63) // 64                                     # :578
        return ("rows", 2 if rq <= 2 else 4)                                        # :582-583
    if (K == 3136 and 32 < B <= 4096 and workspace_floats is not None and nz * 8 * B * O <= workspace_floats
            and aligned):                                                           # :586-587, :596-598
        return ("slabs_one", 8)
    tiles = ((O + 31) // 32) * ((B + 31) // 32) * nz                                # :616
    chunks = (K + 63) // 64                                                         # :617
    ksplit = 1
    if tiles < 128 and chunks >= 16:                                                # :619
        ksplit = min((256 + tiles - 1) // tiles, chunks // 2, 32)                   # :620-622
        while ksplit > 1 and nz * ksplit * B * O > (workspace_floats or 0):         # :623
            ksplit -= 1
        if workspace_floats is None:                                                # :624
            ksplit = 1
    while ksplit > 1 and (ksplit - 1) * ((chunks + ksplit - 1) // ksplit) >= chunks:   # :627
        ksplit -= 1
    return ("igemm", ksplit)


def fwd_limits(B, K, O, nz, aligned, workspace_floats):
    """What igemm's split count was before each of its three limits (the coverage list asks which one bit):
    -> (wanted, after the workspace, after the shrink loop); (1, 1, 1) where the layer is not split at all."""
    tiles = ((O + 31) // 32) * ((B + 31) // 32) * nz
    chunks = (K + 63) // 64
    if not (tiles < 128 and chunks >= 16):
        return (1, 1, 1)
    wanted = ks = min((256 + tiles - 1) // tiles, chunks // 2, 32)
    while ks > 1 and nz * ks * B * O > (workspace_floats or 0):
        ks -= 1
    if workspace_floats is None:
        ks = 1
    return (wanted, ks, fwd_path(B, K, O, nz, aligned, workspace_floats)[1])


def workspace_written(path, B, O, nz):
    """Floats of the workspace a forward call writes (every slab element is written: igemm.hip:626)."""
    if path[0] == "slabs_one":
        return nz * 8 * B * O
    if path[0] == "igemm" and path[1] > 1:
        return nz * path[1] * B * O
    return 0


def bwd_w_path(B, I, O):
    """dra_linear_bwd_w (csrc/igemm.hip:653-665): the tile shape changes at out_features >= 64 (:657); the bias rides as column I
    of an I + 1 wide problem (igemm.h:513-535).  -> ("wgrad", tile width BM = BN, BK, where column I sits in its tile: "last" |
    "first" | "inside", chunks of the reduction over the batch)."""
    bn, bk = (64, 32) if O >= 64 else (32, 64)
    slot = "last" if I % bn == bn - 1 else "first" if I % bn == 0 else "inside"
    return ("wgrad", bn, bk, slot, (B + bk - 1) // bk)


def bwd_x_path(B, I, O):
    """dra_linear_bwd_x (csrc/igemm.hip:667-675): out_features == 512 and in_features >= 1024 go to the one-pass role
    LinDgradOne<512> (:670, oneshot.h:269-349; 32-wide column tiles, the last one partial when I % 32 != 0), everything else to
    LinDgrad<32, 32, 64>.  -> ("one512", I % 32 != 0) | ("igemm",)"""
    if O == 512 and I >= 1024:
        return ("one512", I % 32 != 0)
    return ("igemm",)


def slabs_one_accepts(K, ksplit, aligned):
    """dra_linear_fwd_slabs_one's own conditions (csrc/fused.hip:654-659)."""
    return K == 3136 and ksplit in (8, 14, 28) and aligned


def xw_one512_accepts(I):
    """dra_linear_bwd_xw_one512 (csrc/fused.hip:638)."""
    return I >= 1024


# ------------------------------------------------------------------------------------------------------- case tables
def _fwd(B, K, O, act, reaches, nz=1, off=(), ws="default", null_bias=(), tag=""):
    """off: operands ("x", "w") one float off a 16-byte boundary; ws: "default" = nz * 32 * B * O floats (what ops.linear_fwd
    asks for: never the limit), an int = that many floats, "null" = a null pointer with the default count beside it;
    null_bias: the z whose bias pointer is null, or "array" for a null bias array."""
    name = "fwd-%dx%dx%d%s%s" % (B, K, O, "-nz%d" % nz if nz > 1 else "", "-" + tag if tag else "")
    default = nz * 32 * B * O
    return dict(name=name, B=B, K=K, O=O, nz=nz, act=act, off=tuple(off), ws_null=ws == "null",
                ws_floats=default if ws in ("default", "null") else int(ws), null_bias=null_bias, reaches=reaches)


FWD_CASES = [
    # gemv: KV from ceil(K / 64); float4 staging when K % 4 == 0 and x is aligned; 32 rows per z-block, rounds of 8
    _fwd(1, 1, 1, None, ("gemv", 1, False, 1, 1)),
    _fwd(1, 64, 5, "relu", ("gemv", 1, True, 1, 1)),
    _fwd(1, 4, 65536, "tanh", ("gemv", 1, True, 1, 1)),              # B * O at the limit itself
    _fwd(9, 65, 3, "tanh", ("gemv", 2, False, 1, 9)),
    _fwd(33, 128, 7, None, ("gemv", 2, True, 2, 1)),
    _fwd(5, 100, 6, "relu", ("gemv", 2, True, 1, 5), nz=4, null_bias=(2,)),
    _fwd(40, 129, 6, None, ("gemv", 4, False, 2, 8)),
    _fwd(128, 256, 2, "relu", ("gemv", 4, True, 4, 32)),
    _fwd(67, 192, 3, "tanh", ("gemv", 4, True, 3, 3)),
    _fwd(31, 257, 4, "relu", ("gemv", 8, False, 1, 31)),
    _fwd(128, 512, 512, "tanh", ("gemv", 8, True, 4, 32)),
    _fwd(3, 260, 5, None, ("gemv", 8, False, 1, 3), off=("x",), tag="x-off"),
    # one step beyond each gemv limit: the K-chunked GEMM in a single launch
    _fwd(129, 256, 2, "relu", ("igemm", 1)),
    _fwd(128, 512, 513, None, ("igemm", 1)),
    _fwd(1, 4, 65537, None, ("igemm", 1)),
    _fwd(5, 513, 6, "tanh", ("igemm", 1), null_bias="array"),
    _fwd(5, 958, 6, "relu", ("igemm", 1)),                           # 15 chunks: one below the split threshold
    # rows: R = 2 up to K = 2048, 4 above; two output rows per workgroup, eight samples per round
    _fwd(32, 516, 3, "relu", ("rows", 2)),
    _fwd(9, 1000, 4, "tanh", ("rows", 2)),
    _fwd(7, 2048, 5, None, ("rows", 2)),
    _fwd(7, 2052, 5, "relu", ("rows", 4)),
    _fwd(32, 4096, 3, "tanh", ("rows", 4)),
    _fwd(1, 3136, 2, None, ("rows", 4)),
    _fwd(5, 1024, 6, "relu", ("rows", 2), nz=2),
    # the rows path refused: split-K GEMM + linear_finish_kernel
    _fwd(5, 1024, 6, None, ("igemm", 8), off=("x",), tag="x-off"),
    _fwd(5, 1022, 6, "tanh", ("igemm", 8)),                          # 16 chunks, the last one partial
    _fwd(5, 1030, 9, "relu", ("igemm", 6)),                          # 17 chunks: 8 -> 6
    _fwd(3, 4100, 4, None, ("igemm", 22)),                           # 65 chunks: 32 -> 22
    _fwd(33, 1092, 6, "tanh", ("igemm", 9)),
    _fwd(33, 2000, 6, "relu", ("igemm", 5), ws=5 * 33 * 6, tag="ws5"),
    _fwd(33, 2000, 6, None, ("igemm", 1), ws="null", tag="ws-null"),
    # slabs: K = 3136 at 32 < B <= 4096
    _fwd(33, 3136, 512, "relu", ("slabs_one", 8)),
    _fwd(33, 3136, 40, "tanh", ("slabs_one", 8), nz=2),
    _fwd(65, 3136, 1, None, ("slabs_one", 8)),
    _fwd(32, 3136, 512, "relu", ("rows", 4)),                        # the rows-path neighbour
    _fwd(33, 3136, 512, "tanh", ("igemm", 7), off=("w",), tag="w-off"),
    _fwd(33, 3136, 8, None, ("igemm", 7), ws=8 * 33 * 8 - 1, tag="ws-1"),
]

# dra_linear_fwd_slabs (any ksplit >= 2; a split beyond the chunks writes zeros) and dra_linear_fwd_slabs_one
SLABS_CASES = [dict(name="slabs-%dx%dx%d-ks%d%s" % (B, K, O, ks, "-nz%d" % nz if nz > 1 else ""), B=B, K=K, O=O, nz=nz, ksplit=ks,
                    one_pass=False)
               for B, K, O, nz, ks in ((5, 200, 7, 1, 2), (5, 200, 7, 1, 4), (5, 200, 7, 1, 9), (33, 130, 33, 2, 3))]
SLABS_ONE_CASES = [dict(name="slabs_one-33x3136x40-nz2-ks%d" % ks, B=33, K=3136, O=40, nz=2, ksplit=ks, one_pass=True)
                   for ks in (8, 14, 28)]
# (what, K, ksplit, operand one float off)
SLABS_ONE_REFUSALS = [("in_features 3132", 3132, 8, None), ("ksplit 7", 3136, 7, None), ("x off by 4 bytes", 3136, 8, "x"),
                      ("w off by 4 bytes", 3136, 8, "w")]


def _bw(B, I, O, db=True):
    return dict(name="bwd_w-%dx%dx%d%s" % (B, I, O, "" if db else "-no-db"), B=B, I=I, O=O, db=db, reaches=bwd_w_path(B, I, O))


BWD_W_CASES = [_bw(1, 1, 1), _bw(5, 4, 63), _bw(5, 4, 64), _bw(33, 63, 64), _bw(33, 64, 64), _bw(65, 31, 3), _bw(65, 32, 3),
               _bw(32, 17, 70), _bw(64, 5, 9), _bw(65, 5, 9), _bw(33, 63, 64, db=False)]
BWD_W_REACHES = {
    "bwd_w-1x1x1": ("wgrad", 32, 64, "inside", 1), "bwd_w-5x4x63": ("wgrad", 32, 64, "inside", 1),
    "bwd_w-5x4x64": ("wgrad", 64, 32, "inside", 1), "bwd_w-33x63x64": ("wgrad", 64, 32, "last", 2),
    "bwd_w-33x64x64": ("wgrad", 64, 32, "first", 2), "bwd_w-65x31x3": ("wgrad", 32, 64, "last", 2),
    "bwd_w-65x32x3": ("wgrad", 32, 64, "first", 2), "bwd_w-32x17x70": ("wgrad", 64, 32, "inside", 1),
    "bwd_w-64x5x9": ("wgrad", 32, 64, "inside", 1), "bwd_w-65x5x9": ("wgrad", 32, 64, "inside", 2),
    "bwd_w-33x63x64-no-db": ("wgrad", 64, 32, "last", 2),
}


def _bx(B, I, O, mask, reaches):
    return dict(name="bwd_x-%dx%dx%d-%s" % (B, I, O, mask or "nomask"), B=B, I=I, O=O, mask=mask, reaches=reaches)


BWD_X_CASES = [
    _bx(1, 1, 1, None, ("igemm",)),
    _bx(33, 33, 65, None, ("igemm",)), _bx(33, 33, 65, "relu", ("igemm",)), _bx(33, 33, 65, "tanh", ("igemm",)),
    _bx(5, 1023, 512, None, ("igemm",)),                 # one input short of the one-pass role
    _bx(5, 3136, 511, "tanh", ("igemm",)),               # one output short of it
    _bx(1, 1024, 512, None, ("one512", False)),
    _bx(33, 1030, 512, "relu", ("one512", True)),
    _bx(32, 3136, 512, "tanh", ("one512", False)),
]

XW_CASES = [dict(name="xw-%dx%d-%s-%s" % (B, I, "relu" if relu else "nomask", "db" if db else "no-db"), B=B, I=I, O=512, relu=relu, db=db,
                 reaches=(bwd_x_path(B, I, 512), bwd_w_path(B, I, 512)))
            for B, I in ((1, 1024), (33, 1030)) for relu in (True, False) for db in (True, False)]

ACT_BWD_CASES = [dict(name="act_bwd-%d-%s" % (n, act or "none"), n=n, act=act, trips=(n + ACT_BWD_STRIDE - 1) // ACT_BWD_STRIDE)
                 for n in (1, ACT_BWD_STRIDE, ACT_BWD_STRIDE + 1) for act in ("relu", "tanh", None)]

# nets.linear under autograd: (B, K, O, act, x_relu); each once with contiguous .grad slots inside direct_param_grads (the
# `direct` branch; at (.., >= 1024, 512) that is linear_bwd_xw_512) and once without
AUTOGRAD_CASES = [dict(name="autograd-%dx%dx%d-%s" % (B, K, O, act or "none"), B=B, K=K, O=O, act=act, x_relu=x_relu)
                  for B, K, O, act, x_relu in ((9, 65, 3, "tanh", False), (32, 516, 3, "relu", False), (33, 3136, 512, "relu", True),
                                               (40, 129, 6, None, False))]
RELU_MARGIN = 1e-5      # autograd cases differentiate through ReLU: no float64 pre-activation this close to zero (host test)


def fwd_case_path(c):
    return fwd_path(c["B"], c["K"], c["O"], c["nz"], not c["off"], None if c["ws_null"] else c["ws_floats"],
                    x_aligned="x" not in c["off"])


# what the tables must reach, taken together: name -> predicate (tests/test_linear_edge_cases_host.py lists every item)
def _any_fwd(pred):
    return any(pred(c, c["reaches"]) for c in FWD_CASES)


COVERAGE = {
    **{"gemv KV=%d, act %s" % (kv, a): (lambda kv=kv, a=a: _any_fwd(lambda c, r: r[0] == "gemv" and r[1] == kv and c["act"] == a))
       for kv in (1, 2, 4, 8) for a in ACTS},
    **{"%s, act %s" % (p, a): (lambda p=p, a=a: _any_fwd(lambda c, r: r[0] == p and c["act"] == a))
       for p in ("rows", "slabs_one", "igemm") for a in ACTS},
    "gemv float4 staging": lambda: _any_fwd(lambda c, r: r[0] == "gemv" and r[2]),
    "gemv scalar staging, K % 4 != 0": lambda: _any_fwd(lambda c, r: r[0] == "gemv" and not r[2] and c["K"] % 4),
    "gemv scalar staging, K % 4 == 0 with x unaligned": lambda: _any_fwd(lambda c, r: r[0] == "gemv" and not r[2] and c["K"] % 4 == 0),
    "gemv partial second row block": lambda: _any_fwd(lambda c, r: r[0] == "gemv" and r[3] >= 2 and r[4] < 32),
    "gemv last round shorter than 8": lambda: _any_fwd(lambda c, r: r[0] == "gemv" and r[4] % 8 != 0),
    "gemv several z with a null bias": lambda: _any_fwd(lambda c, r: r[0] == "gemv" and c["nz"] == MAX_Z and c["null_bias"]),
    "gemv at B * O = 65536": lambda: _any_fwd(lambda c, r: r[0] == "gemv" and c["B"] * c["O"] == 65536),
    "fall-through B = 129": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and c["B"] == 129 and c["K"] <= 512),
    "fall-through B * O just beyond 65536": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and c["K"] <= 512 and c["B"] <= 128 and
                                                              c["B"] * c["O"] == 65537),
    "fall-through B = 128, O = 513": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and (c["B"], c["K"], c["O"]) == (128, 512, 513)),
    "fall-through K = 513": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and c["K"] == 513),
    "rows R=2": lambda: _any_fwd(lambda c, r: r == ("rows", 2)),
    "rows R=4": lambda: _any_fwd(lambda c, r: r == ("rows", 4)),
    **{"rows K=%d" % k: (lambda k=k: _any_fwd(lambda c, r: r[0] == "rows" and c["K"] == k)) for k in (516, 2048, 2052, 4096)},
    "rows odd O": lambda: _any_fwd(lambda c, r: r[0] == "rows" and c["O"] % 2),
    "rows nb % 8 != 0": lambda: _any_fwd(lambda c, r: r[0] == "rows" and c["B"] % 8),
    "rows several z": lambda: _any_fwd(lambda c, r: r[0] == "rows" and c["nz"] > 1),
    "rows refused: unaligned pointer": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and 512 < c["K"] <= 4096 and c["K"] % 4 == 0 and
                                                        c["B"] <= 32 and c["off"]),
    "rows refused: K % 4 != 0": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and 512 < c["K"] <= 4096 and c["K"] % 4 and c["B"] <= 32),
    "rows refused: K > 4096": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and c["K"] > 4096 and c["B"] <= 32),
    "rows refused: B = 33": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and 512 < c["K"] <= 4096 and c["K"] % 4 == 0 and c["B"] == 33 and
                                             c["K"] != 3136),
    "slabs O % 64 != 0": lambda: _any_fwd(lambda c, r: r[0] == "slabs_one" and c["O"] % 64),
    "slabs O = 1": lambda: _any_fwd(lambda c, r: r[0] == "slabs_one" and c["O"] == 1),
    "slabs batch 33": lambda: _any_fwd(lambda c, r: r[0] == "slabs_one" and c["B"] == 33),
    "slabs several z": lambda: _any_fwd(lambda c, r: r[0] == "slabs_one" and c["nz"] > 1),
    "slabs neighbour B = 32 on rows": lambda: _any_fwd(lambda c, r: r[0] == "rows" and (c["B"], c["K"]) == (32, 3136)),
    "slabs refused: unaligned pointer": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and c["K"] == 3136 and c["B"] > 32 and c["off"]),
    "slabs refused: workspace one float short": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and c["K"] == 3136 and c["B"] > 32 and
                                                                 c["ws_floats"] == c["nz"] * 8 * c["B"] * c["O"] - 1),
    "igemm ksplit 1": lambda: _any_fwd(lambda c, r: r == ("igemm", 1)),
    "igemm split, count as wanted": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and r[1] > 1 and len(set(_limits(c))) == 1),
    "igemm shrunk count": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and 1 < _limits(c)[2] < _limits(c)[1]),
    "igemm workspace-limited count": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and not c["ws_null"] and 1 < _limits(c)[1] < _limits(c)[0]),
    "igemm null workspace": lambda: _any_fwd(lambda c, r: r == ("igemm", 1) and c["ws_null"] and _limits(c)[0] > 1),
    "igemm partial last chunk under a split": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and r[1] > 1 and c["K"] % 64),
    "igemm null bias array": lambda: _any_fwd(lambda c, r: r[0] == "igemm" and c["null_bias"] == "array"),
    "slabs: more splits than chunks": lambda: any(c["ksplit"] > (c["K"] + 63) // 64 for c in SLABS_CASES),
    "slabs_one: 8, 14 and 28 slices": lambda: {c["ksplit"] for c in SLABS_ONE_CASES} == {8, 14, 28},
    "wgrad 64-wide tiles": lambda: any(c["reaches"][1] == 64 for c in BWD_W_CASES),
    "wgrad 32-wide tiles": lambda: any(c["reaches"][1] == 32 for c in BWD_W_CASES),
    "wgrad O = 63 | 64": lambda: {c["O"] for c in BWD_W_CASES if (c["B"], c["I"]) == (5, 4)} == {63, 64},
    **{"wgrad %d-wide tiles, bias column %s of a tile" % (bn, slot):
       (lambda bn=bn, slot=slot: any(c["reaches"][1] == bn and c["reaches"][3] == slot for c in BWD_W_CASES))
       for bn in (64, 32) for slot in ("last", "first")},
    "wgrad second chunk of one sample": lambda: any(c["reaches"][4] == 2 and c["B"] % c["reaches"][2] == 1 for c in BWD_W_CASES),
    "wgrad db = NULL": lambda: any(not c["db"] for c in BWD_W_CASES),
    "dgrad one-pass without an I tail": lambda: any(c["reaches"] == ("one512", False) for c in BWD_X_CASES),
    "dgrad one-pass with an I tail": lambda: any(c["reaches"] == ("one512", True) for c in BWD_X_CASES),
    "dgrad one-pass at I = 1024": lambda: any(c["reaches"][0] == "one512" and c["I"] == 1024 for c in BWD_X_CASES),
    "dgrad neighbour I = 1023": lambda: any(c["reaches"] == ("igemm",) and (c["I"], c["O"]) == (1023, 512) for c in BWD_X_CASES),
    "dgrad neighbour O = 511": lambda: any(c["reaches"] == ("igemm",) and c["I"] >= 1024 and c["O"] == 511 for c in BWD_X_CASES),
    **{"dgrad %s, mask %s" % (p, m or "none"): (lambda p=p, m=m: any(c["reaches"][0] == p and c["mask"] == m for c in BWD_X_CASES))
       for p in ("igemm", "one512") for m in ACTS},
    "xw: relu on / off x db given / NULL at both shapes": lambda: len(XW_CASES) == 8 and len({c["name"] for c in XW_CASES}) == 8,
    "act_bwd second grid-stride trip": lambda: {c["trips"] for c in ACT_BWD_CASES} == {1, 2},
    "autograd one-launch pair": lambda: any(c["O"] == 512 and c["K"] >= 1024 and c["x_relu"] for c in AUTOGRAD_CASES),
}


def _limits(c):
    return fwd_limits(c["B"], c["K"], c["O"], c["nz"], not c["off"], None if c["ws_null"] else c["ws_floats"])


# ------------------------------------------------------------------------------------------------ operands, references
def _rs(name, kind):
    return np.random.RandomState(zlib.crc32(("%s/%s" % (name, kind)).encode()) & 0x7FFFFFFF)


def _draw(rs, kind, shape, scale=1.0):
    if kind == "integer":
        return rs.randint(-4, 5, size=shape).astype(F)
    return (rs.standard_normal(shape) * scale).astype(F)


def act64(v, act):
    return np.maximum(v, 0.0) if act == "relu" else np.tanh(v) if act == "tanh" else v


def case_act(c, kind):
    return c["act"] if kind == "random" else None


@functools.lru_cache(maxsize=4)
def fwd_operands(name, kind):
    """-> dict(x, w, bias: lists of nz float32 arrays (bias None where the pointer is null), want: nz float64 [B, O])"""
    c = by_name(name)
    rs = _rs(name, kind)
    B, K, O, nz = c["B"], c["K"], c["O"], c["nz"]
    xs = [_draw(rs, kind, (B, K)) for _ in range(nz)]
    ws = [_draw(rs, kind, (O, K), 1.0 / np.sqrt(K)) for _ in range(nz)]
    bs = [_draw(rs, kind, (O,), 0.1) for _ in range(nz)]
    bs = [None if (c["null_bias"] == "array" or z in c["null_bias"]) else b for z, b in enumerate(bs)]
    want = [fwd_ref(x, w, b, case_act(c, kind)) for x, w, b in zip(xs, ws, bs)]
    return dict(x=xs, w=ws, bias=bs, want=want)


def fwd_ref(x, w, b, act, dtype=D):
    pre = x.astype(dtype) @ w.astype(dtype).T
    if b is not None:
        pre = pre + b.astype(dtype)
    return act64(pre, act)


@functools.lru_cache(maxsize=4)
def slabs_operands(name, kind):
    c = by_name(name)
    rs = _rs(name, kind)
    xs = [_draw(rs, kind, (c["B"], c["K"])) for _ in range(c["nz"])]
    ws = [_draw(rs, kind, (c["O"], c["K"]), 1.0 / np.sqrt(c["K"])) for _ in range(c["nz"])]
    return dict(x=xs, w=ws, want=[fwd_ref(x, w, None, None) for x, w in zip(xs, ws)])


@functools.lru_cache(maxsize=4)
def bwd_w_operands(name, kind):
    c = by_name(name)
    rs = _rs(name, kind)
    dy, x = _draw(rs, kind, (c["B"], c["O"])), _draw(rs, kind, (c["B"], c["I"]))
    dw, db = bwd_w_ref(dy, x)
    return dict(dy=dy, x=x, dw=dw, db=db)


def bwd_w_ref(dy, x, dtype=D):
    return dy.astype(dtype).T @ x.astype(dtype), dy.astype(dtype).sum(0)


def mask64(xact, mask, dtype=D):
    if mask == "relu":
        return (xact > 0).astype(dtype)
    if mask == "tanh":
        return 1.0 - xact.astype(dtype) ** 2
    return None


def bwd_x_ref(dy, w, xact, mask, dtype=D):
    dx = dy.astype(dtype) @ w.astype(dtype)
    m = mask64(xact, mask, dtype) if xact is not None else None
    return dx if m is None else dx * m


def _xact(rs, kind, shape, mask):
    """The activated output the mask is derived from: a ReLU output (about half zeros), a tanh output in (-1, 1), or none."""
    if mask is None:
        return None
    v = rs.standard_normal(shape)
    return np.maximum(v, 0.0).astype(F) if mask == "relu" else np.tanh(v).astype(F)


@functools.lru_cache(maxsize=4)
def bwd_x_operands(name, kind):
    c = by_name(name)
    rs = _rs(name, kind)
    mask = c["mask"] if kind == "random" else None
    dy, w = _draw(rs, kind, (c["B"], c["O"])), _draw(rs, kind, (c["O"], c["I"]), 1.0 / np.sqrt(c["I"]))
    xact = _xact(rs, kind, (c["B"], c["I"]), mask)
    return dict(dy=dy, w=w, xact=xact, mask=mask, dx=bwd_x_ref(dy, w, xact, mask))


@functools.lru_cache(maxsize=4)
def xw_operands(name, kind):
    """x is the layer's input (a ReLU output where the case says so: about half zeros) -- the integer set keeps the mask: (x > 0)
    of integers is as exact as the sums."""
    c = by_name(name)
    rs = _rs(name, kind)
    dy, w = _draw(rs, kind, (c["B"], 512)), _draw(rs, kind, (512, c["I"]), 1.0 / np.sqrt(c["I"]))
    x = _draw(rs, kind, (c["B"], c["I"]))
    if c["relu"]:
        x = np.maximum(x, 0).astype(F)
    dw, db = bwd_w_ref(dy, x)
    return dict(dy=dy, w=w, x=x, dx=bwd_x_ref(dy, w, x, "relu" if c["relu"] else None), dw=dw, db=db)


def act_bwd_operands(name):
    """-> dy, y, want: float32(dy * act'(y)) formed in float32 as the kernel's statement reads (igemm.h:36-40; the library is
    built without contraction, so 1 - y * y is a multiply and a subtraction)."""
    c = by_name(name)
    rs = _rs(name, "random")
    dy = rs.standard_normal(c["n"]).astype(F)
    v = rs.standard_normal(c["n"])
    y = (np.tanh(v) if c["act"] == "tanh" else np.maximum(v, 0.0) if c["act"] == "relu" else v).astype(F)
    if c["act"] == "relu":
        want = dy * (y > 0).astype(F)
    elif c["act"] == "tanh":
        want = dy * (F(1.0) - y * y)
    else:
        want = dy * F(1.0)
    assert want.dtype == F
    return dy, y, want


@functools.lru_cache(maxsize=4)
def autograd_operands(name):
    """-> x, w, b, dy (float32) and the float64 CPU autograd results y, dx, dw, db, margin (the smallest |pre-activation| where the
    layer ends in a ReLU, else inf).  x_relu: x is a ReLU output and dx is the gradient of ITS pre-activation (dx * (x > 0))."""
    import torch
    c = by_name(name)
    rs = _rs(name, "random")
    B, K, O = c["B"], c["K"], c["O"]
    x = rs.standard_normal((B, K)).astype(F)
    if c["x_relu"]:
        x = np.maximum(x, 0).astype(F)
    w, b, dy = (rs.standard_normal((O, K)) / np.sqrt(K)).astype(F), (0.1 * rs.standard_normal(O)).astype(F), rs.standard_normal((B, O)).astype(F)
    xt, wt, bt = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b)]
    pre = torch.nn.functional.linear(xt, wt, bt)
    y = torch.relu(pre) if c["act"] == "relu" else torch.tanh(pre) if c["act"] == "tanh" else pre
    y.backward(torch.tensor(dy, dtype=torch.float64))
    dx = xt.grad.numpy() * ((x > 0) if c["x_relu"] else 1.0)
    margin = float(pre.detach().abs().min()) if c["act"] == "relu" else float("inf")
    return dict(x=x, w=w, b=b, dy=dy, y=y.detach().numpy(), dx=dx, dw=wt.grad.numpy(), db=bt.grad.numpy(), margin=margin)


def int_bound(c):
    """Largest |partial sum| any summation order can meet on the integer set: operands in [-4, 4], so 16 per term over the
    case's longest reduction, + 4 for a bias.  Must stay below 2^24 for float32 to hold every partial sum exactly."""
    if "K" in c:
        terms = c["K"]
    else:
        terms = max(c["B"], c["O"])              # weight gradient: over the batch; input gradient: over the outputs
    return 16 * terms + 4


ALL_CASES = FWD_CASES + SLABS_CASES + SLABS_ONE_CASES + BWD_W_CASES + BWD_X_CASES + XW_CASES + ACT_BWD_CASES + AUTOGRAD_CASES
_BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(_BY_NAME) == len(ALL_CASES), "case names must be unique"


def by_name(name):
    return _BY_NAME[name]


def rows_to_compare(B):
    """First and last row of every 32-row block (batch independence of the gemv and rows kernels)."""
    out = []
    for b0 in range(0, B, 32):
        out += [b0, min(b0 + 31, B - 1)]
    return sorted(set(out))
