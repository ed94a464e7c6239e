"""Edge-shape cases of the fused policy-head launches behind CategoricalActorCriticNet and the pixel A2C / PPO agents
(csrc/igemm.hip dra_linear_fwd_pair, dra_linear_bwd_pair, dra_policy_heads_sample / _given / _given_fold / _sample_fold28 / _bwd;
csrc/rollout_roles.h heads_row_outputs_from, policy_head_row, policy_head_row_fold_wg; the head role of csrc/conv_v2.hip
dra_rollout_conv1_heads_phi; ops.fc4_policy_heads_given; nets._LinearPairFn / _PolicyHeadFn and the ladder in
CategoricalActorCriticNet.forward): the case
tables, a restatement of what every launch does with its shape, float64 references and the operand sets.  CPU only, numpy and
torch; tests/test_policy_head_edge_cases_host.py proves the tables, tests/test_gpu_policy_head_edges.py holds the kernels to them.

Operand sets, per case:
  random   standard normals, W0 scaled to logits of a few units, biases at 0.1 scale
  integer  values in [-4, 4] on the LINEAR parts (logits, v, all of linear_bwd_pair): every partial sum is an integer below 2^24
           (int_bound), so any correct summation order gives the int64 result bit for bit.
References: float64 from the float32 operand values -- logits and v as matrix products, the distribution through
loss_edge_cases.categorical_ref / inverse_cdf, dx / dW / db as products of the float64 dlogits, masks from the given features
((x > 0)).  Every reference takes a dtype; the float32 CPU run of the same statement is the yardstick for BAR_OVERRIDES.
The fold is exact, not approximate: phi = relu(((slab0 + slab1) + ... + slab_{KS-1}) + bias) in float32, one rounding per
operation (fold_np), relu(v) = v > 0 ? v : +0.

Bar (not tuned to the kernels): BAR = 1e-5 of the reference's max-abs per output tensor.  BAR_OVERRIDES is empty: the float32
CPU run of every random-operand case stays within the bar (the host test measures it: the largest figure is 4.0e-6, dw0 of
heads_bwd-8192x8x2, a float32 sum over 8192 samples).
Sampled actions equal the float64 inverse CDF on EVERY row: a row is strict (u >= 1: always the last action) or its smallest
CDF-boundary margin is at least cdf_threshold = 2 BAR max|logits64| + 64 * 2^-23 (a logit error of delta moves the cumulative
sums by at most 2 delta; the float32 cumulative sum over <= 64 terms adds the second term).  A drawn uniform that misses the
threshold is replaced by the midpoint of its row's widest CDF step (settle_uniforms); no row is exempt."""
import functools
import itertools
import zlib

import numpy as np
import torch

from loss_edge_cases import U_BELOW_ONE, categorical_ref, clamp_action, inverse_cdf

BAR = 1e-5
# (case name, tensor key) -> (bar, error / scale of the float32 CPU run of the reference on the same inputs)
BAR_OVERRIDES = {}
F, D = np.float32, np.float64
ACTS = (None, "relu", "tanh")

# the launchers' limits, restated (tests/test_policy_head_edge_cases_host.py reads each from the source line cited)
MAX_FWD_BATCH = 65536       # csrc/igemm.hip dra_policy_heads_sample / _given / _given_fold / _sample_fold28, dra_linear_fwd_pair
HEADS_BWD_MAX_BATCH = 8192  # csrc/igemm.hip kHeadsBwdMaxBatch == ops.HEADS_BWD_MAX_BATCH
MAX_K = 512                 # in_features of every launch here; the fold forms are K = 512 only
MAX_A = 64                  # n_actions
GIVEN_FOLD_SLICES = (8, 14)     # csrc/igemm.hip dra_policy_heads_given_fold
ROLLOUT_SLICES = 28             # dra_policy_heads_sample_fold28 and the riding head
RIDING_MAX_BATCH = 4096     # csrc/conv_v2.hip dra_rollout_conv1_heads_phi
NW8_MAX_BATCH = 16          # csrc/conv_v2.hip kConvNw8MaxBatch: eight waves per conv1 workgroup up to here, four beyond
OUT_OF_RANGE = (-1, None, 2 ** 40)      # None: the count itself (head_edge_cases.OUT_OF_RANGE)


def bar(name, key):
    return BAR_OVERRIDES.get((name, key), (BAR,))[0]


# ------------------------------------------------------------------------------------------------- dispatch, restated
def fwd_dispatch(B, K, O0, O1):
    """What heads_row_outputs_from and its launchers do with a shape (rollout_roles.h:19-58, igemm.hip:246-319): four rows per
    workgroup of four waves; the row in 8 registers per lane, k = lane + 64 i; outputs of [0, O0 + O1) in groups of eight, the
    last group's spare slots clamped to output OT - 1."""
    wgs, OT = (B + 3) // 4, O0 + O1
    groups = (OT + 7) // 8
    return dict(wgs=wgs, last_rows=B - 4 * (wgs - 1),                # rows of the last workgroup (1..4)
                kregs=(K + 63) // 64, ktail=K % 64,                  # registers with any lane in range; lanes of the last one (0: all)
                groups=groups, last_group=OT - 8 * (groups - 1),     # outputs of the last group (1..8)
                straddle=O0 % 8 != 0)                                # one group of eight holds rows of w0 AND of w1


def bwd_dispatch(B, K, O0, O1):
    """policy_heads_bwd_kernel / linear_pair_bwd_kernel (igemm.hip:369-445, 476-533): B input-gradient workgroups (thread t owns
    k0 = t and k1 = t + 256), then 2 (O0 + O1) weight-gradient workgroups, each walking the batch in rounds of 32, 8 and 1; the
    fused head stages its gradient column in LDS (max(B, 64) floats) in trips of 256 samples."""
    return dict(wgs=B + 2 * (O0 + O1), rounds=(B // 32, (B % 32) // 8, B % 8), trips=(B + 255) // 256,
                halves=(min(K, 256), max(K - 256, 0)), lds_floats=max(B, 64))


def fold_dispatch(B, KS):
    """policy_head_row_fold_wg (rollout_roles.h:123-167): one workgroup per row, thread t folds features t and t + 256 from slabs
    s * B * 512 floats apart."""
    return dict(wgs=B, slab_stride=B * 512, slices=KS)


def riding_dispatch(B, mode):
    """dra_rollout_conv1_heads_phi (conv_v2.hip:1850-1889): the head's workgroups ride in front of conv1's 13 per sample; eight
    waves per workgroup up to kConvNw8MaxBatch samples, four beyond (the head's workgroups use the first four waves either way)."""
    head_wgs = 0 if mode == "none" else (B + 3) // 4 if mode == "plain" else B
    return dict(waves=8 if B <= NW8_MAX_BATCH else 4, head_wgs=head_wgs, partial_group=mode == "plain" and B % 4 != 0)


def head_path(hidden, A, B, grad, given):
    """CategoricalActorCriticNet.forward over an FCBody on the device (nets.py:1231-1282), float32 features [B, hidden], both
    heads plain Linear layers with biases, no sampler.  -> (heads, distribution):
      ("sample", "sample")                      ops.policy_heads_sample, one launch              nets.py:1247-1254
      ("policy_head_fn", "policy_head_fn")      _PolicyHeadFn: policy_heads_given / _bwd         nets.py:1255-1262
      ("linear_pair_fn" | "linear_fwd_pair" | "separate", "categorical_policy" | "torch")        nets.py:1263-1282"""
    pair = hidden <= MAX_K and B <= MAX_FWD_BATCH                                    # :1242
    if pair and not given and not grad and A <= MAX_A:                               # :1247
        return ("sample", "sample")
    if pair and given and A <= MAX_A and B <= HEADS_BWD_MAX_BATCH:                   # :1255-1256
        return ("policy_head_fn", "policy_head_fn")
    heads = ("linear_pair_fn" if grad else "linear_fwd_pair") if pair else "separate"   # :1263-1273
    return (heads, "categorical_policy" if A <= MAX_A else "torch")                  # :1274


# ------------------------------------------------------------------------------------------------------- case tables
def _fwd(kind, B, K, O0, O1=1, act=None, null=(), reaches=None):
    name = "%s-%dx%dx%d%s%s%s" % (kind, B, K, O0, "+%d" % O1 if kind == "fwd_pair" and O1 != 1 else "",
                                   "-" + act if act else "", "".join("-no-" + n for n in null))
    return dict(name=name, kind=kind, B=B, K=K, O0=O0, O1=O1, A=O0, act=act, null=tuple(null), reaches=dict(reaches or {}))


# (B, K, A, what the shape is there for)
_FWD_SHAPES = [
    (1, 1, 1, dict(wgs=1, last_rows=1, kregs=1, ktail=1, groups=1, last_group=2)),
    (3, 63, 7, dict(last_rows=3, ktail=63, groups=1, last_group=8, straddle=True)),
    (4, 64, 8, dict(last_rows=4, kregs=1, ktail=0, groups=2, last_group=1, straddle=False)),
    (5, 65, 15, dict(wgs=2, last_rows=1, kregs=2, ktail=1, groups=2, last_group=8, straddle=True)),
    (33, 255, 16, dict(wgs=9, last_rows=1, kregs=4, ktail=63, groups=3, last_group=1, straddle=False)),
    (5, 256, 64, dict(kregs=4, ktail=0, groups=9, last_group=1)),
    (3, 257, 7, dict(kregs=5, ktail=1)),
    (4, 511, 15, dict(kregs=8, ktail=63)),
    (33, 512, 64, dict(kregs=8, ktail=0, groups=9, last_group=1)),
    (1, 512, 1, dict(kregs=8, groups=1, last_group=2)),
    (MAX_FWD_BATCH, 4, 2, dict(wgs=16384, last_rows=4)),              # the launchers' limit
]
FWD_CASES = [_fwd(kind, B, K, A, reaches=r) for kind in ("fwd_pair", "sample", "given") for B, K, A, r in _FWD_SHAPES]
# dra_linear_fwd_pair alone: widths that put the w0 / w1 boundary inside a group of eight, O0 beyond 64, every act
_PAIR_WIDTHS = [((3, 7), dict(groups=2, last_group=2, straddle=True)), ((8, 8), dict(groups=2, last_group=8, straddle=False)),
                ((1, 1), dict(groups=1, last_group=2, straddle=True)), ((70, 2), dict(groups=9, last_group=8, straddle=True))]
FWD_CASES += [_fwd("fwd_pair", 5, 65, o0, o1, act=a, reaches=r) for (o0, o1), r in _PAIR_WIDTHS for a in ACTS]
# null biases (bp ? ... : 0)
FWD_CASES += [_fwd(kind, 5, 65, 7, null=n, reaches=dict(straddle=True)) for kind in ("fwd_pair", "sample", "given")
              for n in (("b0",), ("b1",), ("b0", "b1"))]

# the fold forms: slabs are plain arrays [KS][B][512]; B enters the slab stride
FOLD_CASES = [dict(name="%s-ks%d-%dx%d" % (kind, ks, B, A), kind=kind, KS=ks, B=B, K=512, A=A,
                   reaches=dict(wgs=B, slab_stride=B * 512, slices=ks))
              for kind, ks in (("given_fold", 8), ("given_fold", 14), ("sample_fold28", 28))
              for B, A in ((1, 6), (3, 1), (33, 64), (3, 64), (33, 6))]


def _bwd(kind, B, K, O0, O1=1, relu=False, null=(), dx=True, reaches=None, tag=""):
    name = "%s-%dx%dx%d%s%s%s%s%s" % (kind, B, K, O0, "+%d" % O1 if kind == "bwd_pair" and O1 != 1 else "", "-relu" if relu else "",
                                      "".join("-no-" + n for n in null), "" if dx else "-no-dx", "-" + tag if tag else "")
    return dict(name=name, kind=kind, B=B, K=K, O0=O0, O1=O1, A=O0, relu=relu, null=tuple(null), dx=dx, reaches=dict(reaches or {}))


# (B, K, A, relu_mask, what for): every batch of the list, K and A thinned over them
_BWD_SHAPES = [
    (1, 1, 1, False, dict(rounds=(0, 0, 1), halves=(1, 0), lds_floats=64)),
    (7, 255, 8, True, dict(rounds=(0, 0, 7), halves=(255, 0))),
    (8, 256, 64, False, dict(rounds=(0, 1, 0), halves=(256, 0))),              # the 8-round alone
    (9, 257, 1, True, dict(rounds=(0, 1, 1), halves=(256, 1))),
    (31, 512, 8, False, dict(rounds=(0, 3, 7), halves=(256, 256))),
    (32, 1, 64, True, dict(rounds=(1, 0, 0), halves=(1, 0))),                  # the 32-round alone
    (33, 255, 1, False, dict(rounds=(1, 0, 1))),
    (40, 256, 8, True, dict(rounds=(1, 1, 0))),                                # 32 + 8, no tail
    (41, 257, 64, True, dict(rounds=(1, 1, 1), halves=(256, 1), lds_floats=64)),
    (47, 512, 1, True, dict(rounds=(1, 1, 7), halves=(256, 256))),
    (257, 257, 8, True, dict(rounds=(8, 0, 1), trips=2, lds_floats=257)),      # second trip of the staging loop
    (257, 512, 64, False, dict(trips=2, halves=(256, 256))),
    (65, 511, 64, True, dict(halves=(256, 255), lds_floats=65)),
    (64, 64, 64, False, dict(lds_floats=64, rounds=(2, 0, 0))),
    (3, 512, 64, True, dict(halves=(256, 256))),
    (HEADS_BWD_MAX_BATCH, 8, 2, False, dict(trips=32, rounds=(256, 0, 0), lds_floats=8192)),    # the launcher's limit
]
BWD_CASES = [_bwd("heads_bwd", B, K, A, relu=relu, reaches=r) for B, K, A, relu, r in _BWD_SHAPES]
# every subset of the output gradients null, and dx null, on one small shape
_G = ("g_lp", "g_ent", "g_v")
BWD_CASES += [_bwd("heads_bwd", 9, 257, 8, relu=True, null=n, reaches=dict(rounds=(0, 1, 1)))
              for k in (1, 2, 3) for n in itertools.combinations(_G, k)]
BWD_CASES += [_bwd("heads_bwd", 9, 257, 8, relu=r, dx=False, reaches=dict(rounds=(0, 1, 1))) for r in (False, True)]
BWD_CASES += [_bwd("bwd_pair", B, K, A, reaches=r) for B, K, A, _, r in _BWD_SHAPES
              if "lds_floats" not in r or B in (1, 41, 257, HEADS_BWD_MAX_BATCH)]
BWD_CASES += [_bwd("bwd_pair", 9, 65, 3, 7, reaches=dict(wgs=29)), _bwd("bwd_pair", 40, 257, 70, 2, reaches=dict(wgs=184)),
              _bwd("bwd_pair", 9, 257, 8, dx=False, reaches=dict(rounds=(0, 1, 1)))]
for _c in BWD_CASES:
    if _c["kind"] == "bwd_pair":
        _c["reaches"].pop("lds_floats", None)       # linear_pair_bwd_kernel stages nothing
        _c["reaches"].pop("trips", None)

# out-of-range given actions: every eleventh one -1, A or 2^40 -- the forward promises the nearest valid action
# (loss_edge_cases.clamp_action), the backward must differentiate that
OOR_CASES = [dict(name="oor-heads-47x65x7", kind="heads", B=47, K=65, A=7), dict(name="oor-categorical-47x7", kind="categorical", B=47, A=7),
             dict(name="oor-heads-34x64x64", kind="heads", B=34, K=64, A=64), dict(name="oor-categorical-300x2", kind="categorical", B=300, A=2)]

# sampling rows at the uniforms 0, 1 - 2^-24 and 1: identity weights (logits = features, exactly), so rows can be set directly
SAMPLING_CASES = [dict(name="rows-sample-64", kind="sample", K=64, A=64, B=12),
                  dict(name="rows-sample_fold28-512", kind="sample_fold28", K=512, A=64, B=12)]

_RIDING_WAVES = {1: 8, 5: 8, 16: 8, 17: 4}                   # the two sides of kConvNw8MaxBatch
_RIDING_HEAD_WGS = {"none": {1: 0, 5: 0, 16: 0, 17: 0}, "plain": {1: 1, 5: 2, 16: 4, 17: 5}, "fold28": {1: 1, 5: 5, 16: 16, 17: 17}}
RIDING_CASES = [dict(name="riding-%s-%d" % (mode, B), mode=mode, B=B, A=6,
                     reaches=dict(waves=_RIDING_WAVES[B], head_wgs=_RIDING_HEAD_WGS[mode.split("+")[0]][B]))
                for mode in ("none", "plain", "fold28", "fold28+phi") for B in (1, 5, 16, 17)]


def _net(hidden, A, B, grad, given, gate, path, tag=""):
    name = "net-h%d-a%d-b%d-%s-%s-%s%s" % (hidden, A, B, "grad" if grad else "nograd", "given" if given else "sampled", gate,
                                            "-" + tag if tag else "")
    return dict(name=name, hidden=hidden, A=A, B=B, grad=grad, given=given, gate=gate, state_dim=5, reaches=path)


NET_CASES = [
    # both sides of hidden 512 | 513
    _net(512, 6, 5, True, True, "relu", ("policy_head_fn", "policy_head_fn")),
    _net(513, 6, 5, True, True, "relu", ("separate", "categorical_policy")),
    _net(512, 6, 33, False, False, "relu", ("sample", "sample")),
    _net(513, 6, 33, False, False, "relu", ("separate", "categorical_policy")),
    # 64 | 65 actions
    _net(64, 64, 9, True, True, "relu", ("policy_head_fn", "policy_head_fn")),
    _net(64, 65, 9, True, True, "relu", ("linear_pair_fn", "torch")),
    _net(64, 64, 9, False, False, "tanh", ("sample", "sample")),
    _net(64, 65, 9, False, False, "tanh", ("linear_fwd_pair", "torch")),
    # batch 8192 | 8193 (tanh bodies: no gate decides a gradient at these sizes)
    _net(16, 3, HEADS_BWD_MAX_BATCH, True, True, "tanh", ("policy_head_fn", "policy_head_fn")),
    _net(16, 3, HEADS_BWD_MAX_BATCH + 1, True, True, "tanh", ("linear_pair_fn", "categorical_policy")),
    # with | without gradient, given | sampled
    _net(64, 6, 33, False, True, "relu", ("policy_head_fn", "policy_head_fn")),
    _net(64, 6, 33, True, False, "relu", ("linear_pair_fn", "categorical_policy")),
    # fused ReLU | tanh under _PolicyHeadFn
    _net(64, 6, 33, True, True, "relu", ("policy_head_fn", "policy_head_fn")),
    _net(64, 6, 33, True, True, "tanh", ("policy_head_fn", "policy_head_fn")),
]
RELU_MARGIN = 1e-5      # no float64 pre-activation of a ReLU body this close to zero (host test): the gates are the float32 run's

# ops.fc4_policy_heads_given: fc4's one-pass 8-slice forward + the head launch that folds the slices, from fc4's INPUT
FC4_CASES = [dict(name="fc4_given-%dx%d" % (B, A), B=B, A=A) for B, A in ((3, 6), (33, 64))]

ALL_CASES = FWD_CASES + FOLD_CASES + BWD_CASES + OOR_CASES + SAMPLING_CASES + RIDING_CASES + NET_CASES + FC4_CASES
_BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(_BY_NAME) == len(ALL_CASES), "case names must be unique"


def by_name(name):
    return _BY_NAME[name]


def dispatch_of(c):
    """The restated dispatch of a case, by table."""
    if c in FWD_CASES:
        return fwd_dispatch(c["B"], c["K"], c["O0"], c["O1"])
    if c in FOLD_CASES:
        return fold_dispatch(c["B"], c["KS"])
    if c in BWD_CASES:
        return bwd_dispatch(c["B"], c["K"], c["O0"], c["O1"])
    if c in RIDING_CASES:
        return riding_dispatch(c["B"], c["mode"])
    if c in NET_CASES:
        return head_path(c["hidden"], c["A"], c["B"], c["grad"], c["given"])
    return None


# what the tables must reach, taken together: name -> predicate
def _fwd_any(kinds, pred):
    return all(any(c["kind"] == k and pred(c, fwd_dispatch(c["B"], c["K"], c["O0"], c["O1"])) for c in FWD_CASES) for k in kinds)


def _bwd_any(kinds, pred):
    return all(any(c["kind"] == k and pred(c, bwd_dispatch(c["B"], c["K"], c["O0"], c["O1"])) for c in BWD_CASES) for k in kinds)


_HEADS3, _BWD2 = ("fwd_pair", "sample", "given"), ("heads_bwd", "bwd_pair")
COVERAGE = {
    **{"forward K = %d (all three launches)" % k: (lambda k=k: _fwd_any(_HEADS3, lambda c, d: c["K"] == k))
       for k in (1, 63, 64, 65, 255, 256, 257, 511, 512)},
    **{"forward A = %d" % a: (lambda a=a: _fwd_any(_HEADS3, lambda c, d: c["O0"] == a and c["O1"] == 1)) for a in (1, 7, 8, 15, 16, 64)},
    **{"forward B = %d" % b: (lambda b=b: _fwd_any(_HEADS3, lambda c, d: c["B"] == b)) for b in (1, 3, 4, 5, 33, MAX_FWD_BATCH)},
    **{"forward last workgroup of %d rows" % r: (lambda r=r: _fwd_any(_HEADS3, lambda c, d: d["last_rows"] == r)) for r in (1, 3, 4)},
    "forward several workgroups, the last one partial": lambda: _fwd_any(_HEADS3, lambda c, d: d["wgs"] > 1 and d["last_rows"] < 4),
    **{"forward last group of %d outputs" % g: (lambda g=g: _fwd_any(_HEADS3, lambda c, d: d["last_group"] == g)) for g in (1, 2, 8)},
    "forward given at A = 64 (s_out[68], t < A)": lambda: _fwd_any(("given",), lambda c, d: c["A"] == 64),
    "fwd_pair group straddles w0 | w1": lambda: _fwd_any(("fwd_pair",), lambda c, d: d["straddle"] and c["O1"] > 1),
    "fwd_pair O0 > 64": lambda: _fwd_any(("fwd_pair",), lambda c, d: c["O0"] > 64),
    **{"fwd_pair (%d, %d) act %s" % (o0, o1, a): (lambda o0=o0, o1=o1, a=a: _fwd_any(("fwd_pair",), lambda c, d: (c["O0"], c["O1"], c["act"]) == (o0, o1, a)))
       for (o0, o1), _ in _PAIR_WIDTHS for a in ACTS},
    **{"forward null %s" % "+".join(n): (lambda n=n: _fwd_any(_HEADS3, lambda c, d: c["null"] == n)) for n in (("b0",), ("b1",), ("b0", "b1"))},
    "given_fold 8 and 14 slices, sample_fold28": lambda: {(c["kind"], c["KS"]) for c in FOLD_CASES} == {("given_fold", 8), ("given_fold", 14), ("sample_fold28", 28)},
    **{"fold B = %d for every form" % b: (lambda b=b: all(any(c["KS"] == ks and c["B"] == b for c in FOLD_CASES) for ks in (8, 14, 28))) for b in (1, 3, 33)},
    **{"fold A = %d for every form" % a: (lambda a=a: all(any(c["KS"] == ks and c["A"] == a for c in FOLD_CASES) for ks in (8, 14, 28))) for a in (1, 6, 64)},
    **{"backward B = %d (both launches)" % b: (lambda b=b: _bwd_any(_BWD2, lambda c, d: c["B"] == b))
       for b in (1, 7, 8, 9, 31, 32, 33, 40, 41, 47, 257, HEADS_BWD_MAX_BATCH)},
    "backward 32-round alone": lambda: _bwd_any(_BWD2, lambda c, d: d["rounds"] == (1, 0, 0)),
    "backward 8-round alone": lambda: _bwd_any(_BWD2, lambda c, d: d["rounds"] == (0, 1, 0)),
    "backward tail alone": lambda: _bwd_any(_BWD2, lambda c, d: d["rounds"][:2] == (0, 0) and d["rounds"][2] > 0),
    "backward 32 + 8 without a tail (B = 40)": lambda: _bwd_any(_BWD2, lambda c, d: d["rounds"] == (1, 1, 0)),
    "backward all three rounds (B = 47)": lambda: _bwd_any(_BWD2, lambda c, d: d["rounds"] == (1, 1, 7)),
    **{"backward K = %d" % k: (lambda k=k: _bwd_any(_BWD2, lambda c, d: c["K"] == k)) for k in (1, 255, 256, 257, 512)},
    **{"backward A = %d" % a: (lambda a=a: _bwd_any(_BWD2, lambda c, d: c["O0"] == a)) for a in (1, 8, 64)},
    "heads_bwd at A = 64": lambda: _bwd_any(("heads_bwd",), lambda c, d: c["A"] == 64 and d["lds_floats"] == 64),
    "heads_bwd second staging trip": lambda: _bwd_any(("heads_bwd",), lambda c, d: d["trips"] == 2 and c["B"] == 257),
    "heads_bwd at the batch limit": lambda: _bwd_any(("heads_bwd",), lambda c, d: c["B"] == HEADS_BWD_MAX_BATCH),
    "heads_bwd relu_mask on and off": lambda: {c["relu"] for c in BWD_CASES if c["kind"] == "heads_bwd"} == {True, False},
    "heads_bwd every subset of g_* null": lambda: {c["null"] for c in BWD_CASES if c["kind"] == "heads_bwd"} ==
    {n for k in range(4) for n in itertools.combinations(_G, k)},
    "dx null (both launches)": lambda: _bwd_any(_BWD2, lambda c, d: not c["dx"]),
    "bwd_pair O1 > 1 and O0 > 64": lambda: _bwd_any(("bwd_pair",), lambda c, d: c["O1"] > 1) and _bwd_any(("bwd_pair",), lambda c, d: c["O0"] > 64),
    "out-of-range actions: fused head and plain categorical": lambda: {c["kind"] for c in OOR_CASES} == {"heads", "categorical"},
    "sampling rows: stand-alone and fold28": lambda: {c["kind"] for c in SAMPLING_CASES} == {"sample", "sample_fold28"},
    "riding head: every mode at B = 1, 5, 16, 17": lambda: {(c["mode"], c["B"]) for c in RIDING_CASES} ==
    {(m, b) for m in ("none", "plain", "fold28", "fold28+phi") for b in (1, 5, 16, 17)},
    "riding head: 8 and 4 waves": lambda: {c["reaches"]["waves"] for c in RIDING_CASES} == {4, 8},
    **{"net path %s / %s" % p: (lambda p=p: any(c["reaches"] == p for c in NET_CASES))
       for p in (("sample", "sample"), ("policy_head_fn", "policy_head_fn"), ("linear_pair_fn", "categorical_policy"),
                 ("linear_pair_fn", "torch"), ("linear_fwd_pair", "torch"), ("separate", "categorical_policy"))},
    "fc4 + head through ops on both sides of a group of four rows": lambda: {c["B"] for c in FC4_CASES} == {3, 33},
    "net hidden 512 | 513": lambda: {c["hidden"] for c in NET_CASES} >= {512, 513},
    "net 64 | 65 actions": lambda: {c["A"] for c in NET_CASES} >= {64, 65},
    "net batch 8192 | 8193": lambda: {c["B"] for c in NET_CASES} >= {HEADS_BWD_MAX_BATCH, HEADS_BWD_MAX_BATCH + 1},
    "net policy_head_fn over relu and tanh": lambda: {c["gate"] for c in NET_CASES if c["reaches"][0] == "policy_head_fn" and c["grad"]} == {"relu", "tanh"},
    "net given without gradient, sampled with": lambda: any(c["given"] and not c["grad"] for c in NET_CASES) and
    any(c["grad"] and not c["given"] for c in NET_CASES),
}


# ------------------------------------------------------------------------------------------------ operands, references
def _rs(name, kind):
    return np.random.RandomState(zlib.crc32(("%s/%s" % (name, kind)).encode()) & 0x7FFFFFFF)


def _draw(rs, kind, shape, scale=1.0):
    if kind == "integer":
        return rs.randint(-4, 5, size=shape).astype(F)
    return (rs.standard_normal(shape) * scale).astype(F)


def act_ref(v, act):
    return np.maximum(v, 0) if act == "relu" else np.tanh(v) if act == "tanh" else v


def heads_ref(x, w0, b0, w1, b1, act=None, dtype=D):
    """-> (y0 [B, O0], y1 [B, O1]) = act(x W^T + b), a null bias being zero."""
    x = x.astype(dtype)
    y0, y1 = x @ w0.astype(dtype).T, x @ w1.astype(dtype).T
    if b0 is not None:
        y0 = y0 + b0.astype(dtype)
    if b1 is not None:
        y1 = y1 + b1.astype(dtype)
    return act_ref(y0, act), act_ref(y1, act)


def cdf_threshold(logits64):
    return 2 * BAR * float(np.abs(logits64).max()) + 64 * 2.0 ** -23


def settle_uniforms(p64, u, threshold):
    """Rows that are neither strict (u >= 1) nor clear of every CDF boundary by `threshold` get the midpoint of their widest
    CDF step instead (>= 1 / (2 A) from both of its ends)."""
    u = u.copy()
    _, margin = inverse_cdf(p64, u)
    for b in np.nonzero((margin < 2 * threshold) & (u < 1.0))[0]:
        j = int(np.argmax(p64[b]))
        u[b] = F(p64[b, :j].sum() + 0.5 * p64[b, j])
    return u


def head_ref(logits, v, action, g=None, dtype=D):
    """Categorical(logits) of given actions (clamped into range, the forward's promise) -> dict(log_pi_a, entropy, p, dlogits)."""
    B, A = logits.shape
    z = np.zeros(B, F)
    g_lp, g_ent = (z, z) if g is None else (z if g[0] is None else g[0], z if g[1] is None else g[1])
    return categorical_ref(logits.astype(dtype), clamp_action(action, A), g_lp, g_ent, torch.float64 if dtype == D else torch.float32)


ANCHOR = 1.25


def _anchor(b, x_row, w_row):
    """Bias element 0 moved so that output 0 of row 0 is ANCHOR.  A tensor of one or a few outputs has no scale of its own: x . w
    of a single row can cancel to any small value while the partial sums of the float32 run stay O(1), and 1e-5 of a cancelled
    value is no bar for that sum in ANY order.  With one output of known size in it, max-abs is a scale again (MIN_SCALE, which
    the host test holds every linear output of the random set to)."""
    b[0] = F(ANCHOR - float(x_row.astype(D) @ w_row.astype(D)))
    return b


MIN_SCALE = 0.5


def _heads_operands(rs, kind, B, K, O0, O1, null=()):
    x = _draw(rs, kind, (B, K))
    w0 = _draw(rs, kind, (O0, K), 2.5 / np.sqrt(K))
    w1 = _draw(rs, kind, (O1, K), 1.0 / np.sqrt(K))
    b0 = None if "b0" in null else _draw(rs, kind, (O0,), 0.1)
    b1 = None if "b1" in null else _draw(rs, kind, (O1,), 0.1)
    if kind == "random":
        b0 = b0 if b0 is None else _anchor(b0, x[0], w0[0])
        b1 = b1 if b1 is None else _anchor(b1, x[0], w1[0])
    return x, w0, b0, w1, b1


@functools.lru_cache(maxsize=4)
def fwd_operands(name, kind):
    """-> x, w0, b0, w1, b1 (float32; a null bias None), u, action, and the float64 results: y0 / y1 (act applied), and for the
    head launches lp_given / ent / p / sampled (+ lp_sampled) on logits = y0, v = y1[:, 0]."""
    c = by_name(name)
    rs = _rs(name, kind)
    B, A = c["B"], c["O0"]
    x, w0, b0, w1, b1 = _heads_operands(rs, kind, B, c["K"], c["O0"], c["O1"], c["null"])
    act = c["act"] if kind == "random" else None
    y0, y1 = heads_ref(x, w0, b0, w1, b1, act)
    op = dict(x=x, w0=w0, b0=b0, w1=w1, b1=b1, y0=y0, y1=y1, act=act)
    if c["kind"] != "fwd_pair":
        action = rs.randint(0, A, size=B).astype(np.int64)
        ref = head_ref(y0, None, action)
        u = rs.rand(B).astype(F)
        u[B - 1] = 1.0                                    # a strict row in every case
        u = settle_uniforms(ref["p"], u, cdf_threshold(y0))
        sampled, margin = inverse_cdf(ref["p"], u)
        op.update(action=action, u=u, lp_given=ref["log_pi_a"], ent=ref["entropy"], p=ref["p"], sampled=sampled, margin=margin,
                  lp_sampled=np.take_along_axis(ref["logp"], sampled[:, None], 1)[:, 0])
    return op


def fold_np(slabs, bias):
    """relu(((slab0 + slab1) + ... + slab_{KS-1}) + bias) in float32, one rounding per operation; relu(v) = v > 0 ? v : +0."""
    v = slabs[0].astype(F).copy()
    for s in range(1, slabs.shape[0]):
        v = (v + slabs[s]).astype(F)
    v = (v + bias[None, :].astype(F)).astype(F)
    pre = v
    return np.where(v > 0, v, F(0.0)).astype(F), pre


def fold_ref(slabs, bias, dtype=D):
    v = slabs.astype(dtype).sum(0) + bias.astype(dtype)
    return np.maximum(v, 0)


@functools.lru_cache(maxsize=4)
def fold_operands(name):
    """slabs [KS][B][512] and fold bias with exact zeros among the sums: columns 0-3 all +0 with a +0 bias (sum +0), columns 4-7
    all -0.0 with a -0.0 bias (sum -0.0: the only way float32 addition gives it); about half of the other sums negative."""
    c = by_name(name)
    rs = _rs(name, "random")
    KS, B, A = c["KS"], c["B"], c["A"]
    slabs = (rs.standard_normal((KS, B, 512)) / np.sqrt(KS)).astype(F)
    bias = (0.5 * rs.standard_normal(512)).astype(F)
    slabs[:, :, 0:4], bias[0:4] = F(0.0), F(0.0)
    slabs[:, :, 4:8], bias[4:8] = F(-0.0), F(-0.0)
    phi, pre = fold_np(slabs, bias)
    w0 = (rs.standard_normal((A, 512)) * 2.5 / np.sqrt(256)).astype(F)
    w1 = (rs.standard_normal((1, 512)) / np.sqrt(256)).astype(F)
    b0, b1 = (0.1 * rs.standard_normal(A)).astype(F), (0.1 * rs.standard_normal(1)).astype(F)
    b0, b1 = _anchor(b0, phi[0], w0[0]), _anchor(b1, phi[0], w1[0])
    logits, v = heads_ref(phi, w0, b0, w1, b1)
    action = rs.randint(0, A, size=B).astype(np.int64)
    ref = head_ref(logits, None, action)
    u = rs.rand(B).astype(F)
    u[B - 1] = 1.0
    u = settle_uniforms(ref["p"], u, cdf_threshold(logits))
    sampled, margin = inverse_cdf(ref["p"], u)
    return dict(slabs=slabs, bias=bias, phi=phi, pre=pre, w0=w0, b0=b0, w1=w1, b1=b1, logits=logits, v=v[:, 0], action=action, u=u,
                lp_given=ref["log_pi_a"], ent=ref["entropy"], p=ref["p"], sampled=sampled, margin=margin,
                lp_sampled=np.take_along_axis(ref["logp"], sampled[:, None], 1)[:, 0])


def relu_features(rs, shape, kind="random"):
    """A fused-ReLU output: about half the entries exact +0, and -0.0 sprinkled over them (head_edge_cases._features)."""
    x = np.maximum(_draw(rs, kind, shape), 0).astype(F)
    neg = rs.rand(*shape) < 0.05
    x[neg & (x == 0)] = F(-0.0)
    return x


def heads_bwd_ref(logits, action, g_lp, g_ent, g_v, x, w0, w1, relu, dtype=D):
    """-> dict(dlogits, dx, dw0, db0, dw1, db1): the float64 dlogits of Categorical(logits) at the clamped actions, then plain
    products; a null gradient is zero; the mask is (x > 0) of the given features."""
    B = x.shape[0]
    dl = head_ref(logits, None, action, (g_lp, g_ent), dtype)["dlogits"].astype(dtype)
    gv = (np.zeros(B, F) if g_v is None else g_v).astype(dtype)
    return pair_bwd_ref(dl, gv[:, None], x, w0, w1, relu, dtype, dlogits=dl)


def pair_bwd_ref(g0, g1, x, w0, w1, relu=False, dtype=D, **extra):
    g0, g1, xd = g0.astype(dtype), g1.astype(dtype), x.astype(dtype)
    dx = g0 @ w0.astype(dtype) + g1 @ w1.astype(dtype)
    if relu:
        dx = dx * (x > 0)
    return dict(dx=dx, dw0=g0.T @ xd, db0=g0.sum(0), dw1=g1.T @ xd, db1=g1.sum(0), **extra)


# the output gradients of the random set have this mean: db1 = sum_b g_v[b] is ONE number, and a zero-mean sum over 8192 samples
# cancels to about 1 % of its partial sums -- no scale for a float32 sum in any order (see _anchor)
G_MEAN = 0.5


@functools.lru_cache(maxsize=4)
def bwd_operands(name, kind):
    c = by_name(name)
    rs = _rs(name, kind)
    B, K, O0, O1 = c["B"], c["K"], c["O0"], c["O1"]
    x = relu_features(rs, (B, K), kind) if c["relu"] else _draw(rs, kind, (B, K))
    w0, w1 = _draw(rs, kind, (O0, K), 2.5 / np.sqrt(K)), _draw(rs, kind, (O1, K), 1.0 / np.sqrt(K))
    if c["kind"] == "bwd_pair":
        g0, g1 = _draw(rs, kind, (B, O0)), _draw(rs, kind, (B, O1))
        if kind == "random":
            g1 = (g1 + F(G_MEAN)).astype(F)
        return dict(x=x, w0=w0, w1=w1, g0=g0, g1=g1, want=pair_bwd_ref(g0, g1, x, w0, w1))
    assert kind == "random"
    logits = _draw(rs, kind, (B, O0), 2.0)
    action = rs.randint(0, O0, size=B).astype(np.int64)
    g = {k: None if k in c["null"] else (_draw(rs, kind, (B,)) + F(G_MEAN)).astype(F) for k in _G}
    return dict(x=x, w0=w0, w1=w1, logits=logits, action=action, **g,
                want=heads_bwd_ref(logits, action, g["g_lp"], g["g_ent"], g["g_v"], x, w0, w1, c["relu"]))


def sprinkle(rs, idx, n):
    """Every eleventh entry replaced by -1, n or 2^40 in turn (head_edge_cases._sprinkle)."""
    idx = idx.copy().reshape(-1)
    for i in range(0, idx.size, 11):
        bad = OUT_OF_RANGE[(i // 11) % 3]
        idx[i] = n if bad is None else bad
    return idx


@functools.lru_cache(maxsize=4)
def oor_operands(name):
    c = by_name(name)
    rs = _rs(name, "random")
    B, A = c["B"], c["A"]
    action = sprinkle(rs, rs.randint(0, A, size=B).astype(np.int64), A)
    g_lp, g_ent, g_v = (_draw(rs, "random", (B,)) for _ in range(3))
    if c["kind"] == "categorical":
        logits = _draw(rs, "random", (B, A), 2.0)
        ref = head_ref(logits, None, action, (g_lp, g_ent))
        return dict(logits=logits, action=action, g_lp=g_lp, g_ent=g_ent, lp=ref["log_pi_a"], ent=ref["entropy"], dlogits=ref["dlogits"])
    x, w0, b0, w1, b1 = _heads_operands(rs, "random", B, c["K"], A, 1)
    logits, v = heads_ref(x, w0, b0, w1, b1)
    ref = head_ref(logits, None, action)
    return dict(x=x, w0=w0, b0=b0, w1=w1, b1=b1, action=action, g_lp=g_lp, g_ent=g_ent, g_v=g_v, logits=logits, v=v[:, 0],
                lp=ref["log_pi_a"], ent=ref["entropy"], bwd=lambda lg: heads_bwd_ref(lg, action, g_lp, g_ent, g_v, x, w0, w1, False))


@functools.lru_cache(maxsize=2)
def sampling_rows():
    """-> logits [12, 64] (non-negative, so a ReLU fold can deliver them), u [12]: rows 0-3 one logit 50 above the rest (at
    action 0 under u = 0, at the last action under 1 - 2^-24, at 21 under u = 1, at 42 under 0.5), rows 4-7 all logits equal
    under u = 0, 1 - 2^-24, 1 and a value between two boundaries, rows 8-11 spread logits (the first / last action lifted where
    u = 0 / 1 - 2^-24 asks for it), following loss_edge_cases.cat_cases."""
    rs = np.random.RandomState(6100)
    A = 64
    lg = np.abs(rs.standard_normal((12, A)) * 3).astype(F)
    for k, at in enumerate((0, A - 1, 21, 42)):
        lg[k] = np.abs(rs.standard_normal(A) * 0.5).astype(F)
        lg[k, at] += F(50.0)
        lg[4 + k] = F(k + 0.5)
    lg[8, 0] += F(6.0)
    lg[9, A - 1] += F(6.0)
    u = np.array([0.0, U_BELOW_ONE, 1.0, 0.5, 0.0, U_BELOW_ONE, 1.0, 0.5 + 1.0 / 128, 0.0, U_BELOW_ONE, 1.0, 0.37], dtype=F)
    return lg, u


@functools.lru_cache(maxsize=2)
def sampling_operands(name):
    """Identity action weights (logits = the first 64 features, exactly, in any precision), a random value head."""
    c = by_name(name)
    rs = _rs(name, "random")
    lg, u = sampling_rows()
    K, A, B = c["K"], c["A"], c["B"]
    x = np.zeros((B, K), F)
    x[:, :A] = lg
    w0 = np.zeros((A, K), F)
    w0[np.arange(A), np.arange(A)] = 1.0
    w1, b1 = _draw(rs, "random", (1, K), 1.0 / np.sqrt(K)), _draw(rs, "random", (1,), 0.1)
    b0 = np.zeros(A, F)
    logits, v = heads_ref(x, w0, b0, w1, b1)
    assert np.array_equal(logits, lg.astype(D))
    ref = head_ref(logits, None, np.zeros(B, np.int64))
    sampled, margin = inverse_cdf(ref["p"], u)
    op = dict(x=x, w0=w0, b0=b0, w1=w1, b1=b1, u=u, logits=logits, v=v[:, 0], p=ref["p"], ent=ref["entropy"], sampled=sampled,
              margin=margin, lp_sampled=np.take_along_axis(ref["logp"], sampled[:, None], 1)[:, 0])
    if c["kind"] == "sample_fold28":        # the features as slab 3 of 28, all else +0: the fold returns them exactly
        slabs = np.zeros((28, B, K), F)
        slabs[3] = x
        op.update(slabs=slabs, bias=np.zeros(K, F))
        assert np.array_equal(fold_np(slabs, op["bias"])[0], x)
    return op


@functools.lru_cache(maxsize=2)
def riding_operands(name):
    """uint8 frames [B, 4, 84, 84], conv1's weights (OIHW; the launch takes them as [C][KH][KW][OC]), and the head's operands:
    features [B, 512] (a ReLU output) for the plain mode, 28 slabs + bias for the fold."""
    c = by_name(name)
    rs = _rs("riding-%d" % c["B"], "random")        # the modes of one batch share frames and weights
    B, A = c["B"], c["A"]
    frames = rs.randint(0, 256, size=(B, 4, 84, 84)).astype(np.uint8)
    w1c, b1c = (0.05 * rs.standard_normal((32, 4, 8, 8))).astype(F), (0.05 * rs.standard_normal(32)).astype(F)
    slabs = (rs.standard_normal((28, B, 512)) / np.sqrt(28)).astype(F)
    bias = (0.5 * rs.standard_normal(512)).astype(F)
    slabs[:, :, 0:4], bias[0:4] = F(0.0), F(0.0)
    slabs[:, :, 4:8], bias[4:8] = F(-0.0), F(-0.0)
    phi_fold, _ = fold_np(slabs, bias)
    phi_plain = relu_features(rs, (B, 512))
    w0 = (rs.standard_normal((A, 512)) * 2.5 / np.sqrt(256)).astype(F)
    w1 = (rs.standard_normal((1, 512)) / np.sqrt(256)).astype(F)
    b0, b1 = (0.1 * rs.standard_normal(A)).astype(F), (0.1 * rs.standard_normal(1)).astype(F)
    op = dict(frames=frames, w1c=w1c, b1c=b1c, slabs=slabs, bias=bias, w0=w0, b0=b0, w1=w1, b1=b1, phi_fold=phi_fold, phi_plain=phi_plain)
    if c["mode"] != "none":
        phi = phi_plain if c["mode"] == "plain" else phi_fold
        op["b0"], op["b1"] = b0, b1 = _anchor(b0, phi[0], w0[0]), _anchor(b1, phi[0], w1[0])
        logits, v = heads_ref(phi, w0, b0, w1, b1)
        ref = head_ref(logits, None, np.zeros(B, np.int64))
        u = rs.rand(B).astype(F)
        u[B - 1] = 1.0
        u = settle_uniforms(ref["p"], u, cdf_threshold(logits))
        sampled, margin = inverse_cdf(ref["p"], u)
        op.update(phi=phi, u=u, logits=logits, v=v[:, 0], p=ref["p"], ent=ref["entropy"], sampled=sampled, margin=margin,
                  lp_sampled=np.take_along_axis(ref["logp"], sampled[:, None], 1)[:, 0])
    return op


def fc4_ref(op, dtype=D):
    """phi = relu(y3 W4^T + b4), then the head on it for the given actions, one chain in `dtype`."""
    phi = np.maximum(op["y3"].astype(dtype) @ op["w4"].astype(dtype).T + op["b4"].astype(dtype), 0)
    logits, v = heads_ref(phi, op["w0"], op["b0"], op["w1"], op["b1"], dtype=dtype)
    ref = head_ref(logits, None, op["action"], dtype=dtype)
    return dict(phi=phi, logits=logits, v=v[:, 0], log_pi_a=ref["log_pi_a"], entropy=ref["entropy"])


@functools.lru_cache(maxsize=2)
def fc4_operands(name):
    c = by_name(name)
    rs = _rs(name, "random")
    B, A = c["B"], c["A"]
    op = dict(y3=relu_features(rs, (B, 3136)), w4=(rs.standard_normal((512, 3136)) / np.sqrt(1568)).astype(F),
              b4=(0.1 * rs.standard_normal(512)).astype(F), w0=(rs.standard_normal((A, 512)) * 2.5 / np.sqrt(256)).astype(F),
              w1=(rs.standard_normal((1, 512)) / np.sqrt(256)).astype(F), b0=(0.1 * rs.standard_normal(A)).astype(F),
              b1=(0.1 * rs.standard_normal(1)).astype(F), action=rs.randint(0, A, size=B).astype(np.int64))
    phi0 = fc4_ref(dict(op, y3=op["y3"][:1], action=op["action"][:1]))["phi"][0]
    op["b0"][0] = F(ANCHOR - float(phi0 @ op["w0"][0].astype(D)))
    op["b1"][0] = F(ANCHOR - float(phi0 @ op["w1"][0].astype(D)))
    op["want"] = fc4_ref(op)
    return op


@functools.lru_cache(maxsize=2)
def net_operands(name, dtype=torch.float64):
    """Parameters of CategoricalActorCriticNet(FCBody(state_dim, (hidden,), gate)) as float32 arrays, the input, given actions,
    uniforms, output gradients, and the float64 torch clone's results: plain nn.functional.linear and
    torch.distributions.Categorical.  Sampled cases: `sampled` is the float64 inverse CDF of u; the clone then evaluates the
    action handed to net_ref."""
    c = by_name(name)
    rs = _rs(name, "random")
    B, S, H, A = c["B"], c["state_dim"], c["hidden"], c["A"]
    p = dict(wb=(rs.standard_normal((H, S)) / np.sqrt(S)).astype(F), bb=(0.1 * rs.standard_normal(H)).astype(F),
             wa=(rs.standard_normal((A, H)) * 2.5 / np.sqrt(H)).astype(F), ba=(0.1 * rs.standard_normal(A)).astype(F),
             wc=(rs.standard_normal((1, H)) / np.sqrt(H)).astype(F), bc=(0.1 * rs.standard_normal(1)).astype(F))
    x = rs.standard_normal((B, S)).astype(F)
    action = rs.randint(0, A, size=B).astype(np.int64)
    g = {k: rs.standard_normal(B).astype(F) for k in _G}
    op = dict(params=p, x=x, action=action, **g)
    ref = net_ref(op, c, action)
    u = rs.rand(B).astype(F)
    u[B - 1] = 1.0
    u = settle_uniforms(ref["p"], u, cdf_threshold(ref["logits"]))
    sampled, margin = inverse_cdf(ref["p"], u)
    op.update(u=u, sampled=sampled, margin=margin, logits=ref["logits"], p=ref["p"], relu_margin=ref["relu_margin"])
    return op


def net_ref(op, c, action, dtype=torch.float64):
    """The clone: forward at `action`, backward of sum(g_lp log_pi_a + g_ent entropy + g_v v) -> values and gradients."""
    t = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in op["params"].items()}
    x = torch.tensor(op["x"], dtype=dtype, requires_grad=True)
    pre = torch.nn.functional.linear(x, t["wb"], t["bb"])
    phi = torch.relu(pre) if c["gate"] == "relu" else torch.tanh(pre)
    logits = torch.nn.functional.linear(phi, t["wa"], t["ba"])
    v = torch.nn.functional.linear(phi, t["wc"], t["bc"])[:, 0]
    dist = torch.distributions.Categorical(logits=logits)
    lp, ent = dist.log_prob(torch.from_numpy(np.asarray(action, dtype=np.int64))), dist.entropy()
    loss = sum((torch.tensor(op[k], dtype=dtype) * o).sum() for k, o in zip(_G, (lp, ent, v)))
    loss.backward()
    out = dict(log_pi_a=lp, entropy=ent, v=v, logits=logits, p=dist.probs, dx=x.grad, **{"d" + k: t[k].grad for k in t})
    out = {k: o.detach().numpy().astype(np.float64) for k, o in out.items()}
    out["relu_margin"] = float(pre.detach().abs().min()) if c["gate"] == "relu" else float("inf")
    return out


def int_bound(c):
    """Largest |partial sum| any summation order can meet on the integer set: operands in [-4, 4], 16 per term over the case's
    longest reduction (K forward; the batch or the output count backward), + 4 for a bias.  Below 2^24: exact in float32."""
    terms = c["K"] if c in FWD_CASES else max(c["B"], c["O0"] + c["O1"])
    return 16 * terms + 4
