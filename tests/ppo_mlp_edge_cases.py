"""Edge-shape cases, float64 references and bars for csrc/ppo_mlp.hip: the persistent PPO update (dra_ppo_mlp_update), the minibatch
pack (dra_ppo_mlp_pack), the one-launch rollout with its value kernel (dra_ppo_mlp_rollout) and the three stand-alone kernels.
NOT a test file: CPU only, no product code imported.  tests/test_ppo_mlp_edge_cases_host.py proves on the CPU that every case
reaches the path it is named for, that its inputs carry the bars and that its KL gates are unambiguous;
tests/test_gpu_ppo_mlp_edges.py holds the kernels to it.

References
  update   oracle.ppo_mlp_oracle.ppo_update in float64, one call per minibatch with the optimizer state carried through its
           opt_state argument (the same arithmetic as one call over all minibatches -- the host test checks that to the bit -- and
           it yields every minibatch's approx_kl).  Parameters, moments and entries are float64 tensors built from their float32
           values; lr, betas, eps, ratio_clip and entropy_weight are rounded to float32 first, as the kernel holds them.
  pack     pack_reference: a numpy restatement of the packed image from the comment above ppo_pack_kernel.
  rollout  oracle.ppo_mlp_oracle.rollout(forward_dtype=torch.float64).

Bars (those of tests/test_gpu_ppo_mlp.py, not tuned to the kernels)
  param        max |got - want| <= 1e-5 x max(max |want|, 1e-2) per tensor
  exp_avg      1e-5 of the tensor's largest magnitude, floor 1e-6;   exp_avg_sq  2e-5, floor 1e-10
  scalar       the three loss scalars: 1e-5 relative, floor 0.1
  inter        first-minibatch intermediates and gradients: 1e-5 of the tensor's largest magnitude (floor 1e-6); approx_kl 1e-4
  rollout      state, action, log_pi_a, v: 1e-5 x max(max |want|, 1)
  exact        rewards, masks, counters, sampler step, Adam step counts, pack output, dra_rms_normalize, dra_cont_env_step
  sample       dra_gauss_sample: 1e-5 absolute;   running statistics after a rollout: rtol 1e-7
BAR_OVERRIDES is where a tensor whose INPUTS cannot carry its bar would get max(bar, 4 x the error of the float32 CPU run of the
same reference), with both figures beside it.  It is empty: every case's float32 CPU run stays within 0.3 x every bar."""
import functools
from collections import OrderedDict

import numpy as np
import torch

from oracle import ppo_mlp_oracle as O
from oracle.numerics_oracle import MeanStdNormalizerOracle

# (case name, group) -> (bar as a multiple of the group's bar, float32-CPU-run error as a multiple of the group's bar)
BAR_OVERRIDES = {}
BAR_GROUPS = ("param", "exp_avg", "exp_avg_sq", "scalar", "inter", "rollout")
HOST_FRACTION = 0.3          # the float32 CPU run of the reference must stay within this fraction of every bar

K_ROWS, K_MAX_S, K_MAX_A, K_LD3 = 64, 64, 16, 20          # kRows, kMaxS, kMaxA, kLd3 of csrc/ppo_mlp.hip
AUX_LP, AUX_ADV, AUX_RET = 16, 17, 18
LDS_FLOATS_MAX = 160 * 1024 // 4
PACK_GRID_CAP, PACK_BLOCK = 8192, 256
RATIO_CLIP, ENTROPY_WEIGHT = 0.2, 0.01
LR_ACTOR, LR_CRITIC, BETAS, EPS = 3e-4, 1e-3, (0.9, 0.999), 1e-8
# debug dump layout (floats, per role; the critic's region starts at DBG['role'])
DBG = dict(role=32768, h1=0, h2=4096, head=8192, lp=9216, gl=9280, scal=9344, dz3=10240, dz2=11264, dz1=15360, w1=19456, w2=23552,
           w3=27648, b1=28672, b2=28736, b3=28800, std=28816)

_f32 = lambda x: float(np.float32(x))


def hyper():
    """The scalar hyperparameters as the kernel holds them: rounded to float32."""
    return dict(lr_actor=_f32(LR_ACTOR), lr_critic=_f32(LR_CRITIC), betas=(_f32(BETAS[0]), _f32(BETAS[1])), eps=_f32(EPS),
                ratio_clip=_f32(RATIO_CLIP), entropy_weight=_f32(ENTROPY_WEIGHT))


# ------------------------------------------------------------------------------------------------ shapes
def update_lds_floats(H, S):
    """update_lds_floats of csrc/ppo_mlp.hip."""
    return 2 * K_ROWS * (16 * ((S + 15) // 16) + 4 + K_LD3) + 2 * K_ROWS * (H + 4) + 3 * H * (K_ROWS + 4) + H * (H + 4) + \
        16 * (H + 4) + K_ROWS * K_LD3 + 16 * (K_ROWS + 4) + 16 + 16 + 32 + 256


def supported(S, A, H, MB):
    """dra_ppo_mlp_supported's conditions."""
    return 1 <= S <= K_MAX_S and 1 <= A <= K_MAX_A and H in (16, 32, 64) and 1 <= MB <= K_ROWS and update_lds_floats(H, S) <= LDS_FLOATS_MAX


def update_shape(c):
    """What the launcher and the kernel derive from a case's sizes: the instantiations <H, MODE, SC> it runs, the tile counts and
    the rows of the last minibatch of an epoch."""
    S, A, H, MB, n, epochs = c['S'], c['A'], c['H'], c['MB'], c['n'], c['epochs']
    SC = S if (H == 64 and S in (17, 11)) else 0
    per_epoch = (n + MB - 1) // MB
    rows_last = n - (per_epoch - 1) * MB
    # MFMA steps (tk, r) of the first layer that a compiled-in observation size skips: all four k = 16 tk + 4 g + r past SC
    skipped = [(tk, r) for tk in range((S + 15) // 16) for r in range(4) if SC and not 16 * tk + r < SC]
    return dict(S=S, A=A, H=H, MB=MB, n=n, epochs=epochs, SC=SC, KT1=(S + 15) // 16, NT=H // 16, MT=(MB + 15) // 16,
                per_epoch=per_epoch, total=per_epoch * epochs, rows_last=rows_last, MT_last=(rows_last + 15) // 16,
                s2_steps=(A + 3) // 4, product=(H, 0, SC), debug=(H, 1, 0), lds=update_lds_floats(H, S), skipped=skipped,
                launches=c['launches'], steps0=c['steps0'])


def rollout_shape(c):
    H, N, S, A, T = c['H'], c['N'], c['S'], c['A'], c['T']
    return dict(H=H, N=N, S=S, A=A, T=T, horizon=c['horizon'], comps=N * S, tiers=1 + (N * S > 512) + (N * S > 1024),
                pow2=N & (N - 1) == 0, chunks=(N + 7) // 8, MT=(N + 15) // 16, NT=H // 16, idle_heads=max(0, (N + 15) // 16 - H // 16),
                rows_a=T * N, rows=(T + 1) * N, blocks=((T + 1) * N + K_ROWS - 1) // K_ROWS, env0=c['env0'], n_global=c['n_global'],
                rms_update=c['rms_update'])


# ------------------------------------------------------------------------------------------------ update cases
def _u(name, S, A, H, MB, n, epochs, seed, path, target_kl=1e9, drift=0.06, std0=None, steps0=(0, 0), warm=False, launches=1, why=""):
    return dict(name=name, S=S, A=A, H=H, MB=MB, n=n, epochs=epochs, seed=seed, path=path, target_kl=target_kl, drift=drift,
                std0=std0, steps0=steps0, warm=warm, launches=launches, why=why)


# (state, action, hidden, minibatch, n, epochs); `path`: the predicate on update_shape() that proves the case reaches what it is
# named for; `seed`: chosen by tests/test_ppo_mlp_edge_cases_host.py's rules (float32 CPU run within 0.3 x every bar, gates clear)
UPDATE_CASES = [
    # hidden 16: <16,0,0> and <16,1,0>
    _u("h16-s1-a1-mb1-n1-smallest-everything", 1, 1, 16, 1, 1, 2, 101, lambda s: s['n'] == 1 and s['MT'] == 1 and s['KT1'] == 1 and s['s2_steps'] == 1),
    _u("h16-s15-a4-mb15-remainder-one-row", 15, 4, 16, 15, 31, 1, 2, lambda s: s['rows_last'] == 1 and s['KT1'] == 1 and s['s2_steps'] == 1 and s['MT'] == 1),
    _u("h16-s16-a5-mb16-full-tile", 16, 5, 16, 16, 40, 1, 103, lambda s: s['KT1'] == 1 and s['S'] % 16 == 0 and s['s2_steps'] == 2 and s['MB'] % 16 == 0),
    _u("h16-s17-a16-mb17-second-k-tile-of-one", 17, 16, 16, 17, 34, 2, 504, lambda s: s['KT1'] == 2 and s['s2_steps'] == 4 and s['MT'] == 2 and s['rows_last'] == s['MB']),
    _u("h16-s33-a6-mb33-remainder-drops-a-tile", 33, 6, 16, 33, 49, 1, 5, lambda s: s['KT1'] == 3 and s['MT'] == 3 and s['rows_last'] == 16 and s['MT_last'] == 1),
    _u("h16-s64-a2-mb63-largest-observation", 64, 2, 16, 63, 64, 1, 6, lambda s: s['KT1'] == 4 and s['MT'] == 4 and s['MB'] == 63 and s['rows_last'] == 1),
    # hidden 32: <32,0,0> and <32,1,0>
    _u("h32-s1-a4-mb64-n3-fewer-rows-than-minibatch", 1, 4, 32, 64, 3, 2, 7, lambda s: s['n'] < s['MB'] and s['per_epoch'] == 1 and s['rows_last'] == 3),
    _u("h32-s15-a5-mb17-remainder-one-row", 15, 5, 32, 17, 35, 1, 8, lambda s: s['rows_last'] == 1 and s['MT'] == 2 and s['s2_steps'] == 2),
    _u("h32-s16-a16-mb63", 16, 16, 32, 63, 130, 1, 109, lambda s: s['MT'] == 4 and s['MB'] == 63 and s['s2_steps'] == 4 and s['rows_last'] == 4),
    _u("h32-s17-a1-mb1-one-row-minibatches", 17, 1, 32, 1, 5, 1, 10, lambda s: s['MB'] == 1 and s['total'] == 5 and s['KT1'] == 2),
    _u("h32-s33-a3-mb15", 33, 3, 32, 15, 45, 1, 11, lambda s: s['KT1'] == 3 and s['MT'] == 1 and s['MB'] == 15),
    _u("h32-s64-a9-mb33-remainder-drops-a-tile", 64, 9, 32, 33, 82, 1, 12, lambda s: s['KT1'] == 4 and s['MT'] == 3 and s['rows_last'] == 16 and s['MT_last'] == 1),
    # hidden 64: <64,0,0>, <64,0,17>, <64,0,11> and <64,1,0>
    _u("h64-s1-a5-mb16-remainder-one-row", 1, 5, 64, 16, 33, 1, 13, lambda s: s['product'] == (64, 0, 0) and s['rows_last'] == 1 and s['s2_steps'] == 2),
    _u("h64-s11-a3-mb15-compiled-11", 11, 3, 64, 15, 31, 2, 114, lambda s: s['product'] == (64, 0, 11) and s['KT1'] == 1 and s['rows_last'] == 1),
    _u("h64-s11-a16-mb1-n1-compiled-11", 11, 16, 64, 1, 1, 1, 115, lambda s: s['product'] == (64, 0, 11) and s['n'] == 1 and s['s2_steps'] == 4),
    _u("h64-s16-a4-mb64-n3-fewer-rows-than-minibatch", 16, 4, 64, 64, 3, 1, 16, lambda s: s['product'] == (64, 0, 0) and s['n'] < s['MB'] and s['s2_steps'] == 1),
    _u("h64-s17-a6-mb33-compiled-17-remainder-drops-a-tile", 17, 6, 64, 33, 49, 1, 117,
       lambda s: s['product'] == (64, 0, 17) and s['skipped'] == [(1, 1), (1, 2), (1, 3)] and s['rows_last'] == 16 and s['MT_last'] == 1),
    _u("h64-s32-a16-mb17-two-full-k-tiles", 32, 16, 64, 17, 51, 1, 1418, lambda s: s['product'] == (64, 0, 0) and s['KT1'] == 2 and s['S'] % 16 == 0),
    _u("h64-s33-a1-mb63-remainder-one-row", 33, 1, 64, 63, 127, 1, 319, lambda s: s['product'] == (64, 0, 0) and s['KT1'] == 3 and s['rows_last'] == 1),
    _u("h64-s48-a2-mb64-largest-the-lds-admits", 48, 2, 64, 64, 130, 1, 20,
       lambda s: s['product'] == (64, 0, 0) and s['KT1'] == 3 and supported(48, 2, 64, 64) and not supported(49, 2, 64, 64)),
]
# further update cases (one test each in tests/test_gpu_ppo_mlp_edges.py)
CONTINUATION_CASE = _u("continuation-h32-s15-a5-two-launches", 15, 5, 32, 17, 40, 1, 31, lambda s: s['launches'] == 2, launches=2,
                       why="a second launch on the same device buffers with fresh entries: non-zero moments and step counts from the device")
WARM_CASE = _u("warm-start-h64-s17-a6-steps-5000-4990", 17, 6, 64, 64, 130, 1, 32, lambda s: s['steps0'] == (5000, 4990) and s['product'] == (64, 0, 17),
               steps0=(5000, 4990), warm=True, why="preloaded non-zero moments and step counts: pow(beta, t0) and a bias correction near 1")
GATE_CLOSED_CASE = _u("gate-closed-from-the-start-h64-s11", 11, 3, 64, 32, 70, 1, 33, lambda s: s['total'] == 3, target_kl=0.01, drift=0.04,
                      why="approx_kl 0.07 at the first minibatch and at least 0.03 at every one, against a limit of 0.015: the actor comes back bit-identical")
GATE_MIDWAY_CASE = _u("gate-closes-midway-h16-s15-a4", 15, 4, 16, 32, 128, 3, 834, lambda s: s['H'] == 16 and s['total'] == 12, target_kl=0.001, drift=0.0,
                      why="behaviour policy = initial policy: the gate is open at first and closes once the policy has drifted")
STD_SWEEP = (-3.0, -2.0, 0.5413, 5.0, 19.5, 20.5)
# (mean drift as a multiple of softplus(std), seed) per std: approx_kl of the one minibatch in [0.005, 0.1], >= 4 rows inside
# and >= 4 outside the clip range (proved by the host test)
_STD_DRIFT = {-3.0: (0.06, 141), -2.0: (0.045, 2942), 0.5413: (0.02, 43), 5.0: (0.03, 244), 19.5: (0.02, 1245), 20.5: (0.02, 46)}
STD_CASES = [_u("std%+g-h64-s17-a6-mb64" % s, 17, 6, 64, 64, 64, 1, _STD_DRIFT[s][1], lambda sh: sh['total'] == 1 and sh['product'] == (64, 0, 17),
                drift=_STD_DRIFT[s][0], std0=s) for s in STD_SWEEP]
ALL_UPDATE_CASES = UPDATE_CASES + [CONTINUATION_CASE, WARM_CASE, GATE_CLOSED_CASE, GATE_MIDWAY_CASE] + STD_CASES

# (argument overrides, what is wrong) -- dra_ppo_mlp_supported and the launchers answer DRA_EINVAL, nothing launched
UPDATE_REFUSALS = [
    (dict(S=0), "state 0"), (dict(S=65), "state 65"), (dict(S=49, H=64), "hidden 64 with state 49: LDS"), (dict(A=0), "action 0"),
    (dict(A=17), "action 17"), (dict(H=48), "hidden 48"), (dict(MB=0), "minibatch 0"), (dict(MB=65), "minibatch 65"),
    (dict(off_std=-1), "actor without std"), (dict(eps=0.0), "eps 0"), (dict(beta1=1.0), "beta1 1"),
]


def _softplus(x):
    return float(torch.nn.functional.softplus(torch.tensor(float(x), dtype=torch.float64)))


def _inv_softplus(y):
    return float(y + np.log(-np.expm1(-y)))


def _rollout_rows(rs, n, S, A, actor, critic):
    """Rollout-like rows drawn from the behaviour policy (actor, critic): (state, action, log_pi_a, ret, advantage), float32."""
    state = torch.from_numpy(rs.randn(n, S).astype(np.float32))
    with torch.no_grad():
        pred = O.gaussian_forward(actor, critic, state, noise=torch.from_numpy(rs.randn(n, A).astype(np.float32)))
    adv = torch.from_numpy(rs.randn(n, 1).astype(np.float32))
    ret = pred['v'].detach() + torch.from_numpy(rs.randn(n, 1).astype(np.float32))
    return [state, pred['action'].detach(), pred['log_pi_a'].detach(), ret, adv]


@functools.lru_cache(maxsize=None)
def _update_inputs(name):
    c = CASES_BY_NAME[name]
    S, A, H, n = c['S'], c['A'], c['H'], c['n']
    rs = np.random.RandomState(1000 + c['seed'])
    actor, critic = O.init_params(S, A, H, seed=c['seed'])
    actor = OrderedDict((k, v.detach().clone()) for k, v in actor.items())
    critic = OrderedDict((k, v.detach().clone()) for k, v in critic.items())
    behaviour = OrderedDict((k, v.clone()) for k, v in actor.items())
    if c['std0'] is not None:
        # the std sweep: the policy's std is the swept value exactly; the behaviour policy's scale is 5% smaller and the mean
        # drifts by a multiple of the scale, so that approx_kl does not depend on where in the sweep the case sits
        sp = _softplus(c['std0'])
        actor['std'].fill_(c['std0'])
        behaviour['std'].fill_(_inv_softplus(0.95 * sp))
        noise_w, noise_b = rs.randn(A, H).astype(np.float32), rs.randn(A).astype(np.float32)
        scale = min(c['drift'] * sp, 0.12)         # (the mean is a tanh: a larger drift of its argument saturates it)
        actor['w3'].add_(torch.from_numpy(noise_w) * scale)
        actor['b3'].add_(torch.from_numpy(noise_b) * scale)
    launches = []
    for _ in range(c['launches']):
        entries = _rollout_rows(rs, n, S, A, behaviour, critic)
        perms = [rs.permutation(n) for _ in range(c['epochs'])]
        launches.append((entries, perms))
    if c['std0'] is None and c['drift']:
        # move the policy so that ratios differ from 1 and some rows sit outside the clip range
        actor['w3'].add_(c['drift'] * torch.from_numpy(rs.randn(A, H).astype(np.float32)))
        actor['std'].add_(0.1)
    moments = None
    if c['warm']:
        # moments of the size a run leaves behind: exp_avg ~ gradient, exp_avg_sq ~ gradient squared
        moments = {}
        for role, params in (("actor", actor), ("critic", critic)):
            moments[role] = ({k: torch.from_numpy((rs.randn(*v.shape) * 1e-2).astype(np.float32)) for k, v in params.items()},
                             {k: torch.from_numpy((rs.uniform(0.5, 2.0, size=tuple(v.shape)) * 1e-4).astype(np.float32)) for k, v in params.items()})
    return dict(actor=actor, critic=critic, launches=launches, moments=moments)


def update_inputs(c):
    """The float32 inputs of an update case: actor / critic OrderedDicts, per launch (entries, perms), and for a warm start the
    (exp_avg, exp_avg_sq) dicts per role.  Cached: do not modify."""
    return _update_inputs(c['name'])


def _opt_state(params, moments, step, lr, h):
    opt = torch.optim.Adam(list(params.values()), lr, betas=h['betas'], eps=h['eps'])
    for (k, p) in params.items():
        opt.state[p] = dict(step=torch.tensor(float(step)), exp_avg=moments[0][k].to(p.dtype).clone(), exp_avg_sq=moments[1][k].to(p.dtype).clone())
    return opt.state_dict()


def _moments_of(opt, params):
    m, v = {}, {}
    for k, p in params.items():
        st = opt.state.get(p, None)
        m[k] = st['exp_avg'].detach().numpy().copy() if st else np.zeros(tuple(p.shape), dtype=p.detach().numpy().dtype)
        v[k] = st['exp_avg_sq'].detach().numpy().copy() if st else np.zeros(tuple(p.shape), dtype=p.detach().numpy().dtype)
    return m, v


def _first_numpy(first):
    out = {}
    for k, v in first.items():
        if isinstance(v, list):
            out[k] = [g.numpy().astype(np.float64) for g in v]
        elif torch.is_tensor(v):
            out[k] = v.numpy().astype(np.float64)
        else:
            out[k] = float(v)
    return out


def run_reference(c, dtype=torch.float64, per_minibatch=True):
    """The reference run of an update case in `dtype` -> dict(launches=[state after each launch], first=the first minibatch's
    intermediates and gradients, kls=[approx_kl of every minibatch]).  A launch's state: actor / critic {name: array}, m / v
    {role: {name: array}}, steps (Adam step counts), counts (steps of this launch), out3."""
    inp, h = update_inputs(c), hyper()
    actor = OrderedDict((k, v.to(dtype).clone().requires_grad_(True)) for k, v in inp['actor'].items())
    critic = OrderedDict((k, v.to(dtype).clone().requires_grad_(True)) for k, v in inp['critic'].items())
    opt_state = None
    if c['warm']:
        opt_state = (_opt_state(actor, inp['moments']['actor'], c['steps0'][0], h['lr_actor'], h),
                     _opt_state(critic, inp['moments']['critic'], c['steps0'][1], h['lr_critic'], h))
    kw = dict(lr_actor=h['lr_actor'], lr_critic=h['lr_critic'], betas=h['betas'], eps=h['eps'])
    steps = list(c['steps0'])
    MB = c['MB']
    out, first, kls = [], {}, []
    for entries, perms in inp['launches']:
        ent = [e.to(dtype) for e in entries]
        counts, out3 = [0, 0], None
        if per_minibatch:
            for perm in perms:
                for k0 in range(0, c['n'], MB):
                    idx = torch.from_numpy(np.asarray(perm[k0:k0 + MB], dtype=np.int64))
                    sub = [e[idx] for e in ent]
                    aopt, copt, out3, a_steps = O.ppo_update(actor, critic, sub, [np.arange(len(idx))], MB, h['ratio_clip'], h['entropy_weight'],
                                                             c['target_kl'], opt_state=opt_state, first=first if not kls else None, **kw)
                    opt_state = (aopt.state_dict(), copt.state_dict())
                    kls.append(out3[2])
                    counts[0] += a_steps
                    counts[1] += 1
        else:
            aopt, copt, out3, a_steps = O.ppo_update(actor, critic, ent, perms, MB, h['ratio_clip'], h['entropy_weight'], c['target_kl'],
                                                     opt_state=opt_state, **kw)
            opt_state = (aopt.state_dict(), copt.state_dict())
            counts = [a_steps, len(perms) * ((c['n'] + MB - 1) // MB)]
        steps = [steps[0] + counts[0], steps[1] + counts[1]]
        ma, va = _moments_of(aopt, actor)
        mc, vc = _moments_of(copt, critic)
        out.append(dict(actor={k: v.detach().numpy().copy() for k, v in actor.items()},
                        critic={k: v.detach().numpy().copy() for k, v in critic.items()},
                        m=dict(actor=ma, critic=mc), v=dict(actor=va, critic=vc), steps=tuple(steps), counts=tuple(counts),
                        out3=tuple(float(x) for x in out3)))
    return dict(launches=out, first=_first_numpy(first), kls=kls)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return run_reference(CASES_BY_NAME[name])


def reference(c):
    """The float64 reference of an update case, computed once and shared.  Do not modify."""
    return _reference(c['name'])


# ------------------------------------------------------------------------------------------------ bars
def _a(x):
    return np.asarray(x, dtype=np.float64)


def ratio(kind, got, want):
    """The error of `got` against `want` as a multiple of the bar of its kind (<= 1 passes)."""
    got, want = _a(got), _a(want)
    if got.shape != want.shape:
        return float("inf")
    if not got.size:
        return 0.0
    err = float(np.max(np.abs(got - want)))
    if not np.isfinite(got).all():
        return float("inf")
    big = float(np.max(np.abs(want)))
    if kind == "param":
        return err / (1e-5 * max(big, 1e-2))
    if kind == "exp_avg":
        return err / (1e-5 * max(big, 1e-6))
    if kind == "exp_avg_sq":
        return err / (2e-5 * max(big, 1e-10))
    if kind == "scalar":
        return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 0.1))) / 1e-5
    if kind == "inter":
        return err / (1e-5 * max(big, 1e-6))
    if kind == "kl":
        return err / (1e-4 * max(big, 1e-6))
    if kind == "rollout":
        return err / (1e-5 * max(big, 1.0))
    if kind == "sample":
        return err / 1e-5
    raise KeyError(kind)


def bar(case_name, group):
    """1, or the entry of BAR_OVERRIDES: the multiple of the group's bar a case's measured ratio may reach.  Groups: "param",
    "exp_avg", "exp_avg_sq", "scalar" (a launch's state), "inter" (every first-minibatch intermediate and gradient, approx_kl
    included), "rollout"."""
    assert group in BAR_GROUPS, group
    return BAR_OVERRIDES.get((case_name, group), (1.0, 0.0))[0]


def compare_state(got, want):
    """Worst ratios of a launch's state (the format of run_reference's launches) -> {group: (ratio, tensor name)}."""
    worst = {}

    def put(group, r, name):
        if group not in worst or r > worst[group][0]:
            worst[group] = (r, name)
    for role in ("actor", "critic"):
        for k, w in want[role].items():
            put("param", ratio("param", got[role][k], w), role + "." + k)
            put("exp_avg", ratio("exp_avg", got['m'][role][k], want['m'][role][k]), role + "." + k)
            put("exp_avg_sq", ratio("exp_avg_sq", got['v'][role][k], want['v'][role][k]), role + "." + k)
    put("scalar", ratio("scalar", got['out3'], want['out3']), "out3")
    return worst


FIRST_KEYS = ("h1a", "h2a", "h1c", "h2c", "mean", "v", "log_pi_a", "g_log_pi_a", "g_v", "policy_loss", "value_loss")
GRAD_NAMES = ("dW1", "db1", "dW2", "db2", "dW3", "db3", "dstd")


def compare_first(got, want, keys=None):
    """Worst ratios of the first minibatch's intermediates and gradients (the format of run_reference's `first`)."""
    worst = {}
    for k in FIRST_KEYS:
        if keys is None or k in keys:
            worst[k] = ratio("inter", got[k], want[k])
    for role in ("actor", "critic"):
        for name, g, w in zip(GRAD_NAMES, got[role + "_grads"], want[role + "_grads"]):
            if keys is None or role + "." + name in keys:
                worst[role + "." + name] = ratio("inter", g, w)
    if keys is None or "approx_kl" in keys:
        worst["approx_kl"] = ratio("kl", got['approx_kl'], want['approx_kl'])
    return worst


def decode_dump(dbg, c, rows):
    """The debug instantiation's dump of minibatch 0 (float32 [2 x DBG['role']]) in the format of run_reference's `first`, plus
    'padding': the largest magnitude found at a padded position of a dumped gradient (rows >= hidden, columns >= state, ...)."""
    S, A, H = c['S'], c['A'], c['H']
    out, pad = {}, 0.0
    for role, base, a_out in (("actor", 0, A), ("critic", DBG['role'], 1)):
        d = np.asarray(dbg[base:base + DBG['role']], dtype=np.float64)
        sq = lambda key, r, cols: d[DBG[key]:DBG[key] + r * cols].reshape(r, cols)
        sfx = role[0]
        out["h1" + sfx], out["h2" + sfx] = sq('h1', 64, 64)[:rows, :H], sq('h2', 64, 64)[:rows, :H]
        head = sq('head', 64, 16)
        if role == "actor":
            out['mean'] = head[:rows, :A]
            out['log_pi_a'] = d[DBG['lp']:DBG['lp'] + rows].reshape(-1, 1)
            out['g_log_pi_a'] = d[DBG['gl']:DBG['gl'] + rows].reshape(-1, 1)
            out['policy_loss'], out['approx_kl'] = float(d[DBG['scal']]), float(d[DBG['scal'] + 2])
        else:
            out['v'] = head[:rows, :1]
            out['g_v'] = d[DBG['gl']:DBG['gl'] + rows].reshape(-1, 1)
            out['value_loss'] = float(d[DBG['scal'] + 1])
        w1, w2, w3 = sq('w1', 64, 64), sq('w2', 64, 64), sq('w3', 16, 64)
        b1, b2 = d[DBG['b1']:DBG['b1'] + 64], d[DBG['b2']:DBG['b2'] + 64]
        b3, sd = d[DBG['b3']:DBG['b3'] + 16], d[DBG['std']:DBG['std'] + 16]
        grads = [w1[:H, :S], b1[:H], w2[:H, :H], b2[:H], w3[:a_out, :H], b3[:a_out]]
        if role == "actor":
            grads.append(sd[:A])
        out[role + "_grads"] = grads
        for full, used in ((w1, (H, S)), (w2, (H, H)), (w3, (a_out, H))):
            m = np.ones(full.shape, dtype=bool)
            m[:used[0], :used[1]] = False
            pad = max(pad, float(np.abs(full[m]).max()) if m.any() else 0.0)
        for vec, used in ((b1, H), (b2, H), (b3, a_out), (sd, A if role == "actor" else 0)):
            pad = max(pad, float(np.abs(vec[used:]).max()) if used < vec.size else 0.0)
    out['padding'] = pad
    return out


def gate_margin(kl, target_kl):
    """How far an approx_kl lies from the gate, as a multiple of the margin two correct float32 implementations need."""
    limit = 1.5 * target_kl
    return abs(kl - limit) / (1e-5 + 1e-4 * limit)


def clip_census(c):
    """(rows of the first minibatch inside the clip range, rows outside) in the float64 reference."""
    inp, ref = update_inputs(c), reference(c)
    entries, perms = inp['launches'][0]
    rows = np.asarray(perms[0][:c['MB']])
    ratio_ = np.exp(ref['first']['log_pi_a'].reshape(-1) - entries[2].numpy().astype(np.float64).reshape(-1)[rows])
    inside = (ratio_ >= 1.0 - _f32(RATIO_CLIP)) & (ratio_ <= 1.0 + _f32(RATIO_CLIP))
    return int(inside.sum()), int((~inside).sum())


# ------------------------------------------------------------------------------------------------ pack
# (S, A, mb, n, epochs)
PACK_CASES = [
    dict(name="pack-smallest", S=1, A=1, MB=1, n=1, epochs=1, seed=1, path=lambda s: s['images'] == 1 and s['passes'] == 1),
    dict(name="pack-baseline-shape-remainder-8", S=17, A=6, MB=64, n=200, epochs=2, seed=2, path=lambda s: s['rows_last'] == 8 and s['passes'] == 1),
    dict(name="pack-grid-stride", S=64, A=16, MB=1, n=190, epochs=2, seed=3,
         path=lambda s: s['images'] == 380 and s['img'] == 5632 and s['floats'] > PACK_GRID_CAP * PACK_BLOCK and s['passes'] == 2),
]


def pack_shape(c):
    ldx = 16 * ((c['S'] + 15) // 16) + 4
    img = K_ROWS * (ldx + K_LD3)
    per_epoch = (c['n'] + c['MB'] - 1) // c['MB']
    floats = c['epochs'] * per_epoch * img
    threads = min((floats + PACK_BLOCK - 1) // PACK_BLOCK, PACK_GRID_CAP) * PACK_BLOCK
    return dict(ldx=ldx, img=img, per_epoch=per_epoch, images=c['epochs'] * per_epoch, floats=floats, passes=(floats + threads - 1) // threads,
                rows_last=c['n'] - (per_epoch - 1) * c['MB'])


def pack_inputs(c):
    rs = np.random.RandomState(c['seed'])
    n, S, A = c['n'], c['S'], c['A']
    f = lambda *shape: rs.randn(*shape).astype(np.float32)
    return dict(state=f(n, S), action=f(n, A), log_pi_a=f(n, 1), advantage=f(n, 1), ret=f(n, 1),
                perm=np.stack([rs.permutation(n) for _ in range(c['epochs'])]).astype(np.int64))


def pack_reference(inp, MB):
    """The packed images, restated from the comment above ppo_pack_kernel: per minibatch [64][16 ceil(S / 16) + 4] observations
    then [64][20] = action in columns < A, log_pi_a / advantage / ret in columns 16 / 17 / 18; everything else zero."""
    state, action, perm = inp['state'], inp['action'], inp['perm']
    n, S = state.shape
    A = action.shape[1]
    ldx = 16 * ((S + 15) // 16) + 4
    per_epoch = (n + MB - 1) // MB
    out = np.zeros((perm.shape[0], per_epoch, K_ROWS * (ldx + K_LD3)), dtype=np.float32)
    for e in range(perm.shape[0]):
        for k in range(per_epoch):
            obs = np.zeros((K_ROWS, ldx), dtype=np.float32)
            aux = np.zeros((K_ROWS, K_LD3), dtype=np.float32)
            for row, src in enumerate(perm[e, k * MB:min(n, (k + 1) * MB)]):
                obs[row, :S] = state[src]
                aux[row, :A] = action[src]
                aux[row, AUX_LP], aux[row, AUX_ADV], aux[row, AUX_RET] = inp['log_pi_a'][src, 0], inp['advantage'][src, 0], inp['ret'][src, 0]
            out[e, k] = np.concatenate([obs.reshape(-1), aux.reshape(-1)])
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------ rollout cases
def _r(name, H, N, S, A, T, horizon, seed, path, env0=0, n_global=None, rms_update=1):
    return dict(name=name, H=H, N=N, S=S, A=A, T=T, horizon=horizon, seed=seed, path=path, env0=env0, n_global=n_global or N,
                rms_update=rms_update, noise_seed=100 + seed, sampler_step0=3 + seed)


# (hidden, n_env, state, action, t_len, horizon)
ROLLOUT_CASES = [
    _r("h16-smallest-everything-every-step-terminal", 16, 1, 1, 1, 1, 1, 1,
       lambda s: s['comps'] == 1 and s['T'] == 1 and s['horizon'] == 1 and s['rows'] == 2 and s['pow2']),
    _r("h16-n64-s17-three-component-tiers-idle-head-waves", 16, 64, 17, 16, 3, 2, 2,
       lambda s: s['comps'] == 1088 and s['tiers'] == 3 and s['pow2'] and s['chunks'] == 8 and s['idle_heads'] == 3 and s['rows_a'] % 64 == 0),
    _r("h32-n33-s64-five-fold-chunks-hand-over-inside-a-tile", 32, 33, 64, 5, 2, 5, 3,
       lambda s: s['comps'] == 2112 and s['tiers'] == 3 and not s['pow2'] and s['chunks'] == 5 and 0 < s['rows_a'] % 64 < 64 - 1 and s['rows'] > s['rows_a'] + 1),
    _r("h64-n64-s48-largest-workgroup-state", 64, 64, 48, 4, 2, 3, 4, lambda s: s['comps'] == 3072 and s['tiers'] == 3 and s['blocks'] == 3),
    _r("h64-n9-s11-second-fold-chunk", 64, 9, 11, 3, 6, 4, 5, lambda s: s['chunks'] == 2 and not s['pow2'] and s['tiers'] == 1),
    _r("h32-shard-env0-7-of-40", 32, 9, 17, 6, 4, 3, 6, lambda s: s['env0'] == 7 and s['n_global'] == 40 and s['n_global'] > s['N'], env0=7, n_global=40),
    _r("h16-statistics-frozen", 16, 17, 15, 2, 4, 3, 7, lambda s: s['rms_update'] == 0 and s['idle_heads'] == 1, rms_update=0),
]
# (io overrides, what is wrong)
ROLLOUT_REFUSALS = [(dict(n_env=0), "n_env 0"), (dict(n_env=65), "n_env 65"), (dict(t_len=0), "t_len 0"), (dict(horizon=0), "horizon 0"),
                    (dict(n_global=3), "n_global < n_env")]


def run_rollout(c, dtype=torch.float64):
    """The reference run of a rollout case with its forwards in `dtype` -> dict: the inputs the kernel takes (actor, critic, raw0,
    cur0, rms0, seeds), the oracle's outputs (`want`) and the final statistics, counters and sampler step."""
    H, N, S, A, T = c['H'], c['N'], c['S'], c['A'], c['T']
    actor, critic = O.init_params(S, A, H, seed=200 + c['seed'])
    actor = OrderedDict((k, v.detach().clone()) for k, v in actor.items())
    critic = OrderedDict((k, v.detach().clone()) for k, v in critic.items())
    seeds = [500 + 10 * c['seed'] + c['env0'] + i for i in range(N)]
    envs = [O.ContinuousEnvOracle(sd, S, A, c['horizon']) for sd in seeds]
    raw = np.stack([e.reset() for e in envs])
    norm = MeanStdNormalizerOracle()
    # statistics with some history behind them: three batches of the spread the environment has, then the reset observations.
    # The history sits off centre, so that no running mean ends near zero, where rtol 1e-7 would ask for more than the float32
    # actions feeding the observations carry.
    rs = np.random.RandomState(c['seed'])
    for _ in range(3):
        norm(rs.uniform(0.02, 0.18, size=(N, S)))
    cur = np.asarray(norm(raw), dtype=np.float32)
    if not c['rms_update']:
        norm.read_only = True
    rms0 = np.concatenate([norm.rms.mean.reshape(-1), norm.rms.var.reshape(-1), [norm.rms.count]]).astype(np.float64)
    want = O.rollout(actor, critic, envs, raw, norm, cur, T, c['noise_seed'], c['sampler_step0'], n_global=c['n_global'], env0=c['env0'],
                     forward_dtype=dtype)
    rms1 = np.concatenate([norm.rms.mean.reshape(-1), norm.rms.var.reshape(-1), [norm.rms.count]]).astype(np.float64)
    return dict(actor=actor, critic=critic, raw0=raw, cur0=cur, rms0=rms0, seeds=np.asarray(seeds, dtype=np.int64), want=want, rms1=rms1,
                counters=np.asarray([e.c for e in envs], dtype=np.int64), sampler_step=c['sampler_step0'] + T + 1)


@functools.lru_cache(maxsize=None)
def _rollout_reference(name):
    return run_rollout(ROLLOUTS_BY_NAME[name])


def rollout_reference(c):
    """The float64-forward reference of a rollout case, computed once and shared.  Do not modify."""
    return _rollout_reference(c['name'])


ROLLOUT_KEYS = ("state", "action", "log_pi_a", "v")


def compare_rollout(got, want):
    """{key: ratio to the rollout bar} for the four float32 outputs."""
    return {k: ratio("rollout", got[k], want[k]) for k in ROLLOUT_KEYS}


# ------------------------------------------------------------------------------------------------ stand-alone kernels
RMS_CASES = [(1, 1), (3, 257), (2, 4096)]                      # (n, d): one thread; the thread loop (d > 256); the documented limit
RMS_REFUSED_D = 4097
GAUSS_CASES = [(1, 1), (40, 32), (64, 16)]                     # (n, a_dim): 1, 1280 and 1024 elements; a_dim at its limit
GAUSS_REFUSED_A = 33
ENV_CASES = [(1030, 1, 1, 1), (3, 64, 2, 7), (5, 63, 16, 2)]   # (n, s_dim, a_dim, horizon): the grid-stride; s_dim at its limit
ENV_REFUSED_S = 65
ENV_GRID_CAP = 1024

CASES_BY_NAME = {c['name']: c for c in ALL_UPDATE_CASES}
ROLLOUTS_BY_NAME = {c['name']: c for c in ROLLOUT_CASES}
assert len(CASES_BY_NAME) == len(ALL_UPDATE_CASES) and len(ROLLOUTS_BY_NAME) == len(ROLLOUT_CASES)
