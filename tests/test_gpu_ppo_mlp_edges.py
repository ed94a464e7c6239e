"""GPU parity tests of csrc/ppo_mlp.hip at its shape and path edges, through the C ABI: every instantiation of the persistent PPO
update (product and debug), the minibatch pack, the one-launch rollout with its value kernel and the three stand-alone kernels,
against the float64 references and the bars of tests/ppo_mlp_edge_cases.py (whose cases tests/test_ppo_mlp_edge_cases_host.py
proves on the CPU: each reaches its path, its inputs carry the bars, its KL gates are clear of the limit).  Every measured maximum
goes to the parity log as a multiple of its bar."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_mlp_edge_cases as E
from parity_log import record_parity

pytestmark = pytest.mark.gpu
EINVAL = -22


def _ids(cases):
    return [c["name"] for c in cases]


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """A test that left the device in error ends the session: nothing more is launched on a faulted GPU."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test, nothing more is launched: %s" % e, returncode=3)


def _bits(t):
    """A tensor's bytes, for comparisons to the bit (NaN guard values included)."""
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().copy()


# ------------------------------------------------------------------------------------------------ device state of one network
class _DevNet:
    """One network's flat parameter / exp_avg / exp_avg_sq buffers in the layout dra_ppo_mlp_net describes: every tensor 16-byte
    aligned and followed by a guard of 64 NaN floats in all three buffers, which nothing may use or write (a first-layer operand
    load that lost its `k < S` mask reads up to 63 floats past w1: with the guard behind it the forward turns NaN)."""
    GUARD = 64

    def __init__(self, dev, params, lr, step_view, moments=None):
        from deeprl_amd.ppo_mlp import Net
        h = E.hyper()
        self.shapes = {k: tuple(v.shape) for k, v in params.items()}
        self.offs, off = {}, 0
        for k, v in params.items():
            self.offs[k] = off
            off += (v.numel() + 3) // 4 * 4 + self.GUARD
        flat = np.full(off, np.nan, dtype=np.float32)
        m, v2 = np.full(off, np.nan, dtype=np.float32), np.full(off, np.nan, dtype=np.float32)
        self.gap = np.ones(off, dtype=bool)
        for k, v in params.items():
            sl = slice(self.offs[k], self.offs[k] + v.numel())
            flat[sl] = v.detach().numpy().reshape(-1)
            self.gap[sl] = False
            m[sl], v2[sl] = 0.0, 0.0
            if moments is not None:
                m[sl], v2[sl] = moments[0][k].numpy().reshape(-1), moments[1][k].numpy().reshape(-1)
        self.param, self.m, self.v = (torch.from_numpy(x).to(dev) for x in (flat, m, v2))
        n = Net()
        n.param, n.exp_avg, n.exp_avg_sq, n.step_dev = self.param.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), step_view.data_ptr()
        o = self.offs
        n.off_w1, n.off_b1, n.off_w2, n.off_b2, n.off_w3, n.off_b3 = o['w1'], o['b1'], o['w2'], o['b2'], o['w3'], o['b3']
        n.off_std = o['std'] if 'std' in o else -1
        n.lr, n.beta1, n.beta2, n.eps = lr, h['betas'][0], h['betas'][1], h['eps']
        self.net = n

    def read(self):
        out = []
        for buf in (self.param, self.m, self.v):
            a = buf.cpu().numpy()
            out.append({k: a[o:o + int(np.prod(self.shapes[k]))].reshape(self.shapes[k]).copy() for k, o in self.offs.items()})
        for buf in (self.param, self.m, self.v):
            assert np.isnan(buf.cpu().numpy()[self.gap]).all(), "a guard between two tensors was written"
        return out

    def snapshot(self):
        return [_bits(x) for x in (self.param, self.m, self.v)]


class _Update:
    """The device side of one update case: both networks, the step counts, and launches of dra_ppo_mlp_pack + dra_ppo_mlp_update."""

    def __init__(self, dra, c):
        from deeprl_amd import ppo_mlp
        self.c, self.dev, self.inp, h = c, dra.Config.DEVICE, E.update_inputs(c), E.hyper()
        self.steps = torch.tensor(list(c['steps0']), dtype=torch.int64, device=self.dev)
        mo = self.inp['moments'] or dict(actor=None, critic=None)
        self.actor = _DevNet(self.dev, self.inp['actor'], h['lr_actor'], self.steps[0:1], mo['actor'])
        self.critic = _DevNet(self.dev, self.inp['critic'], h['lr_critic'], self.steps[1:2], mo['critic'])
        cfg = ppo_mlp.Cfg()
        cfg.state_dim, cfg.action_dim, cfg.hidden, cfg.mini_batch = c['S'], c['A'], c['H'], c['MB']
        cfg.ratio_clip, cfg.entropy_weight, cfg.kl_limit = h['ratio_clip'], h['entropy_weight'], 1.5 * c['target_kl']
        self.cfg = cfg
        self.out3 = torch.full((3,), float("nan"), dtype=torch.float32, device=self.dev)
        self.counts = torch.full((2,), -7, dtype=torch.int64, device=self.dev)
        self.packed = None

    def pack(self, li):
        from deeprl_amd._lib import lib, ptr, stream_ptr
        c = self.c
        entries, perms = self.inp['launches'][li]
        e = [x.to(self.dev).contiguous() for x in entries]       # state, action, log_pi_a, ret, advantage
        perm = torch.from_numpy(np.concatenate([np.asarray(p, dtype=np.int64) for p in perms])).to(self.dev)
        floats = ctypes.c_int64()
        lib.dra_ppo_mlp_packed_floats(c['n'], c['epochs'], c['MB'], c['S'], ctypes.byref(floats))
        self.packed = torch.full((floats.value,), float("nan"), dtype=torch.float32, device=self.dev)
        lib.dra_ppo_mlp_pack(ptr(e[0]), ptr(e[1]), ptr(e[2]), ptr(e[4]), ptr(e[3]), ptr(perm), c['n'], c['epochs'], c['MB'], c['S'], c['A'],
                             ptr(self.packed), stream_ptr())

    def launch(self, li=0, dbg=False):
        """-> (the state after the launch in the format of E.run_reference's launches, the debug dump or None)."""
        from deeprl_amd import ppo_mlp
        from deeprl_amd._lib import lib, ptr, stream_ptr
        self.pack(li)
        dbg_t = torch.zeros(ppo_mlp.DBG_FLOATS, dtype=torch.float32, device=self.dev) if dbg else None
        lib.dra_ppo_mlp_update(ctypes.byref(self.cfg), ctypes.byref(self.actor.net), ctypes.byref(self.critic.net), ptr(self.packed),
                               self.c['n'], self.c['epochs'], ptr(self.out3), ptr(self.counts), ptr(dbg_t), stream_ptr())
        torch.cuda.synchronize()
        return self.state(), (dbg_t.cpu().numpy() if dbg else None)

    def state(self):
        pa, ma, va = self.actor.read()
        pc, mc, vc = self.critic.read()
        return dict(actor=pa, critic=pc, m=dict(actor=ma, critic=mc), v=dict(actor=va, critic=vc),
                    steps=tuple(int(x) for x in self.steps.cpu()), counts=tuple(int(x) for x in self.counts.cpu()),
                    out3=tuple(float(x) for x in self.out3.cpu()))


def _judge_state(c, tag, got, want):
    """Records and asserts a launch's state: step counts and minibatch counts exact, everything else at the bars."""
    assert got['steps'] == want['steps'] and got['counts'] == want['counts'], (tag, got['steps'], want['steps'], got['counts'], want['counts'])
    worst = E.compare_state(got, want)
    record_parity("ppo_mlp edges update [%s] %s" % (c['name'], tag), **{g: r for g, (r, _) in worst.items()})
    for group, (r, name) in worst.items():
        assert r <= E.bar(c['name'], group), (c['name'], tag, group, name, "error / bar = %.3g" % r)
    return worst


def _judge_first(c, dump, want_first, keys=None):
    rows0 = min(c['MB'], c['n'])
    first = E.decode_dump(dump, c, rows0)
    ratios = E.compare_first(first, want_first, keys)
    record_parity("ppo_mlp edges update [%s] first minibatch (debug instantiation)" % c['name'], padding=first['padding'], **ratios)
    assert first['padding'] == 0.0, "a padded position of a dumped gradient is not zero"
    for key, r in ratios.items():
        assert r <= E.bar(c['name'], "inter"), (c['name'], key, "error / bar = %.3g" % r)


# ------------------------------------------------------------------------------------------------ the update kernel
@pytest.mark.parametrize("c", E.UPDATE_CASES, ids=_ids(E.UPDATE_CASES))
def test_update_edge_case_debug_and_product_instantiations(dra, c):
    """Each case twice from the same inputs.  Through the debug instantiation <H,1,0>: every dumped intermediate and every
    parameter gradient of both networks of minibatch 0 at 1e-5 of the tensor's largest magnitude, padded positions of the dumped
    gradients exactly zero.  Through the product instantiation the launcher picks (<H,0,0>, <64,0,17>, <64,0,11>): parameters,
    both Adam moments, step counts, out_counts and out3 after all minibatches."""
    ref = E.reference(c)
    got, dump = _Update(dra, c).launch(0, dbg=True)
    _judge_first(c, dump, ref['first'])
    _judge_state(c, "debug instantiation", got, ref['launches'][0])
    got, _ = _Update(dra, c).launch(0)
    _judge_state(c, "product instantiation", got, ref['launches'][0])


def test_update_continues_on_the_same_device_buffers(dra):
    """Two launches on the same buffers, the second with fresh entries: the moments and step counts the first launch left on the
    device are what the second starts from (the reference carries opt_state)."""
    c = E.CONTINUATION_CASE
    ref, run = E.reference(c), _Update(dra, c)
    for li in range(2):
        got, _ = run.launch(li)
        _judge_state(c, "launch %d" % li, got, ref['launches'][li])
    assert got['steps'] == (6, 6)


def test_update_warm_start_from_preloaded_moments_and_step_counts(dra):
    c = E.WARM_CASE
    got, _ = _Update(dra, c).launch(0)
    _judge_state(c, "steps0 (5000, 4990)", got, E.reference(c)['launches'][0])
    assert got['steps'] == (5003, 4993)


def test_update_gate_closed_from_the_start_leaves_the_actor_bit_identical(dra):
    """approx_kl of every minibatch above the limit: actor parameters, both actor moments and the actor's step count come back to
    the bit, out_counts[0] is 0, the critic still steps and matches the reference."""
    c = E.GATE_CLOSED_CASE
    ref, run = E.reference(c), _Update(dra, c)
    before = run.actor.snapshot()
    got, _ = run.launch(0)
    assert got['counts'] == (0, 3) and got['steps'] == (0, 3)
    for b, a, what in zip(before, run.actor.snapshot(), ("param", "exp_avg", "exp_avg_sq")):
        assert np.array_equal(a, b), what
    _judge_state(c, "gate closed", got, ref['launches'][0])


def test_update_gate_closing_midway_at_hidden_16(dra):
    c = E.GATE_MIDWAY_CASE
    ref = E.reference(c)
    got, _ = _Update(dra, c).launch(0)
    assert 0 < got['counts'][0] < got['counts'][1] == 12
    _judge_state(c, "gate closes midway", got, ref['launches'][0])


@pytest.mark.parametrize("c", E.STD_CASES, ids=_ids(E.STD_CASES))
def test_update_std_sweep(dra, c):
    """std from -3 to either side of softplus' threshold at 20: log_pi_a, g_log_pi_a, dstd, dW3 and the policy loss from the dump of
    the one minibatch; the stepped std, w3 and their moments (with everything else) from the product run."""
    ref = E.reference(c)
    _, dump = _Update(dra, c).launch(0, dbg=True)
    _judge_first(c, dump, ref['first'], keys=("log_pi_a", "g_log_pi_a", "actor.dstd", "actor.dW3", "policy_loss"))
    got, _ = _Update(dra, c).launch(0)
    worst = _judge_state(c, "product instantiation", got, ref['launches'][0])
    assert set(worst) == {"param", "exp_avg", "exp_avg_sq", "scalar"}
    for k in ("std", "w3"):
        assert E.ratio("param", got['actor'][k], ref['launches'][0]['actor'][k]) <= 1.0, k
        assert not np.array_equal(got['actor'][k], E.update_inputs(c)['actor'][k].numpy()), k      # it stepped


def test_update_refusals_launch_nothing(dra):
    """dra_ppo_mlp_supported and both launchers answer DRA_EINVAL for every unsupported size or optimizer setting; no buffer
    changes."""
    from deeprl_amd import ppo_mlp
    from deeprl_amd._lib import lib, ptr, stream_ptr
    c = E.CASES_BY_NAME["h64-s11-a3-mb15-compiled-11"]
    run = _Update(dra, c)
    run.pack(0)
    roll = _Rollout(dra, E.ROLLOUTS_BY_NAME["h64-n9-s11-second-fold-chunk"])
    torch.cuda.synchronize()
    watched = [run.actor.param, run.actor.m, run.actor.v, run.critic.param, run.critic.m, run.critic.v, run.steps, run.out3, run.counts,
               run.packed] + roll.buffers()
    before = [_bits(t) for t in watched]
    assert lib.dra_ppo_mlp_supported.raw(c['S'], c['A'], c['H'], c['H'], c['MB']) == 0
    for over, what in E.UPDATE_REFUSALS:
        S, A, H, MB = (over.get(k, c[k]) for k in ("S", "A", "H", "MB"))
        if set(over) & {"S", "A", "H", "MB"}:
            assert lib.dra_ppo_mlp_supported.raw(S, A, H, H, MB) == EINVAL, what
        cfg = ppo_mlp.Cfg()
        cfg.state_dim, cfg.action_dim, cfg.hidden, cfg.mini_batch = S, A, H, MB
        cfg.ratio_clip, cfg.entropy_weight, cfg.kl_limit = run.cfg.ratio_clip, run.cfg.entropy_weight, run.cfg.kl_limit
        actor = ppo_mlp.Net.from_buffer_copy(run.actor.net)
        for field in ("off_std", "eps", "beta1"):
            if field in over:
                setattr(actor, field, over[field])
        rc = lib.dra_ppo_mlp_update.raw(ctypes.byref(cfg), ctypes.byref(actor), ctypes.byref(run.critic.net), ptr(run.packed), c['n'],
                                        c['epochs'], ptr(run.out3), ptr(run.counts), None, stream_ptr())
        assert rc == EINVAL, (what, rc)
        if "MB" not in over:          # (the rollout takes no minibatch)
            ractor = ppo_mlp.Net.from_buffer_copy(roll.actor.net)
            for field in ("off_std", "eps", "beta1"):
                if field in over:
                    setattr(ractor, field, over[field])
            rc = lib.dra_ppo_mlp_rollout.raw(ctypes.byref(cfg), ctypes.byref(ractor), ctypes.byref(roll.critic.net), ctypes.byref(roll.io),
                                             stream_ptr())
            assert rc == EINVAL, (what, "rollout", rc)
    for over, what in E.ROLLOUT_REFUSALS:
        io = ppo_mlp.RolloutIO.from_buffer_copy(roll.io)
        for field, value in over.items():
            setattr(io, field, value)
        rc = lib.dra_ppo_mlp_rollout.raw(ctypes.byref(roll.cfg), ctypes.byref(roll.actor.net), ctypes.byref(roll.critic.net), ctypes.byref(io),
                                         stream_ptr())
        assert rc == EINVAL, (what, rc)
    torch.cuda.synchronize()
    for t, b in zip(watched, before):
        assert np.array_equal(_bits(t), b)


# ------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("c", E.PACK_CASES, ids=_ids(E.PACK_CASES))
def test_pack_equals_restatement_bit_for_bit(dra, c):
    """dra_ppo_mlp_pack into a NaN-filled buffer against the numpy restatement of the image layout: every element written, every
    bit equal.  The last case is larger than one pass of the capped grid (8192 blocks x 256 threads)."""
    from deeprl_amd._lib import lib, ptr, stream_ptr
    dev = dra.Config.DEVICE
    inp, sh = E.pack_inputs(c), E.pack_shape(c)
    floats = ctypes.c_int64()
    lib.dra_ppo_mlp_packed_floats(c['n'], c['epochs'], c['MB'], c['S'], ctypes.byref(floats))
    assert floats.value == sh['floats']
    out = torch.full((floats.value,), float("nan"), dtype=torch.float32, device=dev)
    d = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    lib.dra_ppo_mlp_pack(ptr(d['state']), ptr(d['action']), ptr(d['log_pi_a']), ptr(d['advantage']), ptr(d['ret']), ptr(d['perm']), c['n'],
                         c['epochs'], c['MB'], c['S'], c['A'], ptr(out), stream_ptr())
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), E.pack_reference(inp, c['MB'])
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ rollout + value kernel
class _Rollout:
    """The device side of one rollout case: networks, environment state, statistics, NaN-filled outputs, dra_ppo_mlp_rollout_io."""

    def __init__(self, dra, c):
        from deeprl_amd import ppo_mlp
        self.c, self.ref, dev = c, E.rollout_reference(c), dra.Config.DEVICE
        ref, h = self.ref, E.hyper()
        N, S, A, T = c['N'], c['S'], c['A'], c['T']
        self.steps = torch.zeros(2, dtype=torch.int64, device=dev)
        self.actor = _DevNet(dev, ref['actor'], h['lr_actor'], self.steps[0:1])
        self.critic = _DevNet(dev, ref['critic'], h['lr_critic'], self.steps[1:2])
        cfg = ppo_mlp.Cfg()
        cfg.state_dim, cfg.action_dim, cfg.hidden, cfg.mini_batch = S, A, c['H'], 64
        self.cfg = cfg
        t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
        self.env_state, self.env_counter = t(ref['raw0'], torch.float64), torch.zeros(N, dtype=torch.int64, device=dev)
        self.env_seed, self.rms = t(ref['seeds'], torch.int64), t(ref['rms0'], torch.float64)
        self.cur_state = t(ref['cur0'], torch.float32)
        self.sampler = torch.full((1,), c['sampler_step0'], dtype=torch.int64, device=dev)
        f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
        self.o = dict(state=f(T, N, S), action=f(T, N, A), log_pi_a=f(T, N), v=f(T + 1, N), reward=f(T, N), mask=f(T, N))
        io, o = ppo_mlp.RolloutIO(), self.o
        io.env_state, io.env_counter, io.env_seed, io.rms = (x.data_ptr() for x in (self.env_state, self.env_counter, self.env_seed, self.rms))
        io.cur_state, io.sampler_step = self.cur_state.data_ptr(), self.sampler.data_ptr()
        io.out_state, io.out_action, io.out_log_pi_a = o['state'].data_ptr(), o['action'].data_ptr(), o['log_pi_a'].data_ptr()
        io.out_v, io.out_reward, io.out_mask = o['v'].data_ptr(), o['reward'].data_ptr(), o['mask'].data_ptr()
        io.env0, io.n_global, io.noise_seed, io.horizon = c['env0'], c['n_global'], c['noise_seed'], c['horizon']
        io.reward_coef, io.rms_epsilon, io.rms_clip, io.rms_update, io.t_len, io.n_env = 1.0, 1e-8, 10.0, c['rms_update'], T, N
        self.io = io

    def buffers(self):
        return [self.env_state, self.env_counter, self.env_seed, self.rms, self.cur_state, self.sampler, self.actor.param, self.critic.param] + \
            list(self.o.values())


@pytest.mark.parametrize("c", E.ROLLOUT_CASES, ids=_ids(E.ROLLOUT_CASES))
def test_rollout_edge_case(dra, c):
    """dra_ppo_mlp_rollout (rollout kernel + value kernel) against oracle.rollout with float64 forwards: stored observations, actions,
    log-probabilities, values at 1e-5 x max(largest magnitude, 1); rewards, masks, counters and the sampler step exact; observation
    statistics at rtol 1e-7 (bit-identical when rms_update is 0); no output element left unwritten."""
    from deeprl_amd._lib import lib, stream_ptr
    r = _Rollout(dra, c)
    ref, want, S = r.ref, r.ref['want'], c['S']
    lib.dra_ppo_mlp_rollout(ctypes.byref(r.cfg), ctypes.byref(r.actor.net), ctypes.byref(r.critic.net), ctypes.byref(r.io), stream_ptr())
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in r.o.items()}
    for k, v in got.items():
        assert not np.isnan(v).any(), "%s: %d elements never written" % (k, int(np.isnan(v).sum()))
    ratios = E.compare_rollout(got, want)
    cur, env_state, h = r.cur_state.cpu().numpy(), r.env_state.cpu().numpy(), r.rms.cpu().numpy()
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    record_parity("ppo_mlp edges rollout [%s]" % c['name'], cur_state_abs=float(np.abs(cur - want['cur_state']).max()),
                  env_state_abs=float(np.abs(env_state - want['raw_states']).max()), rms_mean_rel=rel(h[:S], ref['rms1'][:S]),
                  rms_var_rel=rel(h[S:2 * S], ref['rms1'][S:2 * S]), **ratios)
    assert int(r.sampler.cpu()[0]) == ref['sampler_step'] == c['sampler_step0'] + c['T'] + 1
    assert np.array_equal(r.env_counter.cpu().numpy(), ref['counters'])
    assert np.array_equal(got['mask'], want['mask']) and np.array_equal(got['reward'], want['reward'])
    for key, ratio in ratios.items():
        assert ratio <= E.bar(c['name'], "rollout"), (c['name'], key, "error / bar = %.3g" % ratio)
    np.testing.assert_allclose(cur, want['cur_state'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(env_state, want['raw_states'], rtol=1e-6, atol=1e-8)
    if c['rms_update']:
        np.testing.assert_allclose(h[:S], ref['rms1'][:S], rtol=1e-7, atol=0)
        np.testing.assert_allclose(h[S:2 * S], ref['rms1'][S:2 * S], rtol=1e-7, atol=0)
        assert h[2 * S] == ref['rms1'][2 * S]
    else:
        assert np.array_equal(h, ref['rms0'])
    # the rollout reads the networks and never steps them
    assert np.array_equal(r.steps.cpu().numpy(), [0, 0])
    for net, params in ((r.actor, ref['actor']), (r.critic, ref['critic'])):
        p, m, v = net.read()
        assert all(np.array_equal(p[k], params[k].numpy()) for k in params) and not any(x.any() for x in list(m.values()) + list(v.values()))


# ------------------------------------------------------------------------------------------------ stand-alone kernels
@pytest.mark.parametrize("n,d", E.RMS_CASES)
def test_rms_normalize_edges_equal_host_class_bit_for_bit(dra, n, d):
    """dra_rms_normalize at one feature, above one pass of its 256 threads and at its documented limit of 4096 features (64 KB of
    dynamic LDS): five updates then a read-only call, statistics and outputs identical to normalizers.MeanStdNormalizer."""
    from deeprl_amd import ppo_mlp
    from deeprl_amd.normalizers import MeanStdNormalizer
    dev = dra.Config.DEVICE
    rs = np.random.RandomState(n * 10007 + d)
    host = MeanStdNormalizer()
    mean = torch.zeros(d, dtype=torch.float64, device=dev)
    var = torch.ones(d, dtype=torch.float64, device=dev)
    count = torch.full((1,), 1e-4, dtype=torch.float64, device=dev)
    for it in range(6):
        x = rs.randn(n, d) * rs.uniform(0.01, 30.0, size=d) + rs.uniform(-5, 5, size=d)
        if it == 5:
            host.set_read_only()
        want = host(x)
        o32, o64 = ppo_mlp.rms_normalize(torch.from_numpy(x).to(dev), mean, var, count, update=it < 5, out_f64=True)
        assert np.array_equal(o64.cpu().numpy(), want), it
        assert np.array_equal(o32.cpu().numpy(), want.astype(np.float32)), it
        assert np.array_equal(mean.cpu().numpy(), host.rms.mean.reshape(-1)), it
        assert np.array_equal(var.cpu().numpy(), host.rms.var.reshape(-1)), it
        assert float(count.cpu()[0]) == host.rms.count and host.rms.count > n * min(it + 1, 5), it


def test_stand_alone_kernels_refuse_sizes_past_their_limits(dra):
    from deeprl_amd._lib import lib, ptr, stream_ptr
    dev = dra.Config.DEVICE
    d = E.RMS_REFUSED_D
    x = torch.zeros(1, d, dtype=torch.float64, device=dev)
    mean, var, count = torch.zeros(d, dtype=torch.float64, device=dev), torch.ones(d, dtype=torch.float64, device=dev), torch.ones(1, dtype=torch.float64, device=dev)
    out = torch.full((1, d), float("nan"), dtype=torch.float32, device=dev)
    assert lib.dra_rms_normalize.raw(ptr(x), 1, d, ptr(mean), ptr(var), ptr(count), 1, 1e-8, 10.0, ptr(out), None, stream_ptr()) == EINVAL
    a = E.GAUSS_REFUSED_A
    m, sc, step = torch.zeros(2, a, device=dev), torch.ones(a, device=dev), torch.full((1,), 4, dtype=torch.int64, device=dev)
    act = torch.full((2, a), float("nan"), device=dev)
    assert lib.dra_gauss_sample.raw(ptr(m), ptr(sc), 2, a, 5, ptr(step), 2, 0, ptr(act), stream_ptr()) == EINVAL
    s = E.ENV_REFUSED_S
    state, counter, seed = torch.zeros(2, s, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev), torch.ones(2, dtype=torch.int64, device=dev)
    action, rew, done = torch.zeros(2, 2, device=dev), torch.full((2,), float("nan"), dtype=torch.float64, device=dev), torch.full((2,), -3, dtype=torch.int32, device=dev)
    assert lib.dra_cont_env_step.raw(ptr(state), ptr(counter), ptr(seed), ptr(action), 2, s, 2, 5, ptr(rew), ptr(done), stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all() and float(count.cpu()[0]) == 1.0 and not mean.cpu().numpy().any()
    assert np.isnan(act.cpu().numpy()).all() and int(step.cpu()[0]) == 4
    assert np.isnan(rew.cpu().numpy()).all() and (done.cpu().numpy() == -3).all() and not counter.cpu().numpy().any() and not state.cpu().numpy().any()


@pytest.mark.parametrize("n,a_dim", E.GAUSS_CASES)
def test_gauss_sample_edges_match_oracle_stream(dra, n, a_dim):
    """dra_gauss_sample at one element, above one pass of its 256 threads and at a_dim 32: 1e-5 absolute against the oracle's numpy
    Box-Muller, the step counter advancing by one; at 64 x 16 a shard also draws its rows of the global matrix to the bit."""
    from deeprl_amd import ppo_mlp
    from oracle.ppo_mlp_oracle import gauss_noise
    dev = dra.Config.DEVICE
    rs = np.random.RandomState(n + a_dim)
    seed, t0 = 77 + n, 11
    step = torch.full((1,), t0, dtype=torch.int64, device=dev)
    scale = rs.uniform(0.3, 1.5, size=a_dim).astype(np.float32)
    worst = 0.0
    for t in range(t0, t0 + 2):
        mean = rs.randn(n, a_dim).astype(np.float32)
        got = ppo_mlp.gauss_sample(torch.from_numpy(mean).to(dev), torch.from_numpy(scale).to(dev), seed, step).cpu().numpy()
        want = gauss_noise(seed, t, n, np.arange(n), a_dim) * scale + mean
        worst = max(worst, E.ratio("sample", got, want))
        assert int(step.cpu()[0]) == t + 1
    record_parity("ppo_mlp edges gauss_sample [%d,%d]" % (n, a_dim), sample=worst)
    assert worst <= 1.0, worst
    if (n, a_dim) == E.GAUSS_CASES[-1]:
        step2 = torch.full((1,), t0 + 1, dtype=torch.int64, device=dev)
        shard = ppo_mlp.gauss_sample(torch.from_numpy(mean[8:24]).to(dev), torch.from_numpy(scale).to(dev), seed, step2, n_global=n, env0=8)
        assert np.array_equal(shard.cpu().numpy(), got[8:24]) and int(step2.cpu()[0]) == t0 + 2


@pytest.mark.parametrize("n,s_dim,a_dim,horizon", E.ENV_CASES)
def test_cont_env_step_edges_equal_host_class_bit_for_bit(dra, n, s_dim, a_dim, horizon):
    """dra_cont_env_step above its 1024-block grid (the grid-stride), at s_dim 64 (one pass of its 64 threads) and 63, at horizon 1
    (every step terminal): five steps identical to envs.SyntheticContinuous behind DummyVecEnv."""
    from deeprl_amd import ppo_mlp
    from deeprl_amd.envs import DummyVecEnv, SyntheticContinuous
    dev = dra.Config.DEVICE
    envs = [SyntheticContinuous(40 + i, s_dim, a_dim, horizon=horizon) for i in range(n)]
    vec = DummyVecEnv(envs)
    state = torch.from_numpy(np.stack(vec.reset())).to(dev)
    counter = torch.zeros(n, dtype=torch.int64, device=dev)
    seed = torch.tensor([e.seed for e in envs], dtype=torch.int64, device=dev)
    rs = np.random.RandomState(n + s_dim)
    n_done = 0
    for t in range(5):
        act = (rs.randn(n, a_dim) * 1.2).astype(np.float32)
        obs, rew, done, _ = vec.step(np.clip(act, -1.0, 1.0))
        r, dn = ppo_mlp.cont_env_step(state, counter, seed, torch.from_numpy(act).to(dev), horizon)
        assert np.array_equal(state.cpu().numpy(), np.stack(obs)), t
        assert np.array_equal(r.cpu().numpy(), rew) and np.array_equal(dn.cpu().numpy().astype(bool), done), t
        n_done += int(done.sum())
    assert np.array_equal(counter.cpu().numpy(), [e.c for e in envs])
    assert n_done == 5 * n if horizon == 1 else 0 < n_done < 5 * n
