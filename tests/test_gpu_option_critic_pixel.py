"""Option-critic on pixels over device-resident rollouts (agents._OCRollout; csrc/option_critic.hip, conv_v2.hip
dra_rollout_conv1_ocheads): the head role in conv1's launch against the stand-alone head and fp64 numpy, its decisions against a
numpy inverse CDF, the bootstrap mode, the loss + heads' backward against fp64 numpy, the agent against the reference's own
OptionCriticAgent.step (tests/golden/option_critic/option_critic_pixel.npz, written by tests/golden/make_golden_option_critic.py)
with the recorded decisions replayed through midpoint uniforms, the device path against the host path, graph replay against eager
runs, and the zoo entry through run_steps."""
import os

import numpy as np
import pytest
import torch

import fake_envs
from parity_log import record_parity

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "option_critic", "option_critic_pixel.npz")
# the fixture's setup (tests/golden/make_golden_option_critic.py)
N_ENVS, N_ACTIONS, N_OPTIONS, ENV_SEED, DONE_PERIOD = 4, 4, 4, 7, 6
PARAM_SEED, STEPS, ROLLOUT = 31, 4, 5
EPS, TARGET_FREQ, TERM_REG, ENT_W = (0.6, 0.1, 200), 3, 0.01, 0.01


class _Quiet:
    def info(self, *a, **k):
        pass

    def add_scalar(self, *a, **k):
        pass

    def add_histogram(self, *a, **k):
        pass


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


def _scale(*arrays):
    return max(1.0, max(float(np.abs(np.asarray(a, dtype=np.float64)).max()) for a in arrays))


def _fold_np(slabs, bias):
    """fc4's finish in float32, slab 0 first, then + bias, ReLU: the kernels' order."""
    v = slabs[0].copy()
    for s in range(1, slabs.shape[0]):
        v = (v + slabs[s]).astype(np.float32)
    v = (v + bias[None, :]).astype(np.float32)
    return np.maximum(v, np.float32(0))


def _inv_cdf(p, u):
    """The first k whose fp32 running sum exceeds u, the last index if none does."""
    cdf = np.cumsum(p.astype(np.float32), axis=-1, dtype=np.float32)
    hit = cdf > u[..., None]
    return np.where(hit.any(-1), hit.argmax(-1), p.shape[-1] - 1)


def _normalise32(p):
    """p / (its fp32 sum in index order), as the device heads normalise a row before the inverse CDF."""
    s = np.zeros(p.shape[:-1], dtype=np.float32)
    for k in range(p.shape[-1]):
        s = (s + p[..., k]).astype(np.float32)
    return (p / s[..., None]).astype(np.float32)


def _midpoint_uniforms(p, k):
    cdf = np.cumsum(p.astype(np.float32), axis=-1, dtype=np.float32)
    hi = np.take_along_axis(cdf, k[..., None], axis=-1)[..., 0]
    lo = np.where(k > 0, np.take_along_axis(cdf, np.maximum(k - 1, 0)[..., None], axis=-1)[..., 0], np.float32(0))
    return ((lo.astype(np.float64) + hi) / 2).astype(np.float32)


def _softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _head_inputs(batch, n_opt, n_act, seed):
    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda:0")
    r = lambda *s, sc=0.05: (torch.randn(*s, generator=g) * sc).to(dev)
    slabs, fold_bias = r(28, batch, 512), r(512)
    heads = (r(n_opt, 512), r(n_opt), r(n_opt, 512, sc=0.1), r(n_opt), r(n_opt * n_act, 512, sc=0.2), r(n_opt * n_act))
    return g, slabs, fold_bias, heads


# ---------------------------------------------------------------------------------------------------- 1. the head role
@pytest.mark.parametrize("n_opt,n_act", [(4, 4), (4, 18)])
@pytest.mark.parametrize("batch", [1, 4, 16, 32])
def test_conv1_ocheads_equal_stand_alone_head_and_numpy(dra, batch, n_opt, n_act):
    d = dra
    dev = torch.device("cuda:0")
    g, slabs, fold_bias, heads = _head_inputs(batch, n_opt, n_act, 200 + batch + n_act)
    frames = torch.randint(0, 256, (batch, 4, 84, 84), dtype=torch.uint8, generator=g).to(dev)
    wt1 = (torch.randn(32, 4, 8, 8, generator=g) * 0.05).permute(1, 2, 3, 0).contiguous().to(dev)
    b1 = (torch.randn(32, generator=g) * 0.05).to(dev)
    coef = 1.0 / 255.0
    eps = torch.tensor([0.3], device=dev)
    mask = (torch.rand(batch, generator=g) > 0.3).float().to(dev)
    prev0 = torch.randint(0, n_opt, (batch,), generator=g).to(dev)
    init0 = (torch.rand(batch, generator=g) < 0.5).to(dev)
    if batch > 1:
        init0[0], init0[1] = True, False               # both branches in every batch of two or more
    uni = torch.rand(batch, 3, generator=g)
    # the action uniforms: the middle of a random category's interval (fp64 softmax of the logits, set below)
    res = []
    for fused in (True, False):
        prev, init = prev0.clone(), init0.clone()
        out = dict(q=torch.empty(batch, n_opt, device=dev), beta=torch.empty(batch, n_opt, device=dev),
                   logits=torch.empty(batch, n_act, device=dev), option=torch.empty(batch, dtype=torch.int64, device=dev),
                   action=torch.empty(batch, dtype=torch.int64, device=dev), log_pi_a=torch.empty(batch, device=dev),
                   entropy=torch.empty(batch, device=dev), prev_option=torch.empty(batch, dtype=torch.int64, device=dev),
                   init=torch.empty(batch, device=dev), phi=torch.empty(batch, 512, device=dev))
        y1 = torch.empty(batch, 32, 20, 20, device=dev)
        if fused:
            d.ops.rollout_conv1_ocheads(frames, wt1, b1, y1, coef, slabs, fold_bias, heads, uni.to(dev), eps, mask, prev, init, out=out)
        else:
            d.ops.oc_heads_fold28(slabs, fold_bias, *heads, uniform=uni.to(dev), eps=eps, mask=mask, prev_option=prev,
                                  is_initial=init, out=out)
        torch.cuda.synchronize()
        res.append((y1, out, prev, init))
    (y1, o, prev, init), (_, o2, prev2, init2) = res
    y1_ref = d.ops.conv_fwd_koc(1, [frames], [wt1], [b1], act="relu", u8_coef=coef)[0]
    assert torch.equal(y1, y1_ref)
    for k in o:
        assert torch.equal(o[k], o2[k]), k
    assert torch.equal(prev, prev2) and torch.equal(init, init2)
    h = {k: v.cpu().numpy() for k, v in o.items()}
    phi_np = _fold_np(slabs.cpu().numpy(), fold_bias.cpu().numpy())
    assert np.array_equal(h['phi'], phi_np)
    wq, bq, wb, bb, wp, bp = [x.cpu().numpy().astype(np.float64) for x in heads]
    p64 = phi_np.astype(np.float64)
    q64, zb64 = p64 @ wq.T + bq, p64 @ wb.T + bb
    logits64 = (p64 @ wp.T + bp).reshape(batch, n_opt, n_act)
    beta64 = 1 / (1 + np.exp(-zb64))
    assert np.abs(h['q'] - q64).max() <= 1e-5 * _scale(q64)
    assert np.abs(h['beta'] - beta64).max() <= 1e-5
    # the decisions: a numpy inverse CDF on the kernel's own probabilities (its q / beta outputs, fp32 as the kernel forms them)
    q, beta = h['q'], h['beta']
    e = np.float32(0.3)
    g_opt = np.argmax(q, axis=-1)
    pi_opt = np.full((batch, n_opt), e / np.float32(n_opt), dtype=np.float32)
    pi_opt[np.arange(batch), g_opt] = np.float32(1) - e + e / np.float32(n_opt)
    p0, i0 = prev0.cpu().numpy(), init0.cpu().numpy()
    keep = np.zeros((batch, n_opt), dtype=np.float32)
    keep[np.arange(batch), p0] = 1
    pi_hat = (np.float32(1) - beta) * keep + beta * pi_opt
    u = uni.numpy()
    if batch >= 4:      # beta is a vector over options: pi_hat does not sum to one and needs the normalisation
        assert np.abs(pi_hat.sum(-1) - 1).max() > 1e-3
    want_opt = np.where(i0, _inv_cdf(_normalise32(pi_opt), u[:, 0]), _inv_cdf(_normalise32(pi_hat), u[:, 1]))
    assert np.array_equal(h['option'], want_opt)
    rows = np.arange(batch)
    chosen64 = logits64[rows, want_opt]
    assert np.abs(h['logits'] - chosen64).max() <= 1e-5 * _scale(chosen64)
    p_act = _softmax64(h['logits'])
    cdf = np.cumsum(p_act, axis=-1)
    a_ref = np.argmax(cdf > u[:, 2:3], axis=-1)
    near = np.abs(cdf - u[:, 2:3]).min(-1) < 1e-5          # a uniform on a boundary (never with these seeds, but exactness needs room)
    assert np.array_equal(h['action'][~near], a_ref[~near])
    lp = np.log(p_act)
    assert np.abs(h['log_pi_a'] - lp[rows, h['action']]).max() <= 1e-5
    assert np.abs(h['entropy'] - (-(p_act * lp).sum(-1))).max() <= 1e-5
    # the carried state: what was read is recorded, then prev <- option, init <- terminal
    assert np.array_equal(h['prev_option'], p0) and np.array_equal(h['init'], i0.astype(np.float32))
    assert np.array_equal(prev.cpu().numpy(), h['option'])
    assert np.array_equal(init.cpu().numpy(), mask.cpu().numpy() == 0)
    if batch > 1:
        assert i0.any() and (~i0).any()


# ---------------------------------------------------------------------------------------------------- 2. bootstrap mode
@pytest.mark.parametrize("batch", [4, 16])
def test_oc_bootstrap_mode_equals_fp64_numpy(dra, batch):
    d = dra
    dev = torch.device("cuda:0")
    n_opt, n_act = 4, 6
    g, slabs, fold_bias, heads = _head_inputs(batch, n_opt, n_act, 300 + batch)
    prev = torch.randint(0, n_opt, (batch,), generator=g).to(dev)
    prev_before = prev.clone()
    boot = torch.empty(batch, device=dev)
    q, beta = torch.empty(batch, n_opt, device=dev), torch.empty(batch, n_opt, device=dev)
    d.ops.oc_heads_fold28(slabs, fold_bias, heads[0], heads[1], heads[2], heads[3], prev_option=prev, boot=boot,
                          out=dict(q=q, beta=beta))
    torch.cuda.synchronize()
    assert torch.equal(prev, prev_before)
    p64 = _fold_np(slabs.cpu().numpy(), fold_bias.cpu().numpy()).astype(np.float64)
    wq, bq, wb, bb = [x.cpu().numpy().astype(np.float64) for x in heads[:4]]
    q64 = p64 @ wq.T + bq
    b64 = 1 / (1 + np.exp(-(p64 @ wb.T + bb)))
    pv = prev.cpu().numpy()
    r = np.arange(batch)
    want = (1 - b64[r, pv]) * q64[r, pv] + b64[r, pv] * q64.max(-1)
    assert np.abs(boot.cpu().numpy() - want).max() <= 1e-5 * _scale(want)
    assert np.abs(q.cpu().numpy() - q64).max() <= 1e-5 * _scale(q64)


# ---------------------------------------------------------------------------------------------------- 3. loss + backward
@pytest.mark.parametrize("t_len,n,n_opt,n_act", [(5, 7, 4, 5), (5, 16, 4, 18), (3, 32, 8, 4)])
def test_oc_loss_bwd_equals_fp64_numpy(dra, t_len, n, n_opt, n_act):
    d = dra
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(t_len * 100 + n + n_act)
    rows = t_len * n
    gamma, term, ent_w = 0.99, 0.01, 0.01
    q = rs.standard_normal((t_len, n, n_opt)).astype(np.float32)
    beta = rs.uniform(0.05, 0.95, (t_len, n, n_opt)).astype(np.float32)
    logits = rs.standard_normal((t_len, n, n_act)).astype(np.float32)
    option = rs.randint(0, n_opt, (t_len, n)).astype(np.int64)
    prev = rs.randint(0, n_opt, (t_len, n)).astype(np.int64)
    action = rs.randint(0, n_act, (t_len, n)).astype(np.int64)
    init = (rs.rand(t_len, n) < 0.3).astype(np.float32)
    lse = np.log(np.exp(logits.astype(np.float64)).sum(-1))
    lp_row = logits - lse[..., None]
    log_pi_a = np.take_along_axis(lp_row, action[..., None], -1)[..., 0].astype(np.float32)
    entropy = (-(np.exp(lp_row) * lp_row).sum(-1)).astype(np.float32)
    reward = np.sign(rs.standard_normal((t_len, n))).astype(np.float32)
    mask = (rs.rand(t_len, n) > 0.25).astype(np.float32)
    boot = rs.standard_normal(n).astype(np.float32)
    eps = np.linspace(0.5, 0.4, t_len).astype(np.float32)
    phi = np.maximum(rs.standard_normal((rows, 512)), 0).astype(np.float32)
    wq, wb = [(rs.standard_normal((n_opt, 512)) * 0.05).astype(np.float32) for _ in range(2)]
    wp = (rs.standard_normal((n_opt * n_act, 512)) * 0.05).astype(np.float32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    roll = dict(q=T(q), beta=T(beta), logits=T(logits), option=T(option), action=T(action), prev_option=T(prev), init=T(init),
                log_pi_a=T(log_pi_a), entropy=T(entropy))
    outs = [d.ops.oc_loss_bwd(roll, T(reward), T(mask), T(boot), T(eps), gamma, term, ent_w, T(phi), T(wq), T(wp), T(wb))
            for _ in range(2)]
    torch.cuda.synchronize()
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    out = {k: v.cpu().numpy().astype(np.float64) for k, v in outs[0].items()}
    # fp64 restatement of OptionCritic_agent.py:95-117
    f = lambda a: a.astype(np.float64)
    ret = np.zeros((t_len, n))
    r_ = f(boot)
    for t in reversed(range(t_len)):
        r_ = f(reward[t]) + gamma * f(mask[t]) * r_
        ret[t] = r_
    q64 = f(q)
    qo = np.take_along_axis(q64, option[..., None], -1)[..., 0]
    adv = ret - qo
    v = q64.max(-1) * (1 - f(eps))[:, None] + q64.mean(-1) * f(eps)[:, None]
    badv = np.take_along_axis(q64, prev[..., None], -1)[..., 0] - v + term
    bprev = np.take_along_axis(f(beta), prev[..., None], -1)[..., 0]
    q_loss = np.mean(0.5 * (qo - ret) ** 2)
    pi_loss = np.mean(-f(log_pi_a) * adv - ent_w * f(entropy))
    beta_loss = np.mean(bprev * badv * (1 - f(init)))
    dq = np.zeros((rows, n_opt))
    dq[np.arange(rows), option.reshape(-1)] = ((qo - ret) / rows).reshape(-1)
    p = np.exp(lp_row).reshape(rows, n_act)
    onehot = np.zeros((rows, n_act))
    onehot[np.arange(rows), action.reshape(-1)] = 1
    gl = (-adv / rows).reshape(-1, 1)
    ge = -ent_w / rows
    dl = gl * (onehot - p) - ge * p * (lp_row.reshape(rows, n_act) + f(entropy).reshape(-1, 1))
    dpi = np.zeros((rows, n_opt * n_act))
    for r in range(rows):
        o = option.reshape(-1)[r]
        dpi[r, o * n_act:(o + 1) * n_act] = dl[r]
    dz = np.zeros((rows, n_opt))
    dz[np.arange(rows), prev.reshape(-1)] = (bprev * (1 - bprev) * badv * (1 - f(init)) / rows).reshape(-1)
    p64 = f(phi)
    want = dict(ret=ret, adv=adv, beta_adv=badv, loss=np.asarray([pi_loss + q_loss + beta_loss, q_loss, pi_loss, beta_loss]),
                dw_q=dq.T @ p64, db_q=dq.sum(0), dw_pi=dpi.T @ p64, db_pi=dpi.sum(0), dw_beta=dz.T @ p64, db_beta=dz.sum(0),
                dphi=(dq @ f(wq) + dpi @ f(wp) + dz @ f(wb)) * (phi > 0))
    for k, w in want.items():
        err = float(np.abs(out[k].reshape(w.shape) - w).max())
        assert err <= 1e-5 * _scale(w), (k, err)
    assert np.all(out['dphi'][phi == 0] == 0)


# ---------------------------------------------------------------------------------------------------- agents
def _config(d, device_env=True, graph_update=True, n_envs=N_ENVS, tag="oc"):
    from deeprl_amd.envs import SyntheticAtari
    cfg = d.Config()
    cfg.merge(dict(game="synthetic-atari", log_level=0, tag=tag, device_env=device_env, graph_update=graph_update))
    cfg.num_workers = n_envs

    def task_fn():
        task = d.Task(cfg.game, num_envs=n_envs, seed=1, synthetic_done_period=DONE_PERIOD)
        # the fixture's emulators (fake_envs.PixelVectorTask: seed + 1000 e)
        task.env.envs[:] = [SyntheticAtari(ENV_SEED + 1000 * e, history=4, n_actions=N_ACTIONS, done_period=DONE_PERIOD)
                            for e in range(n_envs)]
        return task
    cfg.task_fn = task_fn
    cfg.eval_env = d.Task(cfg.game, seed=12)
    cfg.network_fn = lambda: d.OptionCriticNet(d.NatureConvBody(), N_ACTIONS, num_options=N_OPTIONS)
    cfg.optimizer_fn = lambda p: torch.optim.RMSprop(p, lr=1e-4, alpha=0.99, eps=1e-5)
    cfg.random_option_prob = d.LinearSchedule(*EPS)
    cfg.state_normalizer, cfg.reward_normalizer = d.ImageNormalizer(), d.SignNormalizer()
    cfg.discount, cfg.target_network_update_freq, cfg.rollout_length, cfg.gradient_clip = 0.99, TARGET_FREQ, ROLLOUT, 5
    cfg.termination_regularizer, cfg.entropy_weight = TERM_REG, ENT_W
    return cfg


def _oc_shapes():
    return fake_envs.NATURE_SHAPES + [("fc_q.weight", (N_OPTIONS, 512)), ("fc_q.bias", (N_OPTIONS,)),
                                      ("fc_pi.weight", (N_OPTIONS * N_ACTIONS, 512)), ("fc_pi.bias", (N_OPTIONS * N_ACTIONS,)),
                                      ("fc_beta.weight", (N_OPTIONS, 512)), ("fc_beta.bias", (N_OPTIONS,))]


def _agent(d, monkeypatch, **kw):
    import deeprl_amd.agents as agents_mod
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Quiet())
    agent = d.OptionCriticAgent(_config(d, **kw))
    p_np = fake_envs.numpy_params(_oc_shapes(), PARAM_SEED)
    agent.network.load_state_dict({k: torch.from_numpy(v) for k, v in p_np.items()})
    agent._sync_target()
    torch.cuda.synchronize()
    return agent


def _params(agent):
    return {k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()}


def _fixture_uniforms(g):
    """[STEPS][T, N, 3] midpoint uniforms of the reference's recorded draws (fresh option, continued option, action)."""
    return [np.stack([_midpoint_uniforms(g["s%d_%s_p" % (s, name)], g["s%d_%s" % (s, name)])
                      for name in ("fresh", "continued", "action")], axis=-1) for s in range(STEPS)]


def _replay_uniforms(agent, uniforms):
    """Overrides _OCRollout.draw_uniforms: rollout s reads uniforms[s] (at the persistent buffer's address)."""
    oc = agent._oc_rollout
    oc.uniform = torch.empty((ROLLOUT, N_ENVS, 3), dtype=torch.float32, device=torch.device("cuda:0"))
    k = [0]

    def draw(t_len):
        oc.uniform.copy_(torch.from_numpy(np.ascontiguousarray(uniforms[k[0]])))
        k[0] += 1
    oc.draw_uniforms = draw


def test_device_agent_matches_reference_fixture(dra, monkeypatch):
    """Options and actions exact at every step (graph replays included); q, beta, log pi, entropy, returns, advantages and the
    losses within 1e-5 of scale at every step (measured: at most 1.9e-6), parameter digests within 1e-5 of scale after every
    update.  The measured maxima go to the parity log."""
    d = dra
    g = np.load(FIXTURE)
    agent = _agent(d, monkeypatch)
    assert getattr(agent.task, "on_device", False), "synthetic Atari + OptionCriticNet(NatureConvBody) take the device path"
    _replay_uniforms(agent, _fixture_uniforms(g))
    errs = []
    for s in range(STEPS):
        agent.step()
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in agent.last_rollout.items()}
        k = "s%d_" % s
        for name in ("option", "action", "prev_option"):
            assert np.array_equal(out[name], g[k + name]), (s, name)
        assert np.array_equal(out['init'], g[k + "init"]), s
        assert agent.total_steps == int(g[k + "total_steps"])
        log_pi = out['logits'].astype(np.float64)
        log_pi = log_pi - np.log(np.exp(log_pi - log_pi.max(-1, keepdims=True)).sum(-1, keepdims=True)) - log_pi.max(-1, keepdims=True)
        rel = lambda have, want: float(np.abs(np.asarray(have, np.float64) - want).max()) / _scale(want)
        e = dict(q=rel(out['q'], g[k + "q"]), beta=rel(out['beta'], g[k + "beta"]), log_pi=rel(log_pi, g[k + "log_pi"]),
                 entropy=rel(out['entropy'], g[k + "entropy"]), ret=rel(out['ret'], g[k + "ret"]),
                 advantage=rel(out['advantage'], g[k + "advantage"]), beta_advantage=rel(out['beta_advantage'], g[k + "beta_advantage"]),
                 loss=rel(out['losses'], g[k + "loss"]), params=0.0)
        for name, v in _params(agent).items():
            want = g[k + "param_" + name]
            have = v.reshape(-1)[::1009].astype(np.float64)
            e['params'] = max(e['params'], float(np.abs(have - want[2:]).max()) / _scale(want[2:]))
        errs.append(e)
        record_parity("option_critic_pixel_device_vs_reference_step%d" % s, **e)
    for s, e in enumerate(errs):
        assert all(v <= 1e-5 for v in e.values()), (s, errs)
    assert agent.prev_options.dtype == torch.int64 and agent.is_initial_states.dtype == torch.bool
    assert np.array_equal(agent.prev_options.cpu().numpy(), g["s%d_option" % (STEPS - 1)][-1])
    assert np.array_equal(agent.is_initial_states.cpu().numpy(), g["s%d_mask" % (STEPS - 1)][-1] == 0)
    assert agent._dev_graph.graph is not None and agent._dev_graph.calls == STEPS, "steps after the warm-up replay the graph"
    agent.close()


def _run_device(d, monkeypatch, steps, **kw):
    torch.manual_seed(5)
    agent = _agent(d, monkeypatch, **kw)
    assert getattr(agent.task, "on_device", False)
    opts, acts = [], []
    for _ in range(steps):
        agent.step()
        opts.append(agent.last_rollout['option'].cpu().numpy().copy())
        acts.append(agent.last_rollout['action'].cpu().numpy().copy())
    torch.cuda.synchronize()
    res = (_params(agent), np.stack(opts), np.stack(acts), agent.total_steps, agent)
    agent.close()
    return res


def test_device_path_equals_host_path(dra, monkeypatch):
    """The same setup with config.device_env = False (today's host path: module forwards, torch's Categorical draws, host
    emulators) made to take the device run's decisions -- Categorical.sample returns the chosen option for both option draws,
    then the action: parameters within 1e-5 of scale after six agent steps."""
    d = dra
    steps = 6
    dev = _run_device(d, monkeypatch, steps)
    queue = []
    for s in range(steps):
        for t in range(ROLLOUT):
            queue += [dev[1][s][t], dev[1][s][t], dev[2][s][t]]
    queue.reverse()

    def replay(self, sample_shape=torch.Size()):
        return torch.as_tensor(queue.pop(), device=self.probs.device)
    monkeypatch.setattr(torch.distributions.Categorical, "sample", replay)
    host = _agent(d, monkeypatch, device_env=False)
    assert not getattr(host.task, "on_device", False)
    for _ in range(steps):
        host.step()
    torch.cuda.synchronize()
    assert not queue and host.total_steps == dev[3]
    hp = _params(host)
    host.close()
    worst = 0.0
    for k in dev[0]:
        sc = _scale(hp[k])
        e = float(np.abs(dev[0][k] - hp[k]).max())
        assert e <= 1e-5 * sc, (k, e)
        worst = max(worst, e / sc)
    record_parity("option_critic_pixel_device_vs_host", params=worst)


def test_graph_replay_equals_eager_device_path(dra, monkeypatch):
    d = dra
    a = _run_device(d, monkeypatch, 5)
    b = _run_device(d, monkeypatch, 5, graph_update=False)
    assert a[4]._dev_graph.graph is not None and b[4]._dev_graph.graph is None
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k


def test_launcher_runs_option_critic_pixel_through_run_steps(dra):
    """examples.py::option_critic_pixel (examples.py:471-492: 16 workers, rollouts of 5, 4 options) through launch.run_entry +
    run_steps on device-resident synthetic Atari."""
    d = dra
    from deeprl_amd import launch
    import deeprl_amd.zoo as zoo
    mod = launch.load_examples(zoo.__file__, "zoo_examples_oc")
    d.random_seed(3)
    agent = launch.run_entry(mod, "option_critic_pixel", max_steps=1600, game="synthetic-atari", overrides=dict(save_interval=0))
    assert agent.total_steps == 1600
    assert getattr(agent.task, "on_device", False) and agent._dev_graph.graph is not None
    assert all(torch.isfinite(v).all() for v in agent.network.state_dict().values())
