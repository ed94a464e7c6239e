"""GPU tests of the fused DDPG / TD3 update (csrc/dpg_mlp.hip, deeprl_amd/dpg_mlp.py): the kernel calls against the fp64
restatement (tests/dpg_restatement.py, pinned to the reference's recorded updates by tests/test_dpg_update_host.py), the acting
forward, the recorded reference updates replayed, the counter-hash smoothing noise, and DDPGAgent / TD3Agent with
`config.fused_dpg_update` on.
Bars: exact for integer and cadence facts; 1e-5 of a tensor's largest magnitude (floor 1) for one kernel call against fp64;
rtol 2e-4 / atol 2e-5 on parameters against the reference's fp32 run (test_gpu_more_agents.py)."""
import ctypes
import random

import numpy as np
import pytest
import torch
from parity_log import record_parity

import dpg_cases as K
import dpg_restatement as R
import fake_envs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1, 16, 16),          # one row
          (17, 5, 2, 20, 12),         # a row tail of 1, every dimension off the tile grid
          (16, 4, 4, 16, 16),         # everything exactly on the grid
          (100, 17, 6, 400, 300),     # the example's shape
          (128, 64, 16, 512, 512)]    # the corner of the supported range
PAD = 3                               # NaN floats between tensors
LEAD = 7                              # unused floats in front of the first tensor
TAIL = 64                             # sentinel floats behind the workspace's stated size


class _Quiet:
    def __init__(self):
        self.warnings = []

    def info(self, *a, **k):
        pass
    add_scalar = add_histogram = info

    def warning(self, msg, *a, **k):
        self.warnings.append(str(msg))


@pytest.fixture()
def dra(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deeprl_amd as d
    import deeprl_amd.agents as agents_mod
    d.select_device(0)
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Quiet())
    return d


def _within(got, want, what):
    """1e-5 of the tensor's largest magnitude, floor 1.0 (test_gpu_a2c_continuous.py's bar for one kernel call against fp64)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    bar = 1e-5 * max(float(np.abs(want).max()) if want.size else 0.0, 1.0)
    print("%s: max abs error %.3e (bar %.3e)" % (what, err, bar))
    assert err <= bar, (what, err, bar)
    return err / bar


class _Packed:
    """Canonical parameter dicts laid out in ONE flat buffer per kind with a leading gap, the tensors in a scrambled order and
    NaN padding between them (offsets neither start at 0 nor are contiguous), uploaded to the device."""

    def __init__(self, dev, shp, order_seed, aligned=False, **kinds):
        """aligned: every tensor starts on a 16-byte boundary (what optim.FlatParams gives: the kernels' 16-byte requests)."""
        self.shp = shp
        keys = sorted(next(iter(kinds.values())))
        np.random.RandomState(order_seed).shuffle(keys)
        self.off, o = {}, LEAD
        for k in keys:
            o = (o + 3) // 4 * 4 if aligned else o
            self.off[k] = o
            o += next(iter(kinds.values()))[k].numel() + PAD
        self.n = o
        self.host, self.dev = {}, {}
        for name, params in kinds.items():
            flat = np.full(self.n, np.nan, dtype=np.float32)
            for k in keys:
                v = params[k].numpy().astype(np.float32).reshape(-1)
                flat[self.off[k]:self.off[k] + v.size] = v
            self.host[name] = flat
            self.dev[name] = torch.from_numpy(flat.copy()).to(dev)
        self.keys = keys
        self.shapes = {k: tuple(next(iter(kinds.values()))[k].shape) for k in keys}

    def net(self, name):
        from deeprl_amd import dpg_mlp
        n = dpg_mlp.Net()
        n.param = self.dev[name].data_ptr()
        for role in ["a"] + ["c%d" % c for c in range(self.shp[5])]:
            six = (ctypes.c_int32 * 6)(*[self.off["%s.%s" % (role, lay)] for lay in R.LAYERS])
            if role == "a":
                n.actor = six
            else:
                n.critic[int(role[1])] = six
        n.state_dim, n.action_dim, n.h1, n.h2, n.gate, n.n_critics = self.shp
        return n

    def read(self, name):
        flat = self.dev[name].cpu().numpy()
        return flat, {k: flat[self.off[k]:self.off[k] + int(np.prod(self.shapes[k]))].reshape(self.shapes[k]) for k in self.keys}

    def padding_unchanged(self, name, flat):
        mask = np.ones(self.n, dtype=bool)
        for k in self.keys:
            mask[self.off[k]:self.off[k] + int(np.prod(self.shapes[k]))] = False
        return np.array_equal(flat.view(np.uint32)[mask], self.host[name].view(np.uint32)[mask])


def _step_struct(packed, hp, t, counter=0, seed=0):
    from deeprl_amd import dpg_mlp
    from deeprl_amd._lib import lib
    two = (ctypes.c_float * 2)()
    lib.dra_adam_hyper(hp["lr"], hp["beta1"], hp["beta2"], int(t), two)
    s = dpg_mlp.Step()
    s.exp_avg, s.exp_avg_sq = packed.dev["m"].data_ptr(), packed.dev["v"].data_ptr()
    s.step_size, s.inv_sqrt_bc2, s.beta1, s.beta2, s.eps = two[0], two[1], hp["beta1"], hp["beta2"], hp["eps"]
    s.discount, s.td3_noise, s.td3_noise_clip = hp["discount"], hp["td3_noise"], hp["td3_noise_clip"]
    s.action_low, s.action_high = hp["action_low"], hp["action_high"]
    s.noise_seed, s.noise_counter = seed, counter
    return s


def _device_update(dev, packed, batch, hp, t_critic, t_actor, policy=True, noise=None, counter=0, seed=0):
    """dra_dpg_critic_update, then (policy) dra_dpg_actor_update and the soft update; returns (workspace numpy incl. the
    sentinel tail, its stated size)."""
    from deeprl_amd import dpg_mlp, ops
    from deeprl_amd._lib import lib, stream_ptr
    shp = packed.shp
    b = batch["state"].shape[0]
    n_ws = dpg_mlp.workspace_floats(b, shp)
    ws = torch.full((n_ws + TAIL,), -7.25, dtype=torch.float32, device=dev)
    up = lambda x, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)
    f64 = batch["state"].dtype == np.float64
    t = {k: up(batch[k], np.float64 if f64 else np.float32) for k in ("state", "action", "next_state")}
    rew, mask = up(batch["reward"]), up(batch["mask"])
    nz = None if noise is None else up(noise)
    bs = dpg_mlp.Update.batch_struct(t["state"], t["action"], rew, t["next_state"], mask, nz)
    on, tg = packed.net("online"), packed.net("target")
    ref = ctypes.byref
    st = _step_struct(packed, hp, t_critic, counter, seed)
    lib.dra_dpg_critic_update(ref(on), ref(tg), ref(bs), ref(st), ws.data_ptr(), stream_ptr())
    if policy:
        st = _step_struct(packed, hp, t_actor, counter, seed)
        lib.dra_dpg_actor_update(ref(on), ref(bs), ref(st), ws.data_ptr(), stream_ptr())
        ops.soft_update(packed.dev["target"], packed.dev["online"], hp["target_network_mix"])
    torch.cuda.synchronize()
    return ws.cpu().numpy(), n_ws


def _moments(online, seed):
    rs = np.random.RandomState(seed)
    f = lambda x: torch.as_tensor(x.astype(np.float32).astype(np.float64))
    m = {k: f(0.01 * rs.randn(*v.shape)) for k, v in online.items()}
    v = {k: f(rs.uniform(1e-4, 1e-3, size=tuple(v.shape))) for k, v in online.items()}
    return m, v


@pytest.mark.parametrize("gate", [K.GATE_RELU, K.GATE_TANH])
@pytest.mark.parametrize("n_critics", [1, 2])
@pytest.mark.parametrize("dims", SHAPES[1:], ids=lambda d: "x".join(map(str, d)))
def test_kernel_calls_match_restatement_on_16_byte_aligned_tensors(dra, dims, n_critics, gate):
    """The same comparison with every tensor on a 16-byte boundary, as optim.FlatParams lays the agents' parameters out: the
    layers whose rows are then 16-byte aligned take the kernels' 16-byte requests."""
    test_kernel_calls_match_restatement(dra, dims, n_critics, gate, aligned=True)


@pytest.mark.parametrize("gate", [K.GATE_RELU, K.GATE_TANH])
@pytest.mark.parametrize("n_critics", [1, 2])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_kernel_calls_match_restatement(dra, dims, n_critics, gate, aligned=False):
    """dra_dpg_critic_update then dra_dpg_actor_update (then the soft update) from a state with non-zero Adam moments and step
    counts (5, 3): y, q, the per-row loss, online parameters, both moments and target parameters within 1e-5 of each tensor's
    largest magnitude (floor 1) of the fp64 restatement; the NaN padding between the tensors and the floats behind the
    workspace's stated size are bit-unchanged; a second run from the same start gives the same bits."""
    dev = dra.Config.DEVICE
    b, s, a, h1, h2 = dims
    shp = (s, a, h1, h2, gate, n_critics)
    seed = 1000 * b + 10 * n_critics + gate
    online, target, batch, hp = K.random_case(dims, n_critics, seed, head_scale=3.0)
    m0, v0 = _moments(online, seed + 1)
    noise = np.random.RandomState(seed + 2).randn(b, a).astype(np.float32) * 1.5 if n_critics == 2 else None
    st = R.State(online, target, n_critics, gate, exp_avg=m0, exp_avg_sq=v0)
    st.t_critic, st.t_actor = 4, 2
    want = st.update(batch, hp, policy_step=True, noise=noise)

    runs = []
    for _ in range(2):
        packed = _Packed(dev, shp, seed, aligned=aligned, online=online, target=target, m=m0, v=v0)
        ws, n_ws = _device_update(dev, packed, batch, hp, 5, 3, noise=noise)
        runs.append((packed, ws, {k: packed.read(k) for k in ("online", "target", "m", "v")}))
    packed, ws, got = runs[0]
    errs = dict(y=_within(ws[:b], want["y"], "y"), q=_within(ws[b:b + n_critics * b].reshape(n_critics, b), want["q"], "q"),
                loss=_within(ws[3 * b:4 * b], want["loss"], "loss"))
    for name, ref_params in (("online", st.online), ("target", st.target), ("m", st.m), ("v", st.v)):
        errs[name] = max(_within(got[name][1][k], ref_params[k].numpy(), "%s %s" % (name, k)) for k in packed.keys)
    record_parity("dpg kernel calls vs fp64 restatement %s critics %d gate %d%s (fraction of the bar)"
                  % (dims, n_critics, gate, " aligned" if aligned else ""), **errs)
    for name in ("online", "m", "v"):
        assert packed.padding_unchanged(name, got[name][0]), name
    flat_t = got["target"][0]
    assert np.isnan(flat_t[:LEAD]).all() and np.isfinite(flat_t).sum() == sum(int(np.prod(v)) for v in packed.shapes.values())
    assert np.array_equal(ws[n_ws:].view(np.uint32), np.full(TAIL, -7.25, dtype=np.float32).view(np.uint32))
    for name in ("online", "target", "m", "v"):
        assert np.array_equal(runs[0][2][name][0].view(np.uint32), runs[1][2][name][0].view(np.uint32)), name
    assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))
    # the step did move every kind of tensor, and (TD3) the case reaches both clamps
    assert all(float((st.online[k] - online[k]).abs().max()) > 0.0 for k in online)
    if n_critics == 2 and b > 1:
        assert (np.abs(noise * hp["td3_noise"]) > hp["td3_noise_clip"]).any()


def test_critic_update_reads_fp64_strided_rows(dra):
    """The minibatch as the replay ring hands it back: fp64 state / next_state as two views of one [B, 2, S] block, fp64
    actions; the same y as from the fp32 copies (the kernel narrows on load, as the agents' cast does)."""
    from deeprl_amd import dpg_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    dims, nc, gate = (17, 5, 2, 20, 12), 2, K.GATE_RELU
    b, s, a, h1, h2 = dims
    shp = (s, a, h1, h2, gate, nc)
    online, target, batch, hp = K.random_case(dims, nc, 77)
    rs = np.random.RandomState(5)
    wide = {k: (batch[k].astype(np.float64) + 1e-9 * rs.randn(*batch[k].shape)) for k in ("state", "action", "next_state")}
    narrow = dict(batch, **{k: v.astype(np.float32) for k, v in wide.items()})
    noise = rs.randn(b, a).astype(np.float32)
    m0, v0 = _moments(online, 78)
    ys = []
    for mode in ("f32", "f64"):
        packed = _Packed(dev, shp, 3, online=online, target=target, m=m0, v=v0)
        ws = torch.zeros(dpg_mlp.workspace_floats(b, shp), dtype=torch.float32, device=dev)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        if mode == "f32":
            st_, ns_, ac_ = up(narrow["state"]), up(narrow["next_state"]), up(narrow["action"])
        else:
            block = up(np.stack([wide["state"], wide["next_state"]], axis=1))       # [B, 2, S]
            st_, ns_, ac_ = block[:, 0], block[:, 1], up(wide["action"])
            assert st_.stride(0) == 2 * s
        bs = dpg_mlp.Update.batch_struct(st_, ac_, up(batch["reward"]), ns_, up(batch["mask"]), up(noise))
        on, tg, step = packed.net("online"), packed.net("target"), _step_struct(packed, hp, 1)
        lib.dra_dpg_critic_update(ctypes.byref(on), ctypes.byref(tg), ctypes.byref(bs), ctypes.byref(step), ws.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        ys.append((ws[:4 * b].cpu().numpy(), packed.read("online")[0]))
    assert np.array_equal(ys[0][0].view(np.uint32), ys[1][0].view(np.uint32))
    assert np.array_equal(ys[0][1].view(np.uint32), ys[1][1].view(np.uint32))


@pytest.mark.parametrize("n", [1, 17, 128])
def test_act_matches_restatement(dra, n):
    """dra_dpg_act for n rows (fp32 and fp64 observations) against the restatement's actor."""
    from deeprl_amd import dpg_mlp
    from deeprl_amd._lib import lib, stream_ptr
    dev = dra.Config.DEVICE
    dims = (n, 17, 6, 400, 300)
    online, _, _, _ = K.random_case(dims, 1, 40 + n, head_scale=3.0)
    packed = _Packed(dev, (17, 6, 400, 300, K.GATE_RELU, 1), 9, online=online)
    obs = np.random.RandomState(n).randn(n, 17).astype(np.float32)
    want = R.actor(online, R.f64(obs), K.GATE_RELU).numpy()
    net = packed.net("online")
    outs = []
    for dt in (torch.float32, torch.float64):
        x = torch.from_numpy(obs).to(dev).to(dt)
        out = torch.full((n + 1, 6), -7.25, dtype=torch.float32, device=dev)
        lib.dra_dpg_act(ctypes.byref(net), x.data_ptr(), 17, 1 if dt == torch.float64 else 0, n, out.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        assert (outs[-1][n] == -7.25).all()                   # nothing behind row n
    frac = _within(outs[0][:n], want, "action")
    record_parity("dra_dpg_act vs fp64 restatement n=%d (fraction of the bar)" % n, action=frac)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.abs(want).max() > 0.5


@pytest.mark.parametrize("case", sorted(K.FIXTURE_CASES))
def test_recorded_reference_updates_replayed(dra, case):
    """The reference's recorded update from its recorded state, the recorded randn_like draw passed through `noise`: online and
    target parameters land on the reference's "after" tensors at rtol 2e-4 / atol 2e-5; a critic-only TD3 step leaves the
    actor and the targets bit-unchanged."""
    dev = dra.Config.DEVICE
    g = np.load(K.FIXTURE)
    hp, _ = K.fixture_hyper(g)
    st, batch, noise, after = K.fixture_case(g, case)
    nc, policy = K.FIXTURE_CASES[case]
    b, s, a, h1, h2 = [int(x) for x in g[case.split("_")[0] + "_dims"]]
    packed = _Packed(dev, (s, a, h1, h2, K.GATE_RELU, nc), 1, online=st.online, target=st.target, m=st.m, v=st.v)
    _device_update(dev, packed, batch, hp, st.t_critic + 1, st.t_actor + 1, policy=policy, noise=noise)
    got = {k: packed.read(k) for k in ("online", "target", "m", "v")}
    worst = 0.0
    for name in ("online", "target"):
        for k in packed.keys:
            want = after[name][k].numpy()
            np.testing.assert_allclose(got[name][1][k], want, rtol=2e-4, atol=2e-5, err_msg="%s %s %s" % (case, name, k))
            worst = max(worst, float(np.max(np.abs(got[name][1][k] - want) / (2e-5 + 2e-4 * np.abs(want)))))
    record_parity("dpg update vs recorded reference update %s (fraction of the bar)" % case, params=worst)
    if not policy:
        for k in packed.keys:
            n = int(np.prod(packed.shapes[k]))
            sl = slice(packed.off[k], packed.off[k] + n)
            assert np.array_equal(got["target"][0][sl].view(np.uint32), packed.host["target"][sl].view(np.uint32))
            if k.startswith("a."):
                assert np.array_equal(got["online"][0][sl].view(np.uint32), packed.host["online"][sl].view(np.uint32))


def test_hash_noise_when_no_noise_is_passed(dra):
    """noise == NULL: y is the restatement's with gauss_noise(seed, counter, B, rows, A) (the counter-hash stream of
    csrc/cont_env.h); the next counter gives the next draw."""
    dev = dra.Config.DEVICE
    dims, nc, gate = (17, 5, 2, 20, 12), 2, K.GATE_RELU
    b, s, a, h1, h2 = dims
    online, target, batch, hp = K.random_case(dims, nc, 91, head_scale=3.0)
    m0, v0 = _moments(online, 92)
    seed, ys = 12345, []
    for counter in (6, 7):
        noise = R.hash_noise(seed, counter, b, a)
        want = R.target_y(target, batch, hp, nc, gate, noise).reshape(-1).numpy()
        packed = _Packed(dev, (s, a, h1, h2, gate, nc), 2, online=online, target=target, m=m0, v=v0)
        ws, _ = _device_update(dev, packed, batch, hp, 1, 1, policy=False, noise=None, counter=counter, seed=seed)
        frac = _within(ws[:b], want, "y at counter %d" % counter)
        record_parity("dpg hash noise y vs restatement counter %d (fraction of the bar)" % counter, y=frac)
        ys.append(ws[:b].copy())
        other = R.target_y(target, batch, hp, nc, gate, R.hash_noise(seed, counter + 1, b, a)).reshape(-1).numpy()
        assert np.abs(other - want).max() > 1e-3                 # the comparison can tell two counters apart
    assert not np.array_equal(ys[0], ys[1])


# ------------------------------------------------------------------------------------------ agents
def _agent(d, tag, fused=True, noisy=False, td3_noise=0.0, batch=8, warm_up=10):
    cfg = d.Config()
    cfg.merge(dict(game="fake", log_level=0, tag=tag))
    cfg.task_fn = lambda: fake_envs.ContinuousTask(seed=13, state_dim=5, action_dim=2, horizon=9)
    cfg.eval_env = cfg.task_fn()
    adam = lambda p: torch.optim.Adam(p, lr=1e-3)
    if tag == "ddpg":
        cfg.network_fn = lambda: d.DeterministicActorCriticNet(
            5, 2, actor_body=d.FCBody(5, (16, 16), gate=torch.relu), critic_body=d.FCBody(7, (16, 16), gate=torch.relu),
            actor_opt_fn=adam, critic_opt_fn=adam)
        cfg.replay_fn = lambda: d.UniformReplay(memory_size=200, batch_size=batch)
        cfg.random_process_fn = lambda: d.OrnsteinUhlenbeckProcess(size=(2,), std=d.LinearSchedule(0.2))
        cls = d.DDPGAgent
    else:
        cfg.network_fn = lambda: d.TD3Net(2, actor_body_fn=lambda: d.FCBody(5, (16, 16), gate=torch.relu, noisy_linear=noisy),
                                          critic_body_fn=lambda: d.FCBody(7, (16, 16), gate=torch.relu),
                                          actor_opt_fn=adam, critic_opt_fn=adam)
        cfg.replay_fn = lambda: d.ReplayWrapper(d.UniformReplay, dict(memory_size=200, batch_size=batch), False)
        cfg.random_process_fn = lambda: d.GaussianProcess(size=(2,), std=d.LinearSchedule(0.1))
        cfg.td3_noise, cfg.td3_noise_clip, cfg.td3_delay = td3_noise, 0.5, 2
        cls = d.TD3Agent
    cfg.discount, cfg.warm_up, cfg.target_network_mix, cfg.max_steps = 0.99, warm_up, 5e-3, 1e5
    cfg.fused_dpg_update = fused
    torch.manual_seed(7)
    np.random.seed(17)
    random.seed(17)
    return cls(cfg)


def _load(module, g, prefix):
    module.load_state_dict({k: torch.from_numpy(g[prefix + k]) for k in module.state_dict().keys()})


@pytest.mark.parametrize("tag", ["ddpg", "td3"])
def test_fused_agents_match_reference_run(golden, dra, tag):
    """test_gpu_more_agents.py::test_ddpg_td3_match_reference_run's run and assertions with fused_dpg_update on: 40 agent steps,
    same np.random consumption, the replay holds the same actions / rewards, online and target weights land on the reference's
    -- through the fused launches (counted), with .grad left None."""
    d = dra
    g = golden("ddpg_td3_agents")
    agent = _agent(d, tag)
    k = tag + "_"
    _load(agent.network, g, k + "init_")
    agent.target_network.load_state_dict(agent.network.state_dict())
    for _ in range(40):
        agent.step()
    fused = agent._fused_dpg()
    assert fused is not None and fused.t_critic == 31 and fused.t_actor == (31 if tag == "ddpg" else 15)
    assert fused.launches == 30 + 2 * fused.t_critic + 3 * fused.t_actor          # 30 acting forwards after the warm-up
    assert all(p.grad is None for p in agent.network.parameters())
    assert agent.total_steps == int(g[k + "total_steps"])
    assert np.array_equal(np.random.randint(0, 1 << 30, size=4), g[k + "rng_tail"])
    rp = getattr(agent.replay, "replay", agent.replay)
    n = rp.size()
    acts = d.ops._wrap_device_pointer(rp._ring.pointers()[1], n * 2, torch.float64).cpu().numpy().reshape(n, 2)
    np.testing.assert_allclose(acts, g[k + "replay_action"], rtol=1e-5, atol=1e-6)
    rews = d.ops._wrap_device_pointer(rp._ring.pointers()[2], n, torch.float64).cpu().numpy()
    assert np.array_equal(rews, g[k + "replay_reward"])
    for name, v in agent.network.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), g[k + "final_" + name], rtol=2e-4, atol=2e-5, err_msg=name)
    for name, v in agent.target_network.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), g[k + "target_" + name], rtol=2e-4, atol=2e-5, err_msg="target " + name)
    agent.close()


def test_td3_cadence_on_the_fused_path(dra):
    """30 TD3 steps with td3_delay = 2 and smoothing noise on: the actor and the targets move exactly on the steps with
    total_steps % 2 != 0 (bit-equal before and after on the others), the critics on every warm step; the noise stream advances
    by one per update."""
    agent = _agent(dra, "td3", td3_noise=0.2, warm_up=6)
    flat = lambda net: torch.cat([p.detach().reshape(-1) for p in net.parameters()]).clone()
    actor = lambda net: torch.cat([p.detach().reshape(-1) for p in net.actor_params]).clone()
    critic = lambda net: torch.cat([p.detach().reshape(-1) for p in net.critic_params]).clone()
    updates = 0
    for _ in range(30):
        t0, a0, c0 = flat(agent.target_network), actor(agent.network), critic(agent.network)
        agent.step()
        t1, a1, c1 = flat(agent.target_network), actor(agent.network), critic(agent.network)
        warm = agent.total_steps >= 6
        policy = warm and agent.total_steps % 2 != 0
        updates += int(warm)
        assert torch.equal(t0, t1) != policy and torch.equal(a0, a1) != policy, agent.total_steps
        assert torch.equal(c0, c1) != warm, agent.total_steps
    fused = agent._fused_dpg()
    assert fused.updates == updates == fused.t_critic == 25 and fused.t_actor == 12
    agent.close()


def test_switch_on_but_ineligible_takes_the_module_path_with_one_warning(dra):
    """A noisy actor body: the module path runs (torch's optimisers step, gradients exist), and the agent says why, once."""
    agent = _agent(dra, "td3", noisy=True)
    for _ in range(14):
        agent.step()
    agent.eval_step(agent.state)
    assert agent._fused_dpg() is None
    assert len(agent.logger.warnings) == 1 and "fused_dpg_update" in agent.logger.warnings[0] and "network" in agent.logger.warnings[0]
    assert any(p.grad is not None for p in agent.network.parameters())
    assert len(agent.network.critic_opt.state) > 0
    agent.close()


def test_save_load_after_fused_updates(dra, tmp_path):
    """save after fused updates, load into a fresh agent: equal parameters (they are views of the flat buffers the kernels
    step), the same evaluation action, and the fresh agent steps on."""
    a = _agent(dra, "ddpg")
    for _ in range(20):
        a.step()
    path = str(tmp_path / "ddpg")
    a.save(path)
    b = _agent(dra, "ddpg")
    b.load(path)
    for (n1, p1), (n2, p2) in zip(a.network.state_dict().items(), b.network.state_dict().items()):
        assert n1 == n2 and torch.equal(p1, p2), n1
    obs = np.random.RandomState(3).randn(1, 5)
    assert np.array_equal(a.eval_step(obs), b.eval_step(obs))
    before = torch.cat([p.detach().reshape(-1) for p in b.network.parameters()]).clone()
    for _ in range(14):
        b.step()
    assert b._fused_dpg() is not None and b._fused_dpg().t_critic == 5
    assert not torch.equal(before, torch.cat([p.detach().reshape(-1) for p in b.network.parameters()]))
    a.close()
    b.close()


@pytest.mark.parametrize("fused", [False, True])
def test_td3_steps_on_the_synthetic_task(dra, fused):
    """TD3Agent on the synthetic continuous task, whose Box has scalar bounds (tools/bench_agents.py's td3 cases): both paths
    step past the warm-up and move the critics."""
    d = dra
    cfg = d.Config()
    cfg.merge(dict(game="synthetic-continuous-HalfCheetah", log_level=0, tag="td3", fused_dpg_update=fused))
    cfg.task_fn = lambda: d.Task(cfg.game, seed=1)
    cfg.eval_env = d.Task(cfg.game, seed=2)
    adam = lambda p: torch.optim.Adam(p, lr=1e-3)
    cfg.network_fn = lambda: d.TD3Net(cfg.action_dim, actor_body_fn=lambda: d.FCBody(cfg.state_dim, (20, 12), gate=torch.relu),
                                      critic_body_fn=lambda: d.FCBody(cfg.state_dim + cfg.action_dim, (20, 12), gate=torch.relu),
                                      actor_opt_fn=adam, critic_opt_fn=adam)
    cfg.replay_fn = lambda: d.ReplayWrapper(d.UniformReplay, dict(memory_size=100, batch_size=9))
    cfg.random_process_fn = lambda: d.GaussianProcess(size=(cfg.action_dim,), std=d.LinearSchedule(0.1))
    cfg.td3_noise, cfg.td3_noise_clip, cfg.td3_delay = 0.2, 0.5, 2
    cfg.discount, cfg.warm_up, cfg.target_network_mix, cfg.max_steps = 0.99, 10, 5e-3, 1e5
    agent = d.TD3Agent(cfg)
    before = torch.cat([p.detach().reshape(-1) for p in agent.network.critic_params]).clone()
    for _ in range(14):
        agent.step()
    assert (agent._fused_dpg() is not None) == fused
    after = torch.cat([p.detach().reshape(-1) for p in agent.network.critic_params])
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    agent.close()
