"""The device-resident Rainbow actor (config.device_noisy_actor; deeprl_amd/noisy_actor.py): its three kernels -- noisy layers
with one noise draw per row, the greedy action per row, the wrapping multi-slot ring feed -- and the agent on that path against
the reference's recorded run (tests/golden/rainbow_dueling.npz), against its own eager form and against the host-stepped path.

Bars.  Contractions and expected values: 1e-5 of each tensor's maximum (the bar of tests/test_gpu_noisy_rainbow.py).  Agent level:
the bars of tests/test_gpu_noisy_rainbow.py (2e-4 gate over the updates, rtol 3e-4 on the tree)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_envs  # noqa: E402
from golden.make_golden_cases import RAINBOW_SHAPES, HEAD_AGENT_CASES, digest, trajectory_digest  # noqa: E402
from parity_log import check_gated, check_trajectory, record_parity  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rainbow_dueling.npz")
BAR = 1e-5
GATE = 2e-4


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


def _f(e):
    return e.sign() * e.abs().sqrt()


def _rel(got, want):
    scale = max(float(want.abs().max()), 1e-30)
    return float((got.double().cpu() - want.cpu()).abs().max()) / scale


# ------------------------------------------------------------------------------------------------ kernels
ROW_SHAPES = [(1, 3136, 512), (4, 3136, 512), (8, 512, 51), (4, 512, 204), (3, 20, 1), (5, 7, 3)]


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=["%dx%dx%d" % s for s in ROW_SHAPES])
def test_noisy_linear_fwd_rows_equals_the_single_row_kernel(dra, shape, act):
    ops = dra.ops
    rows, k, n = shape
    gen = torch.Generator().manual_seed(31 * rows + k + n + (5 if act else 0))
    r = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    x = torch.relu(r(rows, k))
    bound = 1.0 / np.sqrt(k)
    wmu, bmu = (torch.rand(n, k, generator=gen) * 2 - 1) * bound, (torch.rand(n, generator=gen) * 2 - 1) * bound
    wsig, bsig = torch.full((n, k), 0.5 / np.sqrt(k)) * (1 + 0.1 * r(n, k)), torch.full((n,), 0.5 / np.sqrt(n)) * (1 + 0.1 * r(n))
    e_in, e_out, e_b = r(rows, k) * 0.5, r(rows, n) * 0.5, r(rows, n) * 0.5        # every row its own draw
    c = [v.cuda() for v in (x, wmu, wsig, bmu, bsig, e_in, e_out, e_b)]
    got = ops.noisy_linear_fwd_rows(*c, act=act)
    assert torch.equal(got, ops.noisy_linear_fwd_rows(*c, act=act)), "two calls differ"
    # the same rows out of ONE [rows, numel] block (the layout of _NoiseBlock.draw_rows): padded slices, one row stride
    pad = lambda m: (m + 3) // 4 * 4   # noqa: E731
    block = torch.zeros(rows, pad(k) + 2 * pad(n) + 8)
    o1, o2 = pad(k), pad(k) + pad(n)
    block[:, :k], block[:, o1:o1 + n], block[:, o2:o2 + n] = e_in, e_out, e_b
    block = block.cuda()
    strided = ops.noisy_linear_fwd_rows(*c[:5], block[:, :k], block[:, o1:o1 + n], block[:, o2:o2 + n], act=act)
    assert torch.equal(got, strided), "dense and strided noise rows differ"
    worst = 0.0
    for i in range(rows):
        one = ops.noisy_linear_fwd(c[0][i:i + 1].clone(), c[1], c[2], c[3], c[4], c[5][i].clone(), c[6][i].clone(), c[7][i].clone(),
                                   act=act)
        assert torch.equal(got[i:i + 1], one), "row %d is not the single-row kernel's" % i
        w = wmu.double() + wsig.double() * torch.outer(_f(e_out[i].double()), _f(e_in[i].double()))
        pre = x[i].double() @ w.t() + (bmu.double() + bsig.double() * _f(e_b[i].double()))
        want = torch.relu(pre) if act == "relu" else pre
        worst = max(worst, _rel(got[i], want))
    if rows > 1 and act is None:    # a kernel that reuses row 0's noise would repeat row 0's function on the other rows (a ReLU may hide it)
        reuse = ops.noisy_linear_fwd(c[0][1:2].clone(), c[1], c[2], c[3], c[4], c[5][0].clone(), c[6][0].clone(), c[7][0].clone(), act=act)
        assert not torch.equal(got[1:2], reuse)
    print("noisy rows %s act=%s: fp64 %.2e" % (shape, act, worst))
    record_parity("noisy_linear_fwd_rows %dx%dx%d act=%s" % (rows, k, n, act), y=worst)
    assert worst <= BAR, worst


def _act_ref64(value, adv, atoms):
    v, a, z = value.double(), adv.double(), atoms.double()
    logits = v[:, None, :] + (a - a.mean(1, keepdim=True))
    return (torch.softmax(logits, dim=-1) * z).sum(-1)


ACT_SHAPES = [(1, 4, 51), (4, 4, 51), (8, 2, 3), (3, 64, 64), (2, 1, 51)]


@pytest.mark.parametrize("shape", ACT_SHAPES, ids=["%dx%dx%d" % s for s in ACT_SHAPES])
def test_rainbow_act_rows_matches_fp64(dra, shape):
    ops = dra.ops
    rows, n_act, n_atoms = shape
    gen = torch.Generator().manual_seed(13 + 100 * rows + 10 * n_act + n_atoms)
    value, adv = torch.randn(rows, n_atoms, generator=gen), torch.randn(rows, n_act, n_atoms, generator=gen)
    atoms = torch.linspace(-10, 10, n_atoms)
    q64 = _act_ref64(value, adv, atoms)
    scale = float(q64.abs().max())
    if n_act > 1:       # the seeded inputs owe an unambiguous argmax: top-two gap of every row, on the CPU, before any launch
        top = q64.topk(2, dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min())
        assert gap >= 1e-3 * scale, "the test's inputs have a near tie (gap %.3g of scale %.3g): choose another seed" % (gap, scale)
    action, q = ops.rainbow_act_rows(value.cuda(), adv.cuda(), atoms.cuda(), want_q=True)
    err = _rel(q, q64)
    print("rainbow_act_rows %s: q fp64 %.2e" % (shape, err))
    record_parity("rainbow_act_rows %dx%dx%d" % shape, q=err)
    assert err <= BAR, err
    assert action.dtype == torch.int64 and action.cpu().tolist() == q64.argmax(1).tolist()
    only, none = ops.rainbow_act_rows(value.cuda(), adv.cuda(), atoms.cuda())
    assert none is None and torch.equal(only, action)
    into = torch.full((rows,), -1, dtype=torch.int64, device="cuda")
    ops.rainbow_act_rows(value.cuda(), adv.cuda(), atoms.cuda(), action=into)
    assert torch.equal(into, action)


@pytest.mark.parametrize("tie", ["first_pair", "last_pair", "all"])
def test_rainbow_act_rows_takes_the_first_maximum(dra, tie):
    """Identical advantage slices give identical bits of q: np.argmax's first maximum is the lower index."""
    ops = dra.ops
    rows, n_act, n_atoms = 4, 6, 51
    gen = torch.Generator().manual_seed(3)
    atoms = torch.linspace(-10, 10, n_atoms)
    value = torch.randn(rows, n_atoms, generator=gen)
    adv = 0.1 * torch.randn(rows, n_act, n_atoms, generator=gen)
    high = 0.3 * atoms + 0.1 * torch.randn(rows, n_atoms, generator=gen)     # mass on the high atoms: the largest expected value
    pair = dict(first_pair=(0, 1), last_pair=(n_act - 2, n_act - 1), all=tuple(range(n_act)))[tie]
    for a in pair:
        adv[:, a] = high
    q64 = _act_ref64(value, adv, atoms)
    others = [a for a in range(n_act) if a not in pair]
    if others:
        assert float((q64[:, pair[0]] - q64[:, others].max(1).values).min()) >= 1e-3 * float(q64.abs().max())
    action, q = ops.rainbow_act_rows(value.cuda(), adv.cuda(), atoms.cuda(), want_q=True)
    assert all(torch.equal(q[:, pair[0]], q[:, a]) for a in pair)
    assert action.cpu().tolist() == [pair[0]] * rows


@pytest.mark.parametrize("frame_bytes", [7056, 100], ids=["vec16", "bytes"])
def test_ring_put_rows_equals_put_device_per_slot(dra, frame_bytes):
    d = dra
    from deeprl_amd._lib import DraError
    cap, hist = 10, 4
    gen = torch.Generator().manual_seed(17)
    stacks = torch.randint(0, 256, (9, hist, frame_bytes), generator=gen, dtype=torch.uint8).cuda()
    actions = torch.randint(0, 18, (9,), generator=gen, dtype=torch.int64).cuda()
    rewards = torch.randn(9, generator=gen, dtype=torch.float64).cuda()
    masks = torch.randint(0, 2, (9,), generator=gen, dtype=torch.int32).cuda()
    newest = stacks[:, hist - 1]                 # strided: the newest frame of every stack (a ninth row for the refused count)
    assert not newest.is_contiguous()
    rows_ring, slot_ring = (d.ops.Ring(cap, frame_bytes, 8, hist, 1, 0.99) for _ in range(2))

    def snapshot(ring):
        return [t.clone() for t in ring.arrays()]

    def zero(ring):
        for t in ring.arrays():
            t.zero_()
    for count in (1, 4, 8):
        for first in (0, 7, 9):
            for by_value in (False, True):
                zero(rows_ring), zero(slot_ring)
                if by_value:
                    rows_ring.put_rows(count, newest, hist * frame_bytes, actions, rewards, masks, slot0=first)
                else:
                    word = torch.tensor([first], dtype=torch.int64, device="cuda")
                    rows_ring.put_rows(count, newest, hist * frame_bytes, actions, rewards, masks, slot0_dev=word)
                for k in range(count):
                    slot_ring.put_device((first + k) % cap, newest[k].contiguous(), actions=actions[k:k + 1], rewards=rewards[k:k + 1],
                                         masks=masks[k:k + 1])
                torch.cuda.synchronize()
                for name, a, b in zip(("frames", "actions", "rewards", "masks"), snapshot(rows_ring), snapshot(slot_ring)):
                    assert torch.equal(a, b), (name, count, first, by_value)
                written = sorted((first + k) % cap for k in range(count))
                touched = rows_ring.arrays()[0].view(cap, frame_bytes).ne(0).any(1).nonzero().flatten().tolist()
                assert touched == written, (touched, written)
    zero(rows_ring)
    for bad in (dict(count=0), dict(count=9), dict(count=4, slot0=-1), dict(count=4, slot0=cap)):
        with pytest.raises(DraError, match="-22"):
            rows_ring.put_rows(bad["count"], newest, hist * frame_bytes, actions, rewards, masks, slot0=bad.get("slot0", 0))
    with pytest.raises(DraError, match="-22"):
        word = torch.tensor([0], dtype=torch.int64, device="cuda")
        rows_ring.put_rows(9, newest, hist * frame_bytes, actions, rewards, masks, slot0_dev=word)
    torch.cuda.synchronize()
    assert not any(bool(t.ne(0).any()) for t in rows_ring.arrays()), "a refused call wrote"
    rows_ring.close(), slot_ring.close()


# ------------------------------------------------------------------------------------------------ agent
class _Log:
    def __init__(self):
        self.warnings = []

    def info(self, *a, **k):
        pass

    def add_scalar(self, *a, **k):
        pass

    def add_histogram(self, *a, **k):
        pass

    def warning(self, msg, *a, **k):
        self.warnings.append(str(msg))


def _load(net, shapes, seed):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in fake_envs.numpy_params(shapes, seed).items()}, strict=False)


def _agent(d, patch, memory_size=500, n_step=1, exploration_steps=40, **overrides):
    """The configuration of tests/test_gpu_noisy_rainbow.py::_rainbow_agent; overrides go on top."""
    import deeprl_amd.agents as agents_mod
    log = _Log()
    patch.setattr(agents_mod, "get_logger", lambda *a, **k: log)
    d.Config.NOISY_LAYER_STD = 0.5
    cfg = d.Config()
    cfg.merge(dict(game="synthetic-atari", n_step=n_step, replay_cls=d.PrioritizedReplay, async_replay=False, log_level=0, tag="rainbow",
                   noisy_linear=True))
    cfg.merge(overrides)
    cfg.task_fn = lambda: d.Task(cfg.game, seed=7, synthetic_done_period=8)
    cfg.eval_env = cfg.task_fn()
    cfg.optimizer_fn = lambda p: torch.optim.Adam(p, lr=0.000625, eps=1.5e-4)
    cfg.categorical_v_max, cfg.categorical_v_min, cfg.categorical_n_atoms = 10, -10, 51
    cfg.network_fn = lambda: d.RainbowNet(cfg.action_dim, cfg.categorical_n_atoms, d.NatureConvBody(noisy_linear=True),
                                          noisy_linear=True)
    cfg.random_action_prob = d.LinearSchedule(1.0, 0.05, 60)
    cfg.batch_size, cfg.discount, cfg.history_length = 32, 0.99, 4
    kw = dict(memory_size=memory_size, batch_size=32, n_step=n_step, discount=0.99, history_length=4)
    cfg.replay_fn = lambda: d.ReplayWrapper(cfg.replay_cls, kw, cfg.async_replay)
    cfg.replay_eps, cfg.replay_alpha = 0.01, 0.5
    cfg.replay_beta = d.LinearSchedule(0.4, 1.0, 1000)
    cfg.state_normalizer, cfg.reward_normalizer = d.ImageNormalizer(), d.SignNormalizer()
    cfg.target_network_update_freq, cfg.exploration_steps, cfg.sgd_update_frequency = 3, exploration_steps, 4
    cfg.gradient_clip, cfg.double_q, cfg.async_actor, cfg.max_steps = 10, True, False, 1e5
    d.random_seed(3)
    random.seed(3)
    agent = d.CategoricalDQNAgent(cfg)
    _load(agent.network, RAINBOW_SHAPES, 35)
    agent.target_network.load_state_dict(agent.network.state_dict())
    torch.manual_seed(5)
    return agent, log


def _run(agent, steps, upd_steps=()):
    traj = []
    for t in range(steps):
        agent.step()
        if t in upd_steps:
            torch.cuda.synchronize()
            traj.append(trajectory_digest(dict(agent.network.named_parameters())))
    torch.cuda.synchronize()
    return traj


def _state(agent):
    """Everything two runs are compared on, on the host."""
    rp = agent.replay.replay
    out = dict(params={n: v.detach().cpu().clone() for n, v in agent.network.named_parameters()},
               ring=[t.cpu().clone() for t in rp._ring.arrays()], cursor=(rp.pos, rp.size()), total_steps=agent.total_steps,
               noise={n: b.detach().cpu().clone() for n, b in agent.network.named_buffers() if "noise_" in n},
               actor_steps=agent.actor._total_steps)
    if getattr(rp, "tree", None) is not None:
        out.update(tree=rp.tree.as_tensor().cpu().clone(), max_priority=float(rp.max_priority), write=rp._write,
                   pending=sorted(rp._pending))
    return out


def _tails():
    return (torch.randint(0, 1 << 30, (4,)).numpy(), np.random.randint(0, 1 << 30, size=4), [random.getrandbits(30) for _ in range(2)])


@pytest.fixture(scope="module")
def device_run(dra):
    """The `rainbow` case (24 agent steps, 96 transitions, 14 updates) on the device path, once for the tests below."""
    d = dra
    g = np.load(GOLDEN)
    steps = dict(HEAD_AGENT_CASES)["rainbow"]
    with pytest.MonkeyPatch.context() as patch:
        agent, log = _agent(d, patch, device_noisy_actor=True, device_env=True)
        traj = _run(agent, steps, list(g["rainbow_update_steps"]))
        tails = _tails()
        out = dict(traj=traj, tails=tails, state=_state(agent), warnings=list(log.warnings),
                   on_device=agent._noisy_actor is not None,
                   actor_graph=agent._noisy_actor is not None and agent._noisy_actor.graph is not None,
                   update_graph=agent._graphed.graph is not None, graphed_q_calls=agent.actor._graphed_q.calls,
                   env_frames=agent.actor._task.env.envs[0].frames)
        agent.close()
    return out


def test_device_path_reproduces_the_reference_run(dra, device_run):
    """The `rainbow` case of tests/test_gpu_rainbow_dueling.py on the device path, the bars of tests/test_gpu_noisy_rainbow.py.
    Measured use of the 2e-4 gate: 7.9e-6 over the run's 14 updates (the host-stepped path: 7.9e-6 as well)."""
    d = dra
    g = np.load(GOLDEN)
    k = "rainbow_"
    run, st = device_run, device_run["state"]
    assert run["on_device"] and not run["warnings"], run["warnings"]
    assert run["actor_graph"], "the actor block was not captured"
    assert run["update_graph"], "the PER update was not captured"
    assert run["graphed_q_calls"] == 0, "_GraphedQ was used"
    assert run["env_frames"] == "device", "the host emulator was stepped"
    errs = check_trajectory("noisy_actor_trajectory", run["traj"], g[k + "update_digests"], gate_atol=GATE)
    print("trajectory: max per-update abs error %.3g (gate_atol %.1e)" % (max(errs), GATE))
    assert st["total_steps"] == int(g[k + "total_steps"]) and st["actor_steps"] == st["total_steps"]
    n = st["cursor"][1]
    assert list(st["cursor"]) == list(g[k + "pos_size"])
    frames, actions, rewards, masks = st["ring"]
    assert np.array_equal(actions.view(torch.int64)[:n].numpy(), g[k + "replay_action"])
    assert np.array_equal(rewards[:n].numpy(), g[k + "replay_reward"])
    assert np.array_equal(masks[:n].numpy(), g[k + "replay_mask"])
    np.testing.assert_allclose(st["tree"].numpy(), g[k + "tree"], rtol=3e-4, atol=1e-7)
    np.testing.assert_allclose(st["max_priority"], float(g[k + "max_priority"]), rtol=3e-4)
    assert np.array_equal(run["tails"][0], g[k + "torch_rng_tail"])
    assert np.array_equal(run["tails"][1], g[k + "np_rng_tail"])
    assert np.array_equal(run["tails"][2], g[k + "py_rng_tail"])
    worst = 0.0
    for name, v in st["params"].items():
        got, want = digest(v.numpy())[2:], g[k + "final_" + name][2:]
        worst = max(worst, float(np.abs(got - want).max()))
        check_gated(got, want, "final_" + name, gate_atol=GATE)
    record_parity("noisy_actor_final_parameters", max_abs=worst, max_update_abs=max(errs))


def _assert_same(a, b, what, keys=None):
    for key in keys or a.keys():
        x, y = a[key], b[key]
        if isinstance(x, dict):
            for n in x:
                assert torch.equal(x[n], y[n]), (what, key, n)
        elif isinstance(x, list) and x and isinstance(x[0], torch.Tensor):
            for i, (p, q) in enumerate(zip(x, y)):
                assert torch.equal(p, q), (what, key, i)
        elif isinstance(x, torch.Tensor):
            assert torch.equal(x, y), (what, key)
        else:
            assert x == y, (what, key, x, y)


def test_captured_and_eager_actor_are_bit_identical(dra, device_run, monkeypatch):
    d = dra
    agent, _ = _agent(d, monkeypatch, device_noisy_actor=True, device_env=True, graph_update=False)
    _run(agent, dict(HEAD_AGENT_CASES)["rainbow"])
    assert agent._noisy_actor is not None and agent._noisy_actor.graph is None and agent._graphed.graph is None
    eager = _state(agent)
    agent.close()
    _assert_same(device_run["state"], eager, "captured / eager")


@pytest.mark.parametrize("replay", ["per", "uniform_3step"])
def test_device_path_equals_host_path(dra, monkeypatch, replay):
    """16 agent steps over a ring of 50 slots (blocks wrap, sampled leaves are overwritten before their priority returns), updates
    from the sixth step on.  Both paths run the same update on the same ring contents: the parameters are asserted bit-identical,
    which is what was observed (the 2e-4 gate of the module's other tests is not needed)."""
    d = dra
    kw = dict(memory_size=50, exploration_steps=20)
    if replay == "uniform_3step":
        kw.update(replay_cls=d.UniformReplay, n_step=3)
    states = []
    for device in (True, False):
        agent, log = _agent(d, monkeypatch, device_noisy_actor=device, device_env=True, **kw)
        _run(agent, 16)
        assert (agent._noisy_actor is not None) == device and not log.warnings
        assert agent._graphed.graph is not None, "no update was captured"
        states.append(_state(agent))
        states[-1]["tails"] = [np.asarray(t).tolist() for t in _tails()]
        agent.close()
    dev, host = states
    assert dev["cursor"] == host["cursor"] == (64 % 50, 50)
    worst = max(float((dev["params"][n].double() - host["params"][n].double()).abs().max()) for n in dev["params"])
    print("device / host path (%s): max parameter difference %.3g" % (replay, worst))
    record_parity("noisy_actor_device_vs_host %s" % replay, max_param_abs=worst)
    _assert_same(dev, host, "device / host (%s)" % replay, keys=[k for k in dev if k != "params"])
    assert worst <= GATE, worst
    _assert_same(dev, host, "device / host (%s)" % replay, keys=["params"])


def test_ineligible_agent_warns_once_and_keeps_the_host_path(dra, monkeypatch):
    d = dra
    states = []
    for switch in (True, False):
        agent, log = _agent(d, monkeypatch, device_noisy_actor=switch, device_env=False)
        _run(agent, 12)
        assert agent._noisy_actor is None and agent.actor._graphed_q.calls > 0
        if switch:
            assert len(log.warnings) == 1 and "device_env is False" in log.warnings[0], log.warnings
        else:
            assert not log.warnings
        states.append(_state(agent))
        agent.close()
    _assert_same(states[0], states[1], "switch on, ineligible / switch off")


def test_save_full_raises_and_save_load_round_trips(dra, monkeypatch, tmp_path):
    d = dra
    agent, _ = _agent(d, monkeypatch, device_noisy_actor=True, device_env=True)
    _run(agent, 12)
    name = str(tmp_path / "rainbow")
    with pytest.raises(NotImplementedError, match="device_noisy_actor"):
        agent.save_full(name)
    assert not os.path.exists(name + ".resume") and not os.path.exists(name + ".model"), "an incomplete checkpoint was written"
    with pytest.raises(NotImplementedError, match="device_noisy_actor"):
        agent.load_full(name)
    agent.save(name)
    want = {k: v.detach().cpu().clone() for k, v in agent.network.state_dict().items()}
    f = d.NoisyLinear.transform_noise
    fc4 = agent.network.body.fc4
    assert torch.equal(want["body.fc4.weight_epsilon"], torch.outer(f(fc4.noise_out_weight), f(fc4.noise_in)).cpu())
    agent.close()
    other, _ = _agent(d, monkeypatch, device_noisy_actor=True, device_env=True)
    other.load(name)
    got = other.network.state_dict()
    for k, v in want.items():
        assert torch.equal(got[k].cpu(), v), k
    other.step()                     # goes on from the loaded parameters
    torch.cuda.synchronize()
    other.close()
