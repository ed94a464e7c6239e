"""Evaluation of DDPG / TD3 on the device (csrc/dpg_mlp.hip dra_dpg_eval, dpg_mlp.Update.evaluate, config.fused_eval), the part that
needs no GPU: the restatement the GPU tests lean on (tests/dpg_eval_restatement.py) is pinned three ways -- to
BaseAgent.eval_episodes of the project's own DDPG and TD3 agents built on the CPU, to the reference's DDPGAgent.eval_episodes
(recorded in tests/golden/dpg_eval/, and live where the reference checkout is present), and to the parallel form the kernel
runs (episode e alone, from the counter c0 + e horizon); the struct mirror is the header's and the entry points refuse what they
must before any launch."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

import dpg_env_cases as K
import dpg_eval_cases as C
import dpg_eval_restatement as E
import dpg_restatement as R
import ref_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dpg_eval", "eval_reference.json")
GAME = "classic-Pendulum-v0"
# The bar between an fp32 actor's returns and the fp64 restatement's: the worst |reference's return - restatement's| over the three
# shapes at 5 x 12 (the reference's own fp32 torch forward; measured on the CPU by make_golden_dpg_eval.py's output against
# dpg_eval_cases.restated: 6.8e-7 at (32, 24) relu, 1.9e-6 at (20, 12) tanh, 1.1e-6 at (400, 300) relu), times 10 for the order in
# which another fp32 forward accumulates.
REF_WORST = 1.9e-6
TOL = 10 * REF_WORST


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


class _Rec:
    def __init__(self):
        self.lines = []

    def info(self, msg, *a, **k):
        self.lines.append(str(msg))
    warning = info

    def add_scalar(self, *a, **k):
        pass


def _forward32(shape):
    """network(state) -> the fp32 torch forward of the case's actor over the float32 observation, as a [1, 1] tensor."""
    p32 = {k: v.to(torch.float32) for k, v in C.params(shape).items()}

    def network(state):
        with torch.no_grad():
            return R.actor(p32, torch.as_tensor(np.asarray(state, dtype=np.float32).reshape(1, -1)), shape[4])
    return network


# ------------------------------------------------------------------------------------------ the product's host loop
def _host_agent(entry, shape, n_episodes, horizon, junk):
    """The product's DDPGAgent / TD3Agent built on the CPU through the zoo, with the evaluation environment of the launch.  The
    product's layers run on the device only (there is no CPU path), so the agent's network is stood in for by the case's fp32 torch
    forward over the same weights; BaseAgent.eval_episodes / eval_episode, the agent's eval_step, the normaliser, Task, DummyVecEnv
    and Pendulum are the product's own."""
    import deeprl_amd as d
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    d.select_device(-1)
    rec = _Rec()
    mp = pytest.MonkeyPatch()
    mp.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    try:
        c = zoo.config(entry, game=GAME, tag="dpg_eval_host", overrides=dict(eval_episodes=n_episodes))
        c.task_fn = lambda: d.Task(GAME, seed=3, synthetic_done_period=horizon)
        c.eval_env = d.Task(GAME, seed=C.ENV_SEED, synthetic_done_period=horizon)
        if junk:
            env = c.eval_env.env.envs[0]
            env.c, env.steps, env.ret = C.JUNK["counter"], C.JUNK["ep_steps"], C.JUNK["ep_return"]
            env.s = np.asarray(C.JUNK["state"], dtype=np.float64)
        c.replay_fn = lambda: d.UniformReplay(memory_size=24, batch_size=8)
        agent = getattr(d, zoo.ZOO[entry]["agent"])(c)
    finally:
        mp.undo()
    agent.network = _forward32(shape)
    return agent, rec


@pytest.mark.parametrize("label", list(C.LAUNCHES))
@pytest.mark.parametrize("shape", C.SHAPES[:2], ids=C.shape_id)
@pytest.mark.parametrize("entry", ["ddpg_continuous", "td3_continuous"])
def test_restatement_is_the_product_s_host_evaluation(entry, shape, label):
    """BaseAgent.eval_episodes of the product's agent over the product's Task: under the same fp32 forward the restated loop gives
    the same returns per episode to the bit, the same record and mean, and leaves the environment where the agent's loop leaves
    it; the fp64 restatement of the case stays within TOL of those returns and leaves the same counter."""
    n_episodes, horizon, junk = C.LAUNCHES[label]
    agent, rec = _host_agent(entry, shape, n_episodes, horizon, junk)
    forward = agent.network
    want = E.evaluate(lambda obs: forward(obs).numpy().reshape(-1), C.make_env(junk, horizon), n_episodes)
    returns, episode = [], agent.eval_episode
    agent.eval_episode = lambda: (returns.append(episode()), returns[-1])[1]
    out = agent.eval_episodes()
    env = agent.config.eval_env.env.envs[0]
    assert returns == list(want["returns"])
    mean, sem = want["returns"].mean(), want["returns"].std() / np.sqrt(n_episodes)
    assert out == {'episodic_return_test': mean}
    assert [ln for ln in rec.lines if 'episodic_return_test' in ln] == ['steps 0, episodic_return_test %.2f(%.2f)' % (mean, sem)]
    assert (env.c, env.steps, env.ret) == (want["counter"], 0, 0.0) == (want["counter"], want["ep_steps"], want["ep_return"])
    assert np.array_equal(np.asarray(env.s).view(np.uint64), want["state"].view(np.uint64))
    w64 = C.restated(shape, label)
    worst = float(np.abs(w64["returns"] - want["returns"]).max())
    print("%s %s %s: fp32 forward against the fp64 restatement, worst %.3e (bar %.3e)" % (entry, C.shape_id(shape), label, worst, TOL))
    assert worst <= TOL
    assert w64["counter"] == want["counter"] == (C.JUNK["counter"] if junk else 0) + n_episodes * horizon
    assert np.array_equal(w64["state"].view(np.uint64), want["state"].view(np.uint64))      # (the reset state depends on the counter alone)


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_restatement_is_the_reference_s_recorded_evaluation(shape):
    """tests/golden/dpg_eval/eval_reference.json (make_golden_dpg_eval.py: the reference's DDPGAgent.eval_episodes over the
    shape's weights and envs.Pendulum at 5 x 12, its fp32 torch forward): within TOL of the fp64 restatement, and the measured
    worst difference is what the constant says."""
    rec = json.load(open(GOLDEN))
    assert sorted(rec) == sorted(C.shape_id(s) for s in C.SHAPES)
    want = C.restated(shape, "five")["returns"]
    worst = float(np.abs(np.asarray(rec[C.shape_id(shape)]) - want).max())
    print("%s: the reference against the fp64 restatement, worst %.3e" % (C.shape_id(shape), worst))
    assert worst <= REF_WORST < TOL


def test_reference_worst_difference_is_the_recorded_constant():
    rec = json.load(open(GOLDEN))
    worst = max(float(np.abs(np.asarray(rec[C.shape_id(s)]) - C.restated(s, "five")["returns"]).max()) for s in C.SHAPES)
    assert 0.9 * REF_WORST <= worst <= REF_WORST


@pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")
def test_recorded_evaluation_is_what_the_reference_computes_now():
    """Where the reference checkout is present: its DDPGAgent.eval_episodes, run live, gives the recorded returns."""
    threads = torch.get_num_threads()       # (the generator modules run on one thread and say so when they are imported)
    try:
        from golden import make_golden_dpg_eval as MG
        rec = json.load(open(GOLDEN))
        for shape in C.SHAPES[:2]:
            assert MG.reference_eval(shape) == rec[C.shape_id(shape)]
    finally:
        torch.set_num_threads(threads)


# ------------------------------------------------------------------------------------------ the parallel form
@pytest.mark.parametrize("label", list(C.LAUNCHES))
@pytest.mark.parametrize("shape", C.SHAPES[:2], ids=C.shape_id)
def test_sequential_episodes_are_independent_rows(shape, label):
    """Episode e of the host loop starts in pendulum_reset's state at c0 + e horizon -- by env.reset() and by the auto reset alike --
    so the sequential evaluation equals n independent episodes bit for bit: returns, every state, every action and the words the
    environment is left with."""
    from deeprl_amd.envs import Pendulum
    n_episodes, horizon, junk = C.LAUNCHES[label]
    want = C.restated(shape, label)
    c0 = C.JUNK["counter"] if junk else 0
    rows = E.evaluate_rows(E.actor_of(C.params(shape), shape[4]), C.ENV_SEED, horizon, c0, n_episodes)
    for k in ("returns", "states", "actions", "state"):
        assert np.array_equal(np.asarray(rows[k]).view(np.uint64), np.asarray(want[k]).view(np.uint64)), k
    assert [rows[k] for k in ("steps", "counter", "ep_steps", "ep_return")] == [want[k] for k in ("steps", "counter", "ep_steps", "ep_return")]
    assert want["states"].shape == (n_episodes, horizon + 1, 2) and want["actions"].shape == (n_episodes, horizon)
    for e in range(n_episodes):
        fresh = Pendulum(C.ENV_SEED, horizon=horizon)
        fresh.c = c0 + e * horizon
        fresh.reset()
        assert np.array_equal(np.asarray(fresh.s).view(np.uint64), want["states"][e, 0].view(np.uint64)), e
    if junk:
        assert not np.array_equal(want["states"], C.restated(shape, "five")["states"])


def test_twenty_sequential_zoo_episodes_equal_twenty_independent_ones():
    """The zoo's own count, 20 x 200, at (32, 24)."""
    n, horizon = C.ZOO_LAUNCH
    act = E.actor_of(C.params(C.SHAPES[0]), 1)
    seq = E.evaluate(act, C.make_env(False, horizon), n)
    rows = E.evaluate_rows(act, C.ENV_SEED, horizon, 0, n)
    for k in ("returns", "states", "actions", "state"):
        assert np.array_equal(np.asarray(rows[k]).view(np.uint64), np.asarray(seq[k]).view(np.uint64)), k
    assert seq["counter"] == rows["counter"] == n * horizon and seq["steps"] == n * horizon


# ------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirror_matches_the_header(tmp_path):
    from deeprl_amd import dpg_mlp
    from test_struct_layouts import _c_layout
    names = [f[0] for f in dpg_mlp.EvalIO._fields_]
    got = _c_layout(tmp_path, "dra_dpg_eval_io", names)
    assert got[0] == ctypes.sizeof(dpg_mlp.EvalIO)
    assert got[1:] == [getattr(dpg_mlp.EvalIO, n).offset for n in names]


def test_supported_table():
    from deeprl_amd import dpg_mlp
    ok = dpg_mlp.eval_supported
    for n in (0, 1, 5, 20, 128, 129):
        for hz in (0, 1, 12, 200, 512, 513, 65536, 65537):
            assert ok(n, hz, 3, 1, 400, 300, 1) == (1 <= n <= 128 and hz >= 1 and n * hz <= 65536), (n, hz)
    assert not ok(-1, 5, 3, 1, 32, 24, 1) and not ok(5, -1, 3, 1, 32, 24, 1) and not ok(2, 1 << 40, 3, 1, 32, 24, 1)
    assert ok(20, 200, 3, 1, 512, 512, 2) and ok(5, 12, 3, 1, 20, 12, 2)
    for s, a, h1, h2, gate in ((4, 1, 32, 24, 1), (3, 2, 32, 24, 1), (17, 6, 32, 24, 1), (3, 1, 513, 24, 1), (3, 1, 32, 0, 1), (3, 1, 32, 24, 3)):
        assert not ok(5, 12, s, a, h1, h2, gate), (s, a, h1, h2, gate)


def test_entry_point_refuses_before_any_launch():
    """Without a device: null structs, a net outside the shape table, n_episodes 0 and 129, n_episodes * horizon 65537, horizon 0
    and every null required pointer are DRA_EINVAL."""
    from deeprl_amd import dpg_mlp
    from deeprl_amd._lib import lib
    fn, io, net = lib.dra_dpg_eval, dpg_mlp.EvalIO(), dpg_mlp.Net()
    assert fn.raw(None, ctypes.byref(io), None) == -22 and fn.raw(ctypes.byref(net), None, None) == -22
    assert fn.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    net.param = 4096
    net.state_dim, net.action_dim, net.h1, net.h2, net.gate, net.n_critics = 3, 1, 32, 24, 1, 1
    required = [f for f, t in dpg_mlp.EvalIO._fields_ if t is ctypes.c_void_p and f not in ("out_state", "out_action")]
    for f in required:
        setattr(io, f, 4096)
    for n, hz in ((0, 12), (129, 12), (1, 65537), (121, 542), (5, 0), (5, -3)):
        io.n_episodes, io.horizon = n, hz
        assert fn.raw(ctypes.byref(net), ctypes.byref(io), None) == -22, (n, hz)
    io.n_episodes, io.horizon = 5, 12
    for f in required:
        setattr(io, f, None)
        assert fn.raw(ctypes.byref(net), ctypes.byref(io), None) == -22, f
        setattr(io, f, 4096)
    for field, bad in (("state_dim", 4), ("action_dim", 2), ("h1", 513), ("h2", 0), ("gate", 3)):
        keep = getattr(net, field)
        setattr(net, field, bad)
        assert fn.raw(ctypes.byref(net), ctypes.byref(io), None) == -22, field
        setattr(net, field, keep)


def test_default_config_keeps_the_host_evaluation():
    """With either switch off nothing changes: _fused_eval is None without touching the evaluation environment."""
    import types

    from deeprl_amd import agents
    for cfg in (types.SimpleNamespace(), types.SimpleNamespace(fused_eval=False, fused_dpg_update=True), types.SimpleNamespace(fused_eval=1)):
        assert agents._DeterministicPolicyAgent._fused_eval(types.SimpleNamespace(config=cfg)) is None
    fake = types.SimpleNamespace(config=types.SimpleNamespace(fused_eval=True, fused_dpg_update=False))
    fake._fused_dpg = lambda: agents._DeterministicPolicyAgent._fused_dpg(fake)
    assert agents._DeterministicPolicyAgent._fused_eval(fake) is None and fake._dpg is None
