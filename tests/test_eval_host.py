"""Evaluation on the device (csrc/eval_act.h, dqn_mlp.Step.evaluate, config.fused_eval), the part that needs no GPU: the
restatement the GPU tests lean on (tests/eval_restatement.py) is pinned to BaseAgent.eval_episodes of the project's own agents
built on the CPU and to the reference's DQNAgent.eval_episodes (recorded in tests/golden/eval_feature/, and live where the
reference checkout is present); every case of tests/eval_cases.py keeps the margin condition; the struct mirror is the header's
and the entry points refuse what they must before any launch."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

import eval_cases as C
import eval_restatement as E
import ref_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_feature", "eval_reference.json")
GAME = "classic-CartPole-v0"
ENTRY = {"dqn": "dqn_feature", ("dist", "c51"): "categorical_dqn_feature", ("dist", "qr"): "quantile_regression_dqn_feature",
         "rainbow": "rainbow_feature"}


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


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_cases_keep_the_margin_condition(case):
    """Every launch of every case: the smallest |q1 - q0| is at least 100 bars of the q comparison (1e-5 of the largest |q|, floor
    1), the fp32 restatement takes the same trajectory, the five-episode launches end both ways, horizon 1 ends an episode per
    step, and one episode is the first of the five."""
    got = C.restated(case)
    forward = E.forward_of(case[0], case[2], got["spec"], got["noise"])
    for label, (n_episodes, horizon, junk, both) in C.LAUNCHES.items():
        want = got["runs"][label]
        assert want["margin"] >= E.MARGIN_BARS * E.q_bar(want) and E.comparable(want, horizon, both), label
        assert len(want["returns"]) == n_episodes and want["steps"] == int(want["lengths"].sum()) == want["q"].shape[0]
        assert np.array_equal(want["returns"], want["lengths"].astype(np.float64)) and want["lengths"].max() <= horizon
        assert want["counter"] == (C.JUNK["counter"] if junk else 0) + want["steps"] and want["ep_steps"] == 0 and want["ep_return"] == 0.0
        w32 = E.evaluate(forward, got["params"], C.make_env(junk, horizon), n_episodes, dtype=torch.float32)
        assert np.array_equal(w32["lengths"], want["lengths"]) and np.array_equal(w32["state"], want["state"]), label
        if both:
            assert (want["lengths"] == horizon).any() and (want["lengths"] < horizon).any()
    assert got["runs"]["every_step_ends"]["steps"] == 5
    assert got["runs"]["one"]["returns"][0] == got["runs"]["five"]["returns"][0]
    assert not np.array_equal(got["runs"]["junk_start"]["state"], got["runs"]["five"]["state"])


def test_the_issue_s_case_is_the_first_one():
    """dqn_feature_restatement.init_params(64, seed=0) over CartPole(seed=40, horizon=12): returns [12, 11, 12, 9, 12], the
    smallest margin 4.2e-3, the largest |q| 3.3."""
    got = C.restated(C.CASES[0])
    want = got["runs"]["five"]
    assert got["bump"] == 0 and list(want["returns"]) == [12, 11, 12, 9, 12]
    assert abs(want["margin"] - 4.2e-3) < 1e-4 and abs(want["scale"] - 3.3) < 0.05


# ------------------------------------------------------------------------------------------ the product's host loop
def _host_agent(case, n_episodes, horizon, junk):
    """The product's agent of the case's kind, built on the CPU through the zoo, with the evaluation environment of the launch.  The
    product's layers run on the device only (there is no CPU path), so the agent's network is stood in for by the case's fp32
    torch forward over the same weights, in the dict form the agent's eval_step reads; BaseAgent.eval_episodes / eval_episode,
    the agent's eval_step, the normaliser, Task, DummyVecEnv and CartPole are the product's own."""
    import deeprl_amd as d
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    d.select_device(-1)
    kind, hidden, gate, head = case[:4]
    got = C.restated(case)
    rec = _Rec()
    mp = pytest.MonkeyPatch()
    mp.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    try:
        c = zoo.config(ENTRY[kind if kind != "dist" else (kind, head)], game=GAME, tag="eval_host", overrides=dict(eval_episodes=n_episodes))
        c.task_fn = lambda: d.Task(GAME, seed=3, synthetic_done_period=horizon)
        c.eval_env = d.Task(GAME, seed=C.ENV_SEED, synthetic_done_period=horizon)
        if junk:
            c.eval_env.env.envs[0].c = C.JUNK["counter"]
        if kind != "dqn" and head == "c51":
            c.categorical_n_atoms, c.categorical_v_min, c.categorical_v_max = got["spec"]["n"], got["spec"]["v_min"], got["spec"]["v_max"]
        agent = getattr(d, zoo.ZOO[ENTRY[kind if kind != "dist" else (kind, head)]]["agent"])(c)
    finally:
        mp.undo()
    p32 = E.QR.to_t(got["params"], torch.float32)
    forward = E.forward_of(kind, gate, got["spec"], got["noise"])
    import dist_feature_restatement as DR
    import rainbow_feature_restatement as RR

    def network(state):
        obs = np.asarray(state, dtype=np.float32).reshape(1, 4)
        with torch.no_grad():
            if kind == "dqn":
                return dict(q=forward(p32, obs))
            if kind == "dist" and head == "qr":
                return dict(quantile=DR.head_out(p32, obs, got["spec"], gate))
            if kind == "dist":
                return dict(prob=torch.softmax(DR.head_out(p32, obs, got["spec"], gate), dim=-1))
            z = {k: torch.as_tensor(v) for k, v in got["noise"].items()}
            return dict(prob=torch.softmax(RR.logits(p32, z, obs, got["spec"]["n"], gate), dim=-1))
    agent.network = network
    if hasattr(agent, "atoms"):
        agent.atoms = torch.as_tensor(E.DR.atoms(got["spec"]))
    return agent, rec


@pytest.mark.parametrize("label", list(C.LAUNCHES))
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_restatement_is_the_product_s_host_evaluation(case, label):
    """BaseAgent.eval_episodes of the product's agent over the product's Task: the same returns per episode, the same record and
    mean, and the environment left where the restatement leaves it."""
    n_episodes, horizon, junk, _ = C.LAUNCHES[label]
    want = C.restated(case)["runs"][label]
    agent, rec = _host_agent(case, n_episodes, horizon, junk)
    returns, episode = [], agent.eval_episode
    agent.eval_episode = lambda: (returns.append(episode()), returns[-1])[1]
    out = agent.eval_episodes()
    env = agent.config.eval_env.env.envs[0]
    assert returns == list(want["returns"])
    mean, sem = want["returns"].mean(), want["returns"].std() / np.sqrt(n_episodes)
    assert out == {'episodic_return_test': mean}
    assert [ln for ln in rec.lines if 'episodic_return_test' in ln] == ['steps 0, episodic_return_test %.2f(%.2f)' % (mean, sem)]
    assert env.c == want["counter"] and env.steps == 0 and env.ret == 0.0
    assert np.array_equal(np.asarray(env.s).view(np.uint64), want["state"].view(np.uint64))


# ------------------------------------------------------------------------------------------ the reference
DQN_CASES = [c for c in C.CASES if c[0] == "dqn"]


@pytest.mark.parametrize("case", DQN_CASES, ids=C.case_id)
def test_restatement_is_the_reference_s_recorded_evaluation(case):
    """tests/golden/eval_feature/eval_reference.json (make_golden_eval_feature.py: the reference's DQNAgent.eval_episodes over the
    case's weights and envs.CartPole): the same returns for every launch."""
    rec = json.load(open(GOLDEN))[C.case_id(case)]
    got = C.restated(case)
    assert sorted(rec) == sorted(C.LAUNCHES)
    for label in C.LAUNCHES:
        assert rec[label] == list(got["runs"][label]["returns"]), label


@pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")
def test_recorded_evaluation_is_what_the_reference_computes_now():
    """Where the reference checkout is present: its DQNAgent.eval_episodes, run live, gives the recorded returns."""
    threads = torch.get_num_threads()       # (the generator modules run on one thread and say so when they are imported)
    try:
        from golden import make_golden_eval_feature as MG
        rec = json.load(open(GOLDEN))
        for case in (DQN_CASES[0], DQN_CASES[3]):
            for label in ("five", "junk_start"):
                assert MG.reference_eval(case, label) == rec[C.case_id(case)][label]
    finally:
        torch.set_num_threads(threads)


# ------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirror_matches_the_header(tmp_path):
    from deeprl_amd import dqn_mlp
    from test_struct_layouts import _c_layout
    names = [f[0] for f in dqn_mlp.EvalIO._fields_]
    got = _c_layout(tmp_path, "dra_mlp_eval_io", names)
    assert got[0] == ctypes.sizeof(dqn_mlp.EvalIO)
    assert got[1:] == [getattr(dqn_mlp.EvalIO, n).offset for n in names]


def test_supported_table():
    from deeprl_amd import dqn_mlp
    ok = dqn_mlp.eval_supported
    for n in (0, 1, 5, 10, 256, 257):
        for hz in (0, 1, 12, 200, 256, 257, 65536, 65537):
            assert ok(n, hz) == (1 <= n <= 256 and hz >= 1 and n * hz <= 65536), (n, hz)
    assert not ok(-1, 5) and not ok(5, -1) and not ok(2, 1 << 40)


def test_entry_points_refuse_before_any_launch():
    """Without a device: null structs, a net outside the shape table, n_episodes 0 and 257, n_episodes * horizon 65537, horizon 0
    and every null pointer are DRA_EINVAL."""
    from deeprl_amd import dist_mlp, dqn_mlp, rainbow_mlp
    from deeprl_amd._lib import lib
    io = dqn_mlp.EvalIO()
    nets = ((lib.dra_dqn_mlp_eval, dqn_mlp.Net()), (lib.dra_dist_mlp_eval, dist_mlp.Net()), (lib.dra_rainbow_mlp_eval, rainbow_mlp.Net()))
    for fn, net in nets:
        assert fn.raw(None, ctypes.byref(io), None) == -22 and fn.raw(ctypes.byref(net), None, None) == -22
        assert fn.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
        net.param = 4096
        net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, 64, 1
        if hasattr(net, "n_atoms"):
            net.n_atoms, net.v_min, net.v_max = 50, -10.0, 10.0
        if hasattr(net, "head"):
            net.head = 1
        if hasattr(net, "noise"):
            net.noise = 4096
        pointers = [f for f, t in dqn_mlp.EvalIO._fields_ if t is ctypes.c_void_p and f != "out_q"]
        for f in pointers:
            setattr(io, f, 4096)
        for n, hz in ((0, 12), (257, 12), (1, 65537), (241, 272), (5, 0), (5, -3)):
            io.n_episodes, io.horizon = n, hz
            assert fn.raw(ctypes.byref(net), ctypes.byref(io), None) == -22, (n, hz)
        io.n_episodes, io.horizon = 5, 12
        for f in pointers:
            setattr(io, f, None)
            assert fn.raw(ctypes.byref(net), ctypes.byref(io), None) == -22, f
            setattr(io, f, 4096)
        net.hidden = 48
        assert fn.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
        for f in pointers:
            setattr(io, f, None)


def test_kinds_name_their_evaluation_kernels():
    from deeprl_amd import dist_mlp, dqn_mlp, rainbow_mlp
    from deeprl_amd._lib import lib
    assert (dqn_mlp.Kind.EVAL, dist_mlp.Kind.EVAL, rainbow_mlp.Kind.EVAL) == ("dra_dqn_mlp_eval", "dra_dist_mlp_eval", "dra_rainbow_mlp_eval")
    assert all(k in lib.protos for k in ("dra_dqn_mlp_eval", "dra_dist_mlp_eval", "dra_rainbow_mlp_eval", "dra_mlp_eval_supported"))
