"""dqn_feature on the device (csrc/dqn_mlp.hip, deeprl_amd/dqn_mlp.py), the part that needs no GPU: the restatement the GPU tests
lean on is pinned to the reference's own run (tests/golden/dqn_feature/), the draw planner to the host loop's draws, the struct
mirrors to the header, every why_not reason to its condition, and the case tables to what they claim to cover."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

import dqn_feature_cases as K
import dqn_feature_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dqn_feature")
FIXTURE = os.path.join(GOLDEN, "dqn_feature_steps.npz")
RANDOM = os.path.join(GOLDEN, "random_policy.json")
LEARNING = os.path.join(GOLDEN, "learning_reference.json")
NSTEP_FIXTURE = os.path.join(ROOT, "tests", "golden", "nstep_feature", "nstep_feature_step.npz")
TAGS = tuple(t[0] for t in K.FIXTURE_TAGS)
LENGTHS = (25000, 50000, 100000)
GAME = "classic-CartPole-v0"


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    """These tests seed np.random and switch the package's device; the tests after them see what they saw before."""
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


# ------------------------------------------------------------------------------------------ records
def test_random_policy_mean_is_the_committed_one():
    rec = json.load(open(RANDOM))
    assert rec["episodes"] == 2000 and rec["mean"] == K.random_policy_mean(rec["episodes"], rec["seed"], rec["env_seed"])
    assert 15.0 < rec["mean"] < 30.0


def test_learning_reference_record():
    """The reference's own DQNAgent on the entry: 5 seeds, the last-100 mean at every length, the bar 2 x the random policy's mean
    and n_learn the smallest length at which the median reaches 2 x the bar."""
    rec = json.load(open(LEARNING))
    assert rec["bar"] == 2.0 * json.load(open(RANDOM))["mean"] and abs(rec["bar"] - 44.2) < 0.1
    assert len(rec["runs"]) == 5 and sorted(rec["medians"]) == sorted(str(n) for n in LENGTHS)
    for n in LENGTHS:
        assert rec["medians"][str(n)] == float(np.median([r["ends"][str(n)]["last_mean"] for r in rec["runs"]]))
    reached = [n for n in LENGTHS if rec["medians"][str(n)] >= 2.0 * rec["bar"]]
    assert rec["n_learn"] == (reached[0] if reached else None)


def test_fixture_holds_data_only_and_is_small():
    z = np.load(FIXTURE, allow_pickle=False)
    assert all(z[k].dtype.kind in "fiub" for k in z.files)
    assert os.path.getsize(FIXTURE) <= os.path.getsize(NSTEP_FIXTURE) < (1 << 20)
    for tag in TAGS:
        assert z[tag + "_flags"].shape == (K.FIXTURE["steps"], K.FIXTURE["k"])
        assert z[tag + "_flags"].any() and (~z[tag + "_flags"]).any()
    assert (z["hz3_ring_masks"] == 0).any() and bool(z["double_q_cfg"][2]) and int(z["copy_cfg"][3]) == 5


def test_zoo_config_carries_the_switch():
    from deeprl_amd import zoo
    on = zoo.config("dqn_feature", game=GAME, tag="dqn_feat_switch_on", fused_dqn_feature=True)
    off = zoo.config("dqn_feature", game=GAME, tag="dqn_feat_switch_off")
    assert on.fused_dqn_feature is True and getattr(off, "fused_dqn_feature", False) is False


# ------------------------------------------------------------------------------------------ the restatement and the reference
def _fixture_run(z, tag):
    spec = next(t for t in K.FIXTURE_TAGS if t[0] == tag)
    _, task_seed, horizon, double_q, freq, hidden = spec
    f = K.FIXTURE
    init = {k: z["%s_init_%s" % (tag, k)] for k in R.KEYS}
    target0 = {k: z["%s_target0_%s" % (tag, k)] for k in R.KEYS}
    cfg = dict(k=f["k"], batch=f["batch"], capacity=f["capacity"], exploration_steps=f["exploration_steps"], target_freq=freq,
               discount=K.DISCOUNT, gradient_clip=K.GRADIENT_CLIP, lr=K.LR, double_q=double_q, gate="relu")
    env, _ = K.make_env(task_seed, horizon)
    rs = np.random.RandomState(f["np_seed"])
    out = R.agent_run(init, env, cfg, rs, K.epsilon_schedule(*f["eps"]), f["steps"], target0=target0)
    out["rng_tail"] = rs.randint(0, 1 << 30, size=3)
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_steps(tag):
    """R.agent_run on the fixture's configuration: actions, flags, random actions, the ring's four arrays, the sampled indices, pos
    and the np.random tail exactly; losses, the online parameters after every step and the target's at the end within rtol 2e-5 /
    atol 2e-6 (the reference computes in fp32)."""
    z = np.load(FIXTURE)
    got = _fixture_run(z, tag)
    assert np.array_equal(got["actions"], z[tag + "_actions"]) and np.array_equal(got["flags"], z[tag + "_flags"])
    assert np.array_equal(got["random_actions"], z[tag + "_random_actions"])
    assert got["total"] == int(z[tag + "_total_steps"]) and got["pos"] == int(z[tag + "_pos"])
    for k in ("frames", "rewards"):
        assert np.array_equal(got["ring"][k].view(np.uint64), z["%s_ring_%s" % (tag, k)].view(np.uint64)), k
    assert np.array_equal(got["ring"]["actions"], z[tag + "_ring_actions"]) and np.array_equal(got["ring"]["masks"], z[tag + "_ring_masks"])
    idx = np.stack([np.full(K.FIXTURE["batch"], -1) if i is None else i for i in got["indices"]])
    assert np.array_equal(idx, z[tag + "_indices"]) and (idx[-1] >= 0).all() and (idx[0] < 0).all()
    assert np.array_equal(got["rng_tail"], z[tag + "_rng_tail"])
    np.testing.assert_allclose(got["losses"], z[tag + "_losses"], rtol=2e-5, atol=2e-6)
    for k in R.KEYS:
        want = z["%s_params_%s" % (tag, k)]
        np.testing.assert_allclose(np.stack([p[k] for p in got["params"]]), want, rtol=2e-5, atol=2e-6, err_msg=k)
        np.testing.assert_allclose(got["target"][k], z["%s_target_%s" % (tag, k)], rtol=2e-5, atol=2e-6, err_msg=k)
    if tag == "copy":
        assert got["copies"] == [4, 9]
    if tag == "hz3":
        assert len(got["events"]) >= 12 and all(r == 3.0 for _, _, r in got["events"])


# ------------------------------------------------------------------------------------------ the draw planner
@pytest.mark.parametrize("exploration_steps", [0, 6, 8, 1000])
def test_planner_consumes_the_host_loop_s_draws(exploration_steps):
    """support.plan_actor_epsilon_greedy + UniformReplay's bookkeeping and draw_indices against the host loop's own calls
    (DQNActor._transition's epsilon, support.epsilon_greedy's 2-D branch, the scalar rejection loop): the same flags, random
    actions and indices, the same schedule position and np.random state -- also where exploration_steps is crossed in the middle
    of the four transitions (6)."""
    from deeprl_amd.support import LinearSchedule, epsilon_greedy, plan_actor_epsilon_greedy
    k_len, batch, cap, steps = 4, 10, 24, 8
    # the host loop
    np.random.seed(5)
    sched = LinearSchedule(0.8, 0.1, 30)
    q = np.asarray([[0.25, 0.75]])
    host, actor_steps, total, pos, size = [], 0, 0, 0, 0
    for _ in range(steps):
        flags = []
        for _ in range(k_len):
            eps = 1 if actor_steps < exploration_steps else sched()
            flags.append(int(epsilon_greedy(eps, q)[0]))         # 1: the greedy action; a random 1 cannot be told apart: the
            actor_steps += 1                                       # generator's state below can
            total += 1
            if pos >= size:
                size += 1
            pos = (pos + 1) % cap
        idx = None
        if total > exploration_steps:
            idx = R.draw_indices(np.random, batch, pos, size)
        host.append((flags, idx))
    host_tail, host_eps = np.random.randint(0, 1 << 30, size=3), sched.current
    # the planner
    np.random.seed(5)
    sched = LinearSchedule(0.8, 0.1, 30)
    from deeprl_amd.replay import draw_uniform_indices
    actor_steps, total, pos, size = 0, 0, 0, 0
    for flags, idx in host:
        explore, rand = plan_actor_epsilon_greedy(sched, k_len, 2, actor_steps, exploration_steps)
        assert explore.dtype == np.bool_ and rand.dtype == np.int64 and explore.shape == rand.shape == (k_len,)
        assert [int(r) if e else 1 for e, r in zip(explore, rand)] == flags
        actor_steps += k_len
        total += k_len
        for _ in range(k_len):
            if pos >= size:
                size += 1
            pos = (pos + 1) % cap
        if total > exploration_steps:
            assert np.array_equal(draw_uniform_indices(size, pos, batch, 1, 1), idx)
        else:
            assert idx is None
    assert np.array_equal(np.random.randint(0, 1 << 30, size=3), host_tail) and sched.current == host_eps


def test_planner_is_the_restated_draw_order():
    from deeprl_amd.support import LinearSchedule, plan_actor_epsilon_greedy
    a, want = K.AGENT, K.restated_agent_run()
    np.random.seed(a["np_seed"])
    sched = LinearSchedule(*a["eps"])
    explore, rand = plan_actor_epsilon_greedy(sched, a["k"], 2, 0, a["exploration_steps"])
    assert np.array_equal(explore, want["flags"][0]) and np.array_equal(rand, want["random_actions"][0])
    explore, rand = plan_actor_epsilon_greedy(sched, a["k"], 2, a["k"], a["exploration_steps"])     # exploration_steps crossed inside
    assert np.array_equal(explore, want["flags"][1]) and np.array_equal(rand, want["random_actions"][1])
    assert sched.current == a["eps"][0] + 2 * (a["eps"][1] - a["eps"][0]) / a["eps"][2]


# ------------------------------------------------------------------------------------------ C ABI mirrors, shapes
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_dqn_mlp_act_io", "dra_dqn_mlp_update_io"])
def test_ctypes_mirror_matches_the_header(tmp_path, which):
    from deeprl_amd import dqn_mlp
    from test_struct_layouts import _c_layout
    mirror = {"dra_dqn_mlp_act_io": dqn_mlp.ActIO, "dra_dqn_mlp_update_io": dqn_mlp.UpdateIO}[which]
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, which, names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_supported_shapes():
    from deeprl_amd import dqn_mlp
    ok, up = dqn_mlp.supported, dqn_mlp.update_supported
    for h in (8, 16, 32, 48, 64, 128):
        for gate in (0, 1, 2, 3):
            for k in (0, 1, 4, 8, 9):
                assert ok(4, 2, h, k, gate) == (h in (16, 32, 64) and gate in (1, 2) and 1 <= k <= K.MAX_K)
            for b in (0, 1, 10, 64, 65, 256, 257):
                assert up(4, 2, h, b, gate) == (h in (16, 32, 64) and gate in (1, 2) and 1 <= b <= K.MAX_B)
    assert not ok(5, 2, 64, 4, 1) and not ok(4, 3, 64, 4, 1) and not up(3, 2, 64, 10, 1) and not up(4, 1, 64, 10, 1)
    assert dqn_mlp.MAX_K == K.MAX_K and dqn_mlp.MAX_B == K.MAX_B


def test_kernels_refuse_unsupported_shapes_before_any_launch():
    """dra_dqn_mlp_act / dra_dqn_mlp_update validate on the host: null pointers and shapes outside the table are DRA_EINVAL
    without a device."""
    from deeprl_amd import dqn_mlp
    from deeprl_amd._lib import lib
    net, io, uo = dqn_mlp.Net(), dqn_mlp.ActIO(), dqn_mlp.UpdateIO()
    assert lib.dra_dqn_mlp_act.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    assert lib.dra_dqn_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22
    net.param = net.target = 4096
    net.state_dim, net.n_actions, net.hidden, net.gate = 4, 2, 64, 1
    for f, _ in dqn_mlp.ActIO._fields_[:18]:
        setattr(io, f, 4096)
    io.horizon, io.ring_cap, io.capacity, io.reward_coef = 200, 64, 100, 1.0
    for k, n in ((0, 1), (9, 1), (4, 2), (4, 0)):          # transitions outside 1..8, more or fewer than one environment
        io.t_len, io.n_env = k, n
        assert lib.dra_dqn_mlp_act.raw(ctypes.byref(net), ctypes.byref(io), None) == -22
    for f, _ in dqn_mlp.UpdateIO._fields_[:10]:
        setattr(uo, f, 4096)
    uo.discount = 0.99
    for b, cap in ((0, 100), (257, 100), (10, 1), (10, 1 << 31)):      # rows outside 1..256; a ring without a next frame; too long
        uo.batch, uo.capacity = b, cap
        assert lib.dra_dqn_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None) == -22


# ------------------------------------------------------------------------------------------ eligibility
class _Rec:
    def __init__(self):
        self.warnings = []

    def info(self, *a, **k):
        pass

    def warning(self, msg, *a, **k):
        self.warnings.append(str(msg))


def _stub(d, cls=None, network=None, target=None, optimizer=None, replay=None, target_order=None, task=None, **cfg):
    """What dqn_mlp.why_not reads of a DQNAgent, built without a device."""
    from deeprl_amd.optim import FlatParams, FusedOptimizer
    from deeprl_amd.replay import ReplayWrapper, UniformReplay
    net = lambda: d.VanillaNet(2, d.FCBody(4))
    agent = (cls or d.DQNAgent).__new__(cls or d.DQNAgent)
    c = d.Config()
    c.merge(dict(game=GAME, tag="dqn_feat_stub"))
    c.sgd_update_frequency, c.batch_size, c.n_step, c.history_length, c.double_q, c.async_actor = 4, 10, 1, 1, False, False
    c.fused_dqn_feature = True
    for k, v in cfg.items():
        setattr(c, k, v)
    agent.config, agent.logger = c, _Rec()
    agent.network, agent.target_network = network or net(), target or net()
    agent.optimizer = (optimizer or (lambda p: torch.optim.RMSprop(p, 0.001)))(agent.network.parameters())
    agent._fused = FusedOptimizer.adopt(agent.optimizer) if len(agent.optimizer.param_groups) == 1 else None
    tp = list(agent.target_network.parameters())
    agent._target_flat = FlatParams(tp if target_order is None else [tp[i] for i in target_order])
    agent.replay = replay or ReplayWrapper(UniformReplay, dict(memory_size=100, batch_size=c.batch_size, n_step=c.n_step,
                                                               discount=0.99, history_length=c.history_length), False)

    class Actor:
        _state, _task = None, task or d.Task(GAME, seed=3)
    agent.actor = Actor()
    return agent


def test_why_not_names_the_first_reason(monkeypatch):
    import deeprl_amd as d
    from deeprl_amd import device_env, dqn_mlp
    from deeprl_amd.replay import PrioritizedReplay, ReplayWrapper
    d.select_device(-1)
    why = dqn_mlp.why_not
    assert why(_stub(d)) == "the task is not one envs.CartPole environment, or there is no device"     # everything but a device
    # (with a device: the same stub is eligible)
    monkeypatch.setattr(device_env._RolloutVec, "_host_envs", staticmethod(lambda task, config: task.env.envs))
    assert why(_stub(d)) is None and why(_stub(d, double_q=True)) is None
    assert why(_stub(d, optimizer=lambda p: torch.optim.Adam(p, 1e-3))) is None
    assert why(_stub(d, fused_dqn_feature=False)) == "config.fused_dqn_feature is not on"
    assert why(_stub(d, fused_dqn_feature=1)) == "config.fused_dqn_feature is not on"
    assert "not a plain DQNAgent" in why(_stub(d, cls=d.CategoricalDQNAgent))
    per = ReplayWrapper(PrioritizedReplay, dict(memory_size=128, batch_size=10, n_step=1, discount=0.99, history_length=1), False)
    assert why(_stub(d, replay=per)) == "the replay is a PrioritizedReplay"
    assert why(_stub(d, n_step=3)) == "n_step is not 1"
    assert why(_stub(d, history_length=2)) == "history_length is not 1"
    assert why(_stub(d, noisy_linear=True)) == "noisy_linear is on"
    assert why(_stub(d, async_actor=True)) == "async_actor is on"
    duel = lambda: d.DuelingNet(2, d.FCBody(4))
    assert "the network is not VanillaNet" in why(_stub(d, network=duel(), target=duel()))
    assert "the network is not VanillaNet" in why(_stub(d, network=d.VanillaNet(2, d.FCBody(4, (64, 32)))))
    two_groups = lambda p: (lambda ps: torch.optim.RMSprop([dict(params=ps[:2]), dict(params=ps[2:])], 0.001))(list(p))
    assert "not one plain RMSprop or Adam" in why(_stub(d, optimizer=two_groups))
    a = _stub(d)
    a.optimizer.param_groups[0]['momentum'] = 0.9
    assert "not one plain RMSprop or Adam" in why(a)
    a = _stub(d, optimizer=lambda p: torch.optim.Adam(p, 1e-3))
    a.optimizer.param_groups[0]['amsgrad'] = True
    assert "not one plain RMSprop or Adam" in why(a)
    a = _stub(d)
    a.grad_hook = lambda g: None
    assert why(a) == "a grad_hook is installed"
    a = _stub(d)
    a.dp = type("DP", (), dict(active=True))()
    assert why(a) == "the agent is data parallel"
    assert "the target network is not" in why(_stub(d, target=d.VanillaNet(2, d.FCBody(4, (32, 32)))))
    assert "laid out differently" in why(_stub(d, target_order=[5, 4, 3, 2, 1, 0]))
    assert why(_stub(d, reward_normalizer=d.SignNormalizer())) == "the reward normaliser is not RescaleNormalizer(1.0)"
    assert why(_stub(d, reward_normalizer=d.RescaleNormalizer(0.5))) == "the reward normaliser is not RescaleNormalizer(1.0)"
    assert "dra_dqn_mlp_act is not built for" in why(_stub(d, sgd_update_frequency=9))
    assert why(_stub(d, batch_size=257)) == "dra_dqn_mlp_update is not built for minibatches of 257"
    assert why(_stub(d, batch_size=257, fused_dqn_update=False)) is None
    stepped = d.Task(GAME, seed=3)
    stepped.reset()
    stepped.step([0])
    assert why(_stub(d, task=stepped)) == "the environment has already been stepped on the host"
    a = _stub(d)
    a.actor._state = np.zeros((1, 4))
    assert why(a) == "the environment has already been stepped on the host"
    assert "not one envs.CartPole" in why(_stub(d, task=d.Task(GAME, num_envs=2, seed=3)))
    assert "not one envs.CartPole" in why(_stub(d, task=d.Task("synthetic-vector", seed=3)))


def test_adoption_logs_the_reason_once_and_keeps_the_host_path():
    import deeprl_amd as d
    from deeprl_amd import dqn_mlp
    d.select_device(-1)
    a = _stub(d)
    task = a.actor._task
    assert dqn_mlp.adopt(a) is None and a.actor._task is task and type(task) is d.Task
    assert len(a.logger.warnings) == 1 and "no device" in a.logger.warnings[0]
    b = _stub(d, fused_dqn_feature=False)
    assert dqn_mlp.adopt(b) is None and b.logger.warnings == []


# ------------------------------------------------------------------------------------------ what the case tables cover
@pytest.mark.parametrize("case", K.ACT_CASES, ids=K.act_id)
def test_act_cases_have_margin_and_cover_their_edges(case):
    hidden, gate, k_len, capacity, slot0, horizon, padded = case[:7]
    want, env, start = K.restated_act(case)
    assert want["margin"] >= K.MARGIN and want["fp32_same_actions"]
    assert 1 <= k_len <= K.MAX_K and 0 <= slot0 < capacity
    written = sorted({(slot0 + k) % capacity for k in range(k_len)})
    assert [i for i in range(capacity) if want["ring"]["masks"][i] >= 0] == written
    if horizon == 2:        # the wrap case: rows wrap, more transitions than slots, episodes end every second transition
        assert slot0 + k_len > capacity and k_len > capacity and len(want["events"]) == k_len // 2
        assert list(want["ring"]["masks"]) == [0, 1] * 3 or list(want["ring"]["masks"]) == [1, 0] * 3
    if k_len > 1:
        assert start["explore"].any() and (~start["explore"]).any()
    else:
        assert not start["explore"].any()


def test_act_cases_are_the_stated_ones():
    assert [c[:7] for c in K.ACT_CASES] == [(64, "relu", 4, 64, 0, 200, False), (16, "tanh", 1, 16, 3, 200, False),
                                            (32, "relu", 8, 6, 4, 2, False), (64, "tanh", 8, 32, 10, 200, True)]


def test_update_cases_are_the_stated_ones():
    cross = {(h, g, b, dq) for h in (16, 32, 64) for g in ("relu", "tanh") for b in (1, 10, 32, 64, 65, 256) for dq in (False, True)}
    assert {c[:4] for c in K.UPDATE_CASES if c[4] == "partial"} == cross
    assert any(c[4] == "full_mid" for c in K.UPDATE_CASES) and any(c[4] == "action0" for c in K.UPDATE_CASES)
    full = K.make_ring("full_mid")
    assert full["size"] == K.RINGS["full_mid"]["capacity"] and 0 < full["pos"] < full["size"] - 2
    assert (K.make_ring("action0")["ring"]["actions"][:40] == 0).all()
    part = K.make_ring("partial")
    assert part["pos"] == part["size"] == 260 and (part["ring"]["masks"][:260] == 0).sum() >= 20


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_cases_have_margin_and_cover_their_edges(case):
    hidden, gate, batch, double_q, kind = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    idx = u["idx"]
    assert idx.shape == (batch,) and all(R.valid_index(int(i), rg["pos"], rg["size"]) for i in idx)
    assert idx.min() >= 0 and idx.max() <= K.RINGS[kind]["capacity"] - 2
    if batch >= 4:
        last = max(i for i in range(rg["size"]) if R.valid_index(i, rg["pos"], rg["size"]))
        assert idx[0] == 0 and idx[1] == last and idx[2] == idx[3]
    if batch >= 32 and kind != "action0":
        assert (u["batch"]["mask"] == 0).any() and (u["batch"]["mask"] == 1).any()
        assert (u["batch"]["action"] == 0).any() and (u["batch"]["action"] == 1).any()
    if kind == "full_mid":
        assert (idx < rg["pos"]).any() and (idx >= rg["pos"]).any()
    if kind == "action0":
        assert (u["batch"]["action"] == 0).all() and not u["grads"]["fc_head.weight"][1].any() and u["grads"]["fc_head.bias"][1] == 0
    if gate == "relu":
        assert u["min_preact"] >= K.PREACT_MARGIN
    if double_q:
        assert u["argmax_margin"] >= K.MARGIN and u["fp32_same_argmax"]


def test_agent_case_has_margin_and_covers_its_edges():
    a, want = K.AGENT, K.restated_agent_run()
    want32 = K.restated_agent_run(dtype=torch.float32)
    assert want["margin"] >= K.MARGIN and np.array_equal(want["actions"], want32["actions"])
    assert want["min_preact"] >= K.PREACT_MARGIN
    assert want["explored"] >= 8 and want["greedy"] >= 8 and len(want["events"]) >= 4
    assert want["copies"] == [2, 5] and want["total"] == a["steps"] * a["k"] > a["capacity"]      # copies inside, the ring wraps
    assert a["k"] < a["exploration_steps"] < 2 * a["k"]                                        # crossed inside the second step
    assert [i is None for i in want["indices"]] == [True] + [False] * (a["steps"] - 1)
    assert (want["ring"]["masks"] == 0).any()
