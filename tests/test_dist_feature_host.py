"""categorical_dqn_feature / quantile_regression_dqn_feature on the device (csrc/dist_mlp.hip, deeprl_amd/dist_mlp.py), the part that
needs no GPU: the restatement the GPU tests lean on is pinned to the reference's own runs (tests/golden/dist_feature/), the two zoo
entries to the reference's Configs, the struct mirrors to the header, the shape tables and the why_not reasons to their
conditions, and the case tables to what they claim to cover -- above all the action-value margins every bit comparison rests on."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

import dist_feature_cases as K
import dist_feature_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dist_feature")
FIXTURE = os.path.join(GOLDEN, "steps.npz")
ZOO_REF = os.path.join(GOLDEN, "zoo_reference.json")
LEARNING = os.path.join(GOLDEN, "learning_reference.json")
TAGS = tuple(t[0] for t in K.FIXTURE_TAGS)
LENGTHS = (25000, 50000, 100000)
GAME = "classic-CartPole-v0"
ENTRY = {"c51": "categorical_dqn_feature", "qr": "quantile_regression_dqn_feature"}


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    """These tests seed np.random and switch the package's device; the tests after them see what they saw before."""
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


# ------------------------------------------------------------------------------------------ records
def test_fixture_holds_data_only_and_is_small():
    z = np.load(FIXTURE, allow_pickle=False)
    assert all(z[k].dtype.kind in "fiub" for k in z.files) and os.path.getsize(FIXTURE) < (1 << 20)
    for tag in TAGS:
        assert z[tag + "_flags"].shape == (K.FIXTURE["steps"], K.FIXTURE["k"])
        assert z[tag + "_flags"].any() and (~z[tag + "_flags"]).any()
    assert (z["c51_hz3_ring_masks"] == 0).any() and (z["qr_hz3_ring_masks"] == 0).any()
    assert bool(z["c51_double_q_cfg"][2]) and int(z["c51_copy_cfg"][3]) == 5 and int(z["qr_copy_cfg"][3]) == 5
    assert {t[1] for t in K.FIXTURE_TAGS} == set(K.HEADS)


@pytest.mark.parametrize("head", K.HEADS)
def test_zoo_entry_builds_the_reference_config(head):
    """zoo.config(entry) describes the Config the reference's own entry point builds (crosscheck_cases.describe_config), field for
    field; the switch rides along as a keyword and is off by default."""
    from deeprl_amd import zoo
    from golden import crosscheck_cases as C
    name = ENTRY[head]
    rec = json.load(open(ZOO_REF))[name]
    assert rec["agent"] == zoo.ZOO[name]["agent"] == ("CategoricalDQNAgent" if head == "c51" else "QuantileRegressionDQNAgent")
    want, have = rec["config"], C.describe_config(zoo.config(name, game=rec["game"]))
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert have[k] == want[k], k
    assert callable(getattr(zoo, name))
    on = zoo.config(name, game=GAME, tag="dist_feat_switch_on", fused_dist_feature=True)
    off = zoo.config(name, game=GAME, tag="dist_feat_switch_off")
    assert on.fused_dist_feature is True and getattr(off, "fused_dist_feature", False) is False


@pytest.mark.parametrize("head", K.HEADS)
def test_learning_reference_record(head):
    """The reference's own agent on the entry: 5 seeds, the last-100 mean at every length, the bar 2 x the random policy's mean and
    n_learn the smallest length at which the median reaches 2 x the bar (None: the reference never gets there)."""
    rec = json.load(open(LEARNING))[head]
    assert rec["bar"] == 2.0 * K.random_policy_mean() and abs(rec["bar"] - 44.2) < 0.1 and rec["entry"] == ENTRY[head]
    assert len(rec["runs"]) == 5 and sorted(rec["medians"]) == sorted(str(n) for n in LENGTHS)
    for n in LENGTHS:
        assert rec["medians"][str(n)] == float(np.median([r["ends"][str(n)]["last_mean"] for r in rec["runs"]]))
    reached = [n for n in LENGTHS if rec["medians"][str(n)] >= 2.0 * rec["bar"]]
    assert rec["n_learn"] == (reached[0] if reached else None)


# ------------------------------------------------------------------------------------------ the restatement and the reference
def _fixture_run(z, tag):
    _, head, task_seed, horizon, double_q, freq, hidden = next(t for t in K.FIXTURE_TAGS if t[0] == tag)
    f = K.FIXTURE
    init = {k: z["%s_init_%s" % (tag, k)] for k in R.keys(head)}
    target0 = {k: z["%s_target0_%s" % (tag, k)] for k in R.keys(head)}
    cfg = dict(k=f["k"], batch=f["batch"], capacity=f["capacity"], exploration_steps=f["exploration_steps"], target_freq=freq,
               discount=K.DISCOUNT, gradient_clip=K.GRADIENT_CLIP, lr=K.LR, double_q=double_q, gate="relu", spec=K.fixture_spec(head))
    env, _ = K.make_env(task_seed, horizon)
    rs = np.random.RandomState(f["np_seed"])
    out = R.agent_run(init, env, cfg, rs, K.epsilon_schedule(*f["eps"]), f["steps"], target0=target0)
    out["rng_tail"] = rs.randint(0, 1 << 30, size=3)
    return out, head


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_steps(tag):
    """R.agent_run on the fixture's configuration: actions, flags, random actions, the ring's four arrays, the sampled indices, pos
    and the np.random tail exactly; losses, the online parameters after every step and the target's at the end within rtol 2e-5 /
    atol 2e-6 (the reference computes in fp32)."""
    z = np.load(FIXTURE)
    got, head = _fixture_run(z, tag)
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
    for k in R.keys(head):
        want = z["%s_params_%s" % (tag, k)]
        np.testing.assert_allclose(np.stack([p[k] for p in got["params"]]), want, rtol=2e-5, atol=2e-6, err_msg=k)
        np.testing.assert_allclose(got["target"][k], z["%s_target_%s" % (tag, k)], rtol=2e-5, atol=2e-6, err_msg=k)
    if tag.endswith("copy"):
        assert got["copies"] == [4, 9]
    if tag.endswith("hz3"):
        assert len(got["events"]) >= 12 and all(r == 3.0 for _, _, r in got["events"])


def test_atoms_and_taus_are_the_hosts():
    """The restatement's support and tau are what the agents hand their networks: fp64 values narrowed to float32."""
    for n, (lo, hi) in K.SUPPORT.items():
        z = R.atoms(K.spec_of("c51", n))
        assert z.dtype == np.float32 and np.array_equal(z, torch.as_tensor(np.linspace(lo, hi, n)).float().numpy())
        step = (hi - lo) / (n - 1)
        mine = np.asarray([np.float32(hi) if i == n - 1 else np.float32(i * step + lo) for i in range(n)])      # the kernel's form
        assert np.array_equal(z, mine)
    t = R.taus(20)
    assert t.dtype == np.float32 and np.array_equal(t, torch.as_tensor((2 * np.arange(20) + 1) / 40.0).float().numpy())


# ------------------------------------------------------------------------------------------ C ABI mirrors, shapes
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_dist_mlp_net", "dra_dist_mlp_update_io"])
def test_ctypes_mirror_matches_the_header(tmp_path, which):
    from deeprl_amd import dist_mlp
    from test_struct_layouts import _c_layout
    mirror = {"dra_dist_mlp_net": dist_mlp.Net, "dra_dist_mlp_update_io": dist_mlp.UpdateIO}[which]
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, which, names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_supported_shapes():
    from deeprl_amd import dist_mlp
    ok, up = dist_mlp.supported, dist_mlp.update_supported
    for head in (0, 1, 2, 3):
        for n in (1, 2, 20, 50, 51, 52, 64):
            good = head in (1, 2) and 2 <= n <= K.MAX_ATOMS
            for h in (8, 16, 32, 48, 64, 128):
                for gate in (0, 1, 2, 3):
                    net = h in (16, 32, 64) and gate in (1, 2)
                    for k in (0, 1, 8, 9):
                        assert ok(4, 2, h, k, gate, head, n) == (good and net and 1 <= k <= K.MAX_K)
                    for b in (0, 1, 256, 257):
                        assert up(4, 2, h, b, gate, head, n) == (good and net and 1 <= b <= K.MAX_B)
    assert not ok(5, 2, 64, 4, 1, 1, 20) and not ok(4, 3, 64, 4, 1, 2, 20) and not up(3, 2, 64, 10, 1, 1, 20)
    assert (dist_mlp.MAX_K, dist_mlp.MAX_B, dist_mlp.MAX_ATOMS) == (K.MAX_K, K.MAX_B, K.MAX_ATOMS)


def test_kernels_refuse_bad_arguments_before_any_launch():
    """dra_dist_mlp_act / dra_dist_mlp_update validate on the host: null pointers, a negative offset, fewer than 2 atoms, a
    categorical support with v_max <= v_min and shapes outside the table are DRA_EINVAL without a device."""
    from deeprl_amd import dist_mlp
    from deeprl_amd._lib import lib
    net, io, uo = dist_mlp.Net(), dist_mlp.ActIO(), dist_mlp.UpdateIO()
    act = lambda: lib.dra_dist_mlp_act.raw(ctypes.byref(net), ctypes.byref(io), None)
    upd = lambda: lib.dra_dist_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None)
    assert act() == -22 and upd() == -22
    assert lib.dra_dist_mlp_act.raw(None, ctypes.byref(io), None) == -22 and lib.dra_dist_mlp_update.raw(ctypes.byref(net), None, None) == -22
    net.param = net.target = 4096
    net.state_dim, net.n_actions, net.hidden, net.gate, net.head, net.n_atoms, net.v_min, net.v_max = 4, 2, 64, 1, 1, 20, -10.0, 10.0
    for f, _ in dist_mlp.ActIO._fields_[:18]:
        setattr(io, f, 4096)
    io.horizon, io.ring_cap, io.capacity, io.reward_coef = 200, 64, 100, 1.0
    for f, _ in dist_mlp.UpdateIO._fields_[:11]:
        setattr(uo, f, 4096)
    uo.discount, uo.capacity, uo.batch, io.t_len, io.n_env = 0.99, 100, 10, 4, 1
    # every refusal below changes ONE thing of a pair of structs that differs from a valid one by nothing else
    for k, n in ((0, 1), (9, 1), (4, 2), (4, 0)):
        io.t_len, io.n_env = k, n
        assert act() == -22
    io.t_len, io.n_env = 4, 1
    for b, cap in ((0, 100), (257, 100), (10, 1), (10, 1 << 31)):
        uo.batch, uo.capacity = b, cap
        assert upd() == -22
    uo.batch, uo.capacity = 10, 100
    for field, bad, good in (("n_atoms", 1, 20), ("n_atoms", 52, 20), ("head", 0, 1), ("head", 3, 1), ("wq", -1, 0), ("b1", -4, 0),
                             ("v_max", -10.0, 10.0), ("v_max", -11.0, 10.0), ("v_max", float("nan"), 10.0), ("hidden", 128, 64)):
        setattr(net, field, bad)
        assert act() == -22 and upd() == -22, (field, bad)
        setattr(net, field, good)
    for f in ("out_q", "err", "slot0"):
        keep = getattr(io, f)
        setattr(io, f, None)
        assert act() == -22, f
        setattr(io, f, keep)
    for f in ("out_loss_vec", "out_q_next", "out_target", "idx", "grad"):
        keep = getattr(uo, f)
        setattr(uo, f, None)
        assert upd() == -22, f
        setattr(uo, f, keep)


# ------------------------------------------------------------------------------------------ eligibility
class _Rec:
    def __init__(self):
        self.warnings = []

    def info(self, *a, **k):
        pass

    def warning(self, msg, *a, **k):
        self.warnings.append(str(msg))


def _stub(d, head="c51", cls=None, network=None, target=None, replay=None, task=None, **cfg):
    """What dist_mlp.why_not reads of an agent, built without a device."""
    from deeprl_amd.optim import FlatParams, FusedOptimizer
    from deeprl_amd.replay import ReplayWrapper, UniformReplay
    net = (lambda: d.CategoricalNet(2, 20, d.FCBody(4))) if head == "c51" else (lambda: d.QuantileNet(2, 20, d.FCBody(4)))
    cls = cls or (d.CategoricalDQNAgent if head == "c51" else d.QuantileRegressionDQNAgent)
    agent = cls.__new__(cls)
    c = d.Config()
    c.merge(dict(game=GAME, tag="dist_feat_stub"))
    c.sgd_update_frequency, c.batch_size, c.n_step, c.history_length, c.double_q, c.async_actor = 4, 10, 1, 1, False, False
    c.categorical_n_atoms, c.categorical_v_min, c.categorical_v_max, c.num_quantiles = 20, -10, 10, 20
    c.fused_dist_feature = True
    for k, v in cfg.items():
        setattr(c, k, v)
    agent.config, agent.logger = c, _Rec()
    agent.network, agent.target_network = network or net(), target or net()
    agent.optimizer = torch.optim.RMSprop(agent.network.parameters(), 0.001)
    agent._fused = FusedOptimizer.adopt(agent.optimizer)
    agent._target_flat = FlatParams(list(agent.target_network.parameters()))
    agent.replay = replay or ReplayWrapper(UniformReplay, dict(memory_size=100, batch_size=c.batch_size), False)

    class Actor:
        _state, _task = None, task or d.Task(GAME, seed=3)
    agent.actor = Actor()
    return agent


def test_why_not_names_the_first_reason(monkeypatch):
    import deeprl_amd as d
    from deeprl_amd import device_env, dist_mlp
    from deeprl_amd.replay import PrioritizedReplay, ReplayWrapper
    d.select_device(-1)
    why = dist_mlp.why_not
    for head in K.HEADS:
        assert why(_stub(d, head)) == "the task is not one envs.CartPole environment, or there is no device"
    monkeypatch.setattr(device_env._RolloutVec, "_host_envs", staticmethod(lambda task, config: task.env.envs))
    for head in K.HEADS:
        assert why(_stub(d, head)) is None and why(_stub(d, head, double_q=True)) is None
        assert why(_stub(d, head, history_length=None)) is None        # (the two entries leave it unset)
        assert why(_stub(d, head, async_actor=True)) is None           # (the Config's default, a no-op for these agents)
        assert why(_stub(d, head, fused_dist_feature=False)) == "config.fused_dist_feature is not on"
        assert why(_stub(d, head, fused_dist_feature=1)) == "config.fused_dist_feature is not on"
        per = ReplayWrapper(PrioritizedReplay, dict(memory_size=128, batch_size=10, n_step=1, discount=0.99, history_length=1), False)
        assert why(_stub(d, head, replay=per)) == "the replay is a PrioritizedReplay"
        assert why(_stub(d, head, n_step=3)) == "n_step is not 1" and why(_stub(d, head, noisy_linear=True)) == "noisy_linear is on"
        assert "dra_dist_mlp_act is not built for" in why(_stub(d, head, sgd_update_frequency=9))
        assert why(_stub(d, head, batch_size=257, fused_dist_update=True)) == "dra_dist_mlp_update is not built for minibatches of 257"
        assert why(_stub(d, head, batch_size=257, fused_dist_update=False)) is None
        # unset, the update kernel is the quantile head's default and the module form the categorical head's
        assert (why(_stub(d, head, batch_size=257)) is None) == (head == "c51")
        shp = dist_mlp.shape(_stub(d, head).network)
        assert dist_mlp.Kind.fused_update(_stub(d, head).config, shp) == (head == "qr")
        assert dist_mlp.Kind.fused_update(_stub(d, head, fused_dist_update=True).config, shp) is True
        assert dist_mlp.Kind.fused_update(_stub(d, head, fused_dist_update=False).config, shp) is False
    assert "not a CategoricalDQNAgent or a QuantileRegressionDQNAgent" in why(_stub(d, cls=d.DQNAgent))
    vanilla = lambda: d.VanillaNet(2, d.FCBody(4))
    assert "the network is not CategoricalNet / QuantileNet" in why(_stub(d, network=vanilla(), target=vanilla()))
    assert "the network is not CategoricalNet / QuantileNet" in why(_stub(d, network=d.CategoricalNet(2, 20, d.FCBody(4, (64, 32)))))
    qn = lambda: d.QuantileNet(2, 20, d.FCBody(4))
    assert "the network's head is not the agent's" in why(_stub(d, "c51", network=qn(), target=qn()))
    assert why(_stub(d, "c51", categorical_n_atoms=21)) == "the network has 20 atoms per action, the configuration 21"
    assert why(_stub(d, "qr", num_quantiles=10)) == "the network has 20 atoms per action, the configuration 10"
    assert why(_stub(d, "c51", categorical_v_max=-10)) == "categorical_v_max is not above categorical_v_min"
    big = lambda: d.CategoricalNet(2, 52, d.FCBody(4))
    assert "dra_dist_mlp_act is not built for" in why(_stub(d, "c51", network=big(), target=big(), categorical_n_atoms=52))
    assert "the target network is not" in why(_stub(d, "qr", target=d.QuantileNet(2, 20, d.FCBody(4, (32, 32)))))
    # dqn_feature's own list is what it was
    from deeprl_amd import dqn_mlp
    assert "not a plain DQNAgent" in dqn_mlp.why_not(_stub(d, "c51", fused_dqn_feature=True))
    assert dqn_mlp.Kind.ASYNC_ACTOR is False and dist_mlp.Kind.ASYNC_ACTOR is True


def test_adoption_logs_the_reason_once_and_keeps_the_host_path():
    import deeprl_amd as d
    from deeprl_amd import dist_mlp
    d.select_device(-1)
    a = _stub(d, "qr")
    task = a.actor._task
    assert dist_mlp.adopt(a) is None and a.actor._task is task and type(task) is d.Task
    assert len(a.logger.warnings) == 1 and "no device" in a.logger.warnings[0]
    b = _stub(d, "c51", fused_dist_feature=False)
    assert dist_mlp.adopt(b) is None and b.logger.warnings == []


def test_step_overrides_only_what_differs():
    """dist_mlp.Step is dqn_mlp.Step but for the net struct, the update's io and the output buffers."""
    from deeprl_amd import dist_mlp, dqn_mlp
    own = {k for k in vars(dist_mlp.Step) if not k.startswith("__")}
    assert own == {"KIND", "make_outputs", "net_struct", "update"}
    for k in ("prepare", "step", "_learn", "check", "drain", "state_dict", "load_state_dict", "act_io", "__init__", "act",
              "module_update"):
        assert getattr(dist_mlp.Step, k) is getattr(dqn_mlp.Step, k), k


# ------------------------------------------------------------------------------------------ what the case tables cover
def test_act_cases_are_the_stated_ones():
    grid = {(h, hid, g, n, k) for h in K.HEADS for hid, g in ((16, "tanh"), (64, "relu")) for n in (2, 20, 51) for k in (1, 4, 8)}
    assert grid <= {c[:5] for c in K.ACT_CASES} and len(set(K.ACT_CASES)) == len(K.ACT_CASES)
    for head in K.HEADS:
        assert any(c[0] == head and c[6] == c[5] - 2 and c[4] > 2 for c in K.ACT_CASES)        # the ring wraps
        assert any(c[0] == head and c[7] == 3 and c[8] for c in K.ACT_CASES)                    # episodes end inside the launch


@pytest.mark.parametrize("case", K.ACT_CASES, ids=K.act_id)
def test_act_cases_have_margin_and_cover_their_edges(case):
    head, hidden, gate, n, k_len, capacity, slot0, horizon, padded, _ = case
    want, env, start = K.restated_act(case)
    assert want["margin"] >= K.MARGIN and want["fp32_same_actions"]
    assert 1 <= k_len <= K.MAX_K and 0 <= slot0 < capacity and 2 <= n <= K.MAX_ATOMS
    written = sorted({(slot0 + k) % capacity for k in range(k_len)})
    assert [i for i in range(capacity) if want["ring"]["masks"][i] >= 0] == written
    if horizon == 3:
        assert len(want["events"]) == k_len // 3 and (want["ring"]["masks"] == 0).any()
    if k_len > 1:
        assert start["explore"].any() and (~start["explore"]).any()
    else:
        assert not start["explore"].any()


def test_update_cases_are_the_stated_ones():
    r = K.ROW_BLOCK
    for head in K.HEADS:
        part = {(c[1], c[4], c[5]) for c in K.UPDATE_CASES if c[0] == head and c[6] == "partial"}
        dqs = (False, True) if head == "c51" else (False,)
        assert {(n, b, dq) for n in (2, 20, 50, 51) for b in (1, 10, r - 1, r, r + 1, 2 * r + 1) for dq in dqs} <= part
        assert any(c[0] == head and c[4] == 256 for c in K.UPDATE_CASES) and any(c[0] == head and c[6] == "action0" for c in K.UPDATE_CASES)
    assert {c[6] for c in K.UPDATE_CASES if c[0] == "c51"} >= {"clamps", "terminal", "on_atoms"}
    assert {(c[2], c[3]) for c in K.UPDATE_CASES} == {(h, g) for h in (16, 32, 64) for g in ("relu", "tanh")}
    assert all(K.update_padded(c) == (c[4] == r + 1) for c in K.UPDATE_CASES)
    assert (K.make_ring("action0")["ring"]["actions"][:40] == 0).all()
    part = K.make_ring("partial")
    assert part["pos"] == part["size"] == 260 and (part["ring"]["masks"][:260] == 0).sum() >= 20


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_cases_have_margin_and_cover_their_edges(case):
    head, n, hidden, gate, batch, double_q, kind, discount, _ = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    spec, idx = u["spec"], u["idx"]
    assert u["argmax_margin"] >= K.MARGIN and u["fp32_same_argmax"]
    if gate == "relu":
        assert u["min_preact"] >= K.PREACT_MARGIN
    assert idx.shape == (batch,) and all(R.valid_index(int(i), rg["pos"], rg["size"]) for i in idx)
    if batch >= 4:
        assert idx[0] == 0 and idx[2] == idx[3]
    if batch >= 32 and kind == "partial":
        assert (u["batch"]["mask"] == 0).any() and (u["batch"]["mask"] == 1).any()
        assert (u["batch"]["action"] == 0).any() and (u["batch"]["action"] == 1).any()
    w, b = R.keys(head)[4:]
    if kind == "action0":
        assert (u["batch"]["action"] == 0).all() and not u["grads"][w][n:].any() and not u["grads"][b][n:].any()
    if head == "c51":
        np.testing.assert_allclose(u["target"].sum(-1), 1.0, atol=1e-6)
        z = R.atoms(spec).astype(np.float64)
        delta = (spec["v_max"] - spec["v_min"]) / (n - 1)
        tz = u["batch"]["reward"][:, None] + discount * u["batch"]["mask"][:, None] * z[None]
    if kind == "clamps":
        assert (tz.min(1) > spec["v_max"]).any() and (tz.max(1) < spec["v_min"]).any()        # all mass on the last / the first atom
        assert ((tz.max(1) > spec["v_max"]) & (tz.min(1) < spec["v_max"])).any()               # part of the mass clamped
        assert (u["target"][:, -1] == 1.0).any() and (u["target"][:, 0] == 1.0).any()
    if kind == "terminal":
        assert (u["batch"]["mask"] == 0).all() and ((u["target"] > 0).sum(-1) <= 2).all()
    if kind == "on_atoms":
        assert discount == 1.0 and delta == 1.0 and (u["batch"]["mask"] == 1).all()
        assert np.array_equal(np.clip(tz, spec["v_min"], spec["v_max"]) % 1.0, np.zeros_like(tz))      # every Tz is an atom


@pytest.mark.parametrize("head", K.HEADS)
def test_agent_case_has_margin_and_covers_its_edges(head):
    a, want = K.AGENT, K.restated_agent_run(head)
    want32 = K.restated_agent_run(head, dtype=torch.float32)
    assert want["margin"] >= K.MARGIN and want["argmax_margin"] >= K.MARGIN and np.array_equal(want["actions"], want32["actions"])
    assert want["min_preact"] >= K.PREACT_MARGIN
    assert want["explored"] >= 8 and want["greedy"] >= 8 and len(want["events"]) >= 4
    assert want["copies"] == [2, 5] and want["total"] == a["steps"] * a["k"] > a["capacity"]      # copies inside, the ring wraps
    assert a["k"] < a["exploration_steps"] < 2 * a["k"]                                        # crossed inside the second step
    assert [i is None for i in want["indices"]] == [True] + [False] * (a["steps"] - 1)
    assert (want["ring"]["masks"] == 0).any()
    long = K.restated_agent_run(head, 10, 14)
    assert long["margin"] >= K.MARGIN and long["argmax_margin"] >= K.MARGIN
