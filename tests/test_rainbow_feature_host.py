"""rainbow_feature (the zoo entry, csrc/rainbow_mlp.hip, deeprl_amd/rainbow_mlp.py), the part that needs no GPU: the restatement
the GPU tests lean on is pinned to the reference's own RainbowNet (tests/golden/rainbow_feature/modules.npz), the zoo entry to the
reference's Config, the struct mirrors to the header, the shape tables to their conditions, the network walk to RainbowNet's
layout, and the case tables to what they claim to cover -- above all the action-value margins every bit comparison rests on."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

import rainbow_feature_cases as K
import rainbow_feature_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rainbow_feature")
MODULES = os.path.join(GOLDEN, "modules.npz")
ZOO_REF = os.path.join(GOLDEN, "zoo_reference.json")
MODULE_TAGS = ("h16_n3", "h64_n50", "h32_n51")
GAME = "classic-CartPole-v0"
ENTRY = "rainbow_feature"


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
    z = np.load(MODULES, allow_pickle=False)
    assert all(z[k].dtype.kind in "fiub" for k in z.files) and os.path.getsize(MODULES) < (1 << 20)
    for tag in MODULE_TAGS:
        hidden, n, _, rows = (int(v) for v in z[tag + "_cfg"])
        assert z[tag + "_prob"].shape == (rows, 2, n) and z[tag + "_obs"].shape == (rows, 4)
        for k in R.KEYS + R.NOISE_KEYS:
            assert "%s_sd_%s" % (tag, k) in z.files, k
        assert z[tag + "_sd_fc_advantage.weight_mu"].shape == (2 * n, hidden)
        assert np.unique(z[tag + "_sd_fc_value.weight_sigma"]).size > 1      # (the sigmas were spread: a constant one hides a transpose)


def test_zoo_entry_builds_the_reference_config():
    """zoo.config("rainbow_feature") describes the Config the reference's own entry point builds (crosscheck_cases.describe_config),
    field for field: noisy_linear on, n_step 3 and the PrioritizedReplay as keywords, Config.NOISY_LAYER_STD left alone."""
    import deeprl_amd as d
    from deeprl_amd import zoo
    from golden import crosscheck_cases as C
    std = d.Config.NOISY_LAYER_STD
    rec = json.load(open(ZOO_REF))[ENTRY]
    assert rec["agent"] == zoo.ZOO[ENTRY]["agent"] == "CategoricalDQNAgent"
    cfg = zoo.config(ENTRY, game=rec["game"])
    want, have = rec["config"], C.describe_config(cfg)
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert have[k] == want[k], k
    assert callable(getattr(zoo, ENTRY)) and d.Config.NOISY_LAYER_STD == std
    assert cfg.noisy_linear is True and cfg.n_step == 3 and cfg.double_q is True and cfg.replay_cls.__name__ == "PrioritizedReplay"
    assert "noisy_linear" not in zoo.ZOO[ENTRY]["kw"]      # (set behind merge(kwargs): a keyword cannot turn it off, as in the reference)
    assert zoo.config(ENTRY, game=GAME, tag="rainbow_feat_kw", noisy_linear=False).noisy_linear is True
    assert zoo.config(ENTRY, game=GAME, tag="rainbow_feat_n", n_step=1).replay_kwargs["n_step"] == 1


def test_learning_reference_record():
    """The reference's own agent on the entry: 5 seeds, the last-100 mean at 25 000, 50 000 and 100 000 steps, the bar 2 x the
    random policy's mean (dqn_feature's random_policy.json) and n_learn the smallest length at which the median reaches 2 x the
    bar."""
    rec = json.load(open(os.path.join(GOLDEN, "learning_reference.json")))
    rnd = json.load(open(os.path.join(ROOT, "tests", "golden", "dqn_feature", "random_policy.json")))
    lengths = (25000, 50000, 100000)
    assert rec["random_policy_mean"] == rnd["mean"] and rec["bar"] == 2.0 * rnd["mean"] and rec["entry"] == ENTRY
    assert rec["seeds"] == [1, 2, 3, 4, 5] and len(rec["runs"]) == 5 and sorted(rec["medians"]) == sorted(str(n) for n in lengths)
    for n in lengths:
        assert rec["medians"][str(n)] == float(np.median([r["ends"][str(n)]["last_mean"] for r in rec["runs"]]))
    reached = [n for n in lengths if rec["medians"][str(n)] >= 2.0 * rec["bar"]]
    assert reached and rec["n_learn"] == reached[0]


STEPS = os.path.join(GOLDEN, "steps.npz")
TAGS = tuple(t[0] for t in K.FIXTURE_TAGS)


@pytest.mark.parametrize("tag", TAGS)
def test_recorded_runs_show_what_they_are_there_for(tag):
    """steps.npz by the REFERENCE alone: at least one update pads an invalid draw through random.choice (the drawn leaves are not
    the ones it trained on), at least one draws a leaf twice, at least one sampled window holds a terminal, every greedy choice
    has an action-value margin of at least 1e-4; the ring wrapped, ten or more updates, a tag without double_q and a target copy
    inside a run."""
    z = np.load(STEPS, allow_pickle=False)
    assert all(z[k].dtype.kind in "fiub" for k in z.files) and os.path.getsize(STEPS) < (1 << 20)
    f = K.FIXTURE
    cap, n, b = f["capacity"], f["n_step"], f["batch"]
    drawn, leaves = z[tag + "_drawn"], z[tag + "_leaves"]
    assert drawn.shape == leaves.shape == (len(z[tag + "_update_steps"]), b) and 8 <= len(drawn) <= 12
    padded = sum(not np.array_equal(a, c) for a, c in zip(drawn, leaves))
    twice = sum(len(set(a.tolist())) < b for a in drawn)
    terminal = sum(int((z[tag + "_ring_masks"][u][d:d + n] == 0).any()) for u in range(len(leaves)) for d in leaves[u] - (cap - 1))
    q = z[tag + "_q"]
    assert padded >= 1 and twice >= 1 and terminal >= 1 and np.abs(q[..., 1] - q[..., 0]).min() >= K.MARGIN
    assert int(z[tag + "_total_steps"]) == f["steps"] * f["k"] > cap and int(z[tag + "_size"]) == cap      # (the ring wrapped)
    assert {bool(z[t + "_cfg"][2]) for t in TAGS} == {True, False} and any(len(z[t + "_copies"]) for t in TAGS)
    assert {int(z[t + "_cfg"][5]) for t in TAGS} >= {3, 50}


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_recorded_agent_steps(tag):
    """R.agent_run from the recorded run's initial parameters and the three generators' seeds against the reference's own
    CategoricalDQNAgent after every step: actions, the drawn leaves, the leaves behind the check and the padding, the pending
    set, the ring, the noise rows and the three generators' next draws equal; KL vectors, priorities, probabilities, the tree
    and its totals within 1e-5 relative (the reference computes them in fp32); parameters within rtol 2e-5 / atol 2e-6, the
    family's bar (the generator kept the first parameter seed that stays within half of it); every a_next margin >= 1e-4."""
    z = np.load(STEPS, allow_pickle=False)
    f = K.FIXTURE
    spec = next(t for t in K.FIXTURE_TAGS if t[0] == tag)
    torch_state = torch.get_rng_state()
    try:
        got = K.restated(z, tag)
        tails = np.random.randint(0, 1 << 30, size=3), torch.rand(3).numpy()
    finally:
        torch.set_rng_state(torch_state)
    assert np.array_equal(got["actions"], z[tag + "_actions"]) and min(got["margin"], got["argmax_margin"]) >= K.MARGIN
    steps = [int(s) for s in z[tag + "_update_steps"]]
    assert [i for i, u in enumerate(got["updates"]) if u is not None] == steps and got["copies"] == [int(s) for s in z[tag + "_copies"]]
    close = lambda a, w, rtol=1e-5, atol=1e-6: bool((np.abs(np.asarray(a) - w) <= atol + rtol * np.abs(w)).all())
    for u, step in enumerate(steps):
        g = got["updates"][step]
        assert np.array_equal(g["drawn"], z[tag + "_drawn"][u]) and np.array_equal(g["leaves"], z[tag + "_leaves"][u])
        assert g["beta"] == z[tag + "_beta"][u]
        assert close(g["prob"], z[tag + "_prob"][u]) and close([g["total"]], z[tag + "_total_before"][u:u + 1])
        assert close(g["kl"], z[tag + "_kl"][u]) and close(g["prio"], z[tag + "_prio"][u])
        flat = np.concatenate([g["noise"][k] for k in R.NOISE_KEYS]), np.concatenate([g["target_noise"][k] for k in R.NOISE_KEYS])
        assert np.array_equal(flat[0], z[tag + "_noise"][u]) and np.array_equal(flat[1], z[tag + "_target_noise"][u])
        for k in ("frames", "actions", "rewards", "masks"):
            filled = min(f["capacity"], (step + 1) * f["k"])      # (the slots behind it: NaN here, 0 in the record)
            assert np.array_equal(got["rings"][step][k][:filled], z["%s_ring_%s" % (tag, k)][u][:filled]), k
        for k in R.KEYS:
            want = z["%s_params_%s" % (tag, k)][u]
            assert close(got["params"][step][k], want, 2e-5, 2e-6), (step, k)
    rows = np.stack([[np.concatenate([r[k] for k in R.NOISE_KEYS]) for r in step_rows] for step_rows in got["rows"]])
    assert np.array_equal(rows, z[tag + "_rows"])
    assert close(got["tree"], z[tag + "_tree"]) and got["pending"] == z[tag + "_pending"].tolist()
    assert close([got["max_priority"]], z[tag + "_max_priority"].reshape(1))
    assert (got["pos"], got["size"], got["total"]) == (int(z[tag + "_pos"]), int(z[tag + "_size"]), int(z[tag + "_total_steps"]))
    assert np.array_equal(tails[0], z[tag + "_np_tail"]) and np.array_equal(tails[1], z[tag + "_torch_tail"])
    assert np.array_equal(got["random_tail"], z[tag + "_random_tail"])


@pytest.mark.parametrize("tag", MODULE_TAGS)
def test_restatement_reproduces_the_reference_network(tag):
    """R.logits on the reference's own parameters and RAW noise vectors: its probabilities and their logarithms within fp32
    rounding (the reference computes in fp32), and the effective weights equal to mu + sigma * the reference's stored products to
    the bit in fp32."""
    z = np.load(MODULES, allow_pickle=False)
    sd = {k[len(tag) + 4:]: z[k] for k in z.files if k.startswith(tag + "_sd_")}
    n = int(z[tag + "_cfg"][1])
    p, nz = R.to_t({k: sd[k] for k in R.KEYS}), R.to_t({k: sd[k] for k in R.NOISE_KEYS})
    out = R.logits(p, nz, z[tag + "_obs"], n)
    assert np.abs(torch.softmax(out, -1).numpy() - z[tag + "_prob"]).max() <= 2e-7
    assert np.abs(torch.log_softmax(out, -1).numpy() - z[tag + "_log_prob"]).max() <= 2e-6
    p32, nz32 = R.to_t(sd, torch.float32), R.to_t(sd, torch.float32)
    for layer in R.LAYERS:
        w, b = R.effective(p32, nz32, layer)
        assert np.array_equal(w.numpy(), sd[layer + ".weight_mu"] + sd[layer + ".weight_sigma"] * sd[layer + ".weight_epsilon"])
        assert np.array_equal(b.numpy(), sd[layer + ".bias_mu"] + sd[layer + ".bias_sigma"] * sd[layer + ".bias_epsilon"])


def test_minibatch_is_the_reference_replays_fold():
    """R.minibatch against what the reference's own UniformReplay.construct_transition returned on the same ring
    (tests/golden/rainbow_feature/replay_fold.npz) at EVERY valid index, n_step 1 and 3: which indices are valid, where the next
    state lies, the folded reward narrowed to float32 and the masks' product."""
    z = np.load(os.path.join(GOLDEN, "replay_fold.npz"), allow_pickle=False)
    rg = K.make_ring("partial")
    for n_step in (1, 3):
        rec = z["n%d" % n_step]
        idx = [i for i in range(rg["size"]) if K.valid_index(i, rg["pos"], rg["size"], n_step)]
        assert idx == [int(i) for i in rec[:, 0]] and np.array_equal(rec[:, 1], rec[:, 0] + n_step)
        mb = R.minibatch(rg["ring"], idx, n_step, K.DISCOUNT)
        assert np.array_equal(mb["reward"], rec[:, 2].astype(np.float32)) and np.array_equal(mb["mask"], rec[:, 3].astype(np.float32))
        assert (rec[:, 3] == 0).any() and (rec[:, 3] == 1).any()


# ------------------------------------------------------------------------------------------ C ABI mirrors, shapes
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_rainbow_mlp_layer", "dra_rainbow_mlp_net", "dra_rainbow_mlp_update_io"])
def test_ctypes_mirror_matches_the_header(tmp_path, which):
    from deeprl_amd import rainbow_mlp
    from test_struct_layouts import _c_layout
    mirror = {"dra_rainbow_mlp_layer": rainbow_mlp.Layer, "dra_rainbow_mlp_net": rainbow_mlp.Net,
              "dra_rainbow_mlp_update_io": rainbow_mlp.UpdateIO}[which]
    names = [f[0] for f in mirror._fields_]
    got = _c_layout(tmp_path, which, names)
    assert got[0] == ctypes.sizeof(mirror)
    assert got[1:] == [getattr(mirror, n).offset for n in names]


def test_supported_shapes():
    """The entry's own shape -- hidden 64, 50 atoms, batch 32, n_step 3 -- is supported; the update's largest batch is MAX_B = 64
    (the target network's probabilities of every row stay in LDS)."""
    from deeprl_amd import rainbow_mlp
    ok, up = rainbow_mlp.supported, rainbow_mlp.update_supported
    assert ok(4, 2, 64, 4, 1, 50) and up(4, 2, 64, 32, 1, 50, 3)
    for n in (1, 2, 50, 51, 52, 64):
        good = 2 <= n <= K.MAX_ATOMS
        for h in (8, 16, 32, 48, 64, 128):
            for gate in (0, 1, 2, 3):
                net = h in (16, 32, 64) and gate in (1, 2)
                for k in (0, 1, 8, 9):
                    assert ok(4, 2, h, k, gate, n) == (good and net and 1 <= k <= K.MAX_K)
                for b in (0, 1, K.MAX_B, K.MAX_B + 1, 256):
                    for n_step in (0, 1, 3, K.MAX_N_STEP, K.MAX_N_STEP + 1):
                        assert up(4, 2, h, b, gate, n, n_step) == (good and net and 1 <= b <= K.MAX_B and 1 <= n_step <= K.MAX_N_STEP)
    assert not ok(5, 2, 64, 4, 1, 50) and not ok(4, 3, 64, 4, 1, 50) and not up(3, 2, 64, 10, 1, 50, 3)
    assert (rainbow_mlp.MAX_K, rainbow_mlp.MAX_B, rainbow_mlp.MAX_ATOMS, rainbow_mlp.MAX_N_STEP) == (K.MAX_K, K.MAX_B, K.MAX_ATOMS,
                                                                                                     K.MAX_N_STEP)


def test_kernels_refuse_bad_arguments_before_any_launch():
    """dra_rainbow_mlp_act / dra_rainbow_mlp_update validate on the host: null pointers, a negative offset, fewer than 2 atoms, a
    support with v_max <= v_min, a ring shorter than the n-step window and shapes outside the table are DRA_EINVAL without a device."""
    from deeprl_amd import rainbow_mlp
    from deeprl_amd._lib import lib
    net, io, uo = rainbow_mlp.Net(), rainbow_mlp.ActIO(), rainbow_mlp.UpdateIO()
    act = lambda: lib.dra_rainbow_mlp_act.raw(ctypes.byref(net), ctypes.byref(io), None)
    upd = lambda: lib.dra_rainbow_mlp_update.raw(ctypes.byref(net), ctypes.byref(uo), None)
    assert act() == -22 and upd() == -22
    assert lib.dra_rainbow_mlp_act.raw(None, ctypes.byref(io), None) == -22
    assert lib.dra_rainbow_mlp_update.raw(ctypes.byref(net), None, None) == -22
    net.param = net.target = net.noise = net.target_noise = 4096
    net.state_dim, net.n_actions, net.hidden, net.gate, net.n_atoms, net.v_min, net.v_max = 4, 2, 64, 1, 50, -100.0, 100.0
    for f, _ in rainbow_mlp.ActIO._fields_[:18]:
        setattr(io, f, 4096)
    io.horizon, io.ring_cap, io.capacity, io.reward_coef = 200, 64, 100, 1.0
    for f, _ in rainbow_mlp.UpdateIO._fields_[:15]:
        setattr(uo, f, 4096)
    uo.discount, uo.step_discount, uo.capacity, uo.batch, uo.n_step, io.t_len, io.n_env = 0.97, 0.99, 100, 32, 3, 4, 1
    # every refusal below changes ONE thing of a pair of structs that differs from a valid one by nothing else
    for k, n in ((0, 1), (9, 1), (4, 2), (4, 0)):
        io.t_len, io.n_env = k, n
        assert act() == -22
    io.t_len, io.n_env = 4, 1
    for b, cap, n_step in ((0, 100, 3), (K.MAX_B + 1, 100, 3), (32, 3, 3), (32, 1 << 31, 3), (32, 100, 0), (32, 100, K.MAX_N_STEP + 1)):
        uo.batch, uo.capacity, uo.n_step = b, cap, n_step
        assert upd() == -22
    uo.batch, uo.capacity, uo.n_step = 32, 100, 3
    for field, bad, good in (("n_atoms", 1, 50), ("n_atoms", 52, 50), ("noise_stride", -1, 0), ("v_max", -100.0, 100.0),
                             ("v_max", -101.0, 100.0), ("v_max", float("nan"), 100.0), ("hidden", 128, 64), ("gate", 3, 1)):
        setattr(net, field, bad)
        assert act() == -22 and upd() == -22, (field, bad)
        setattr(net, field, good)
    for layer in rainbow_mlp.LAYERS:
        for field in ("w_mu", "b_sigma", "e_in", "e_b"):
            setattr(getattr(net, layer), field, -1)
            assert act() == -22 and upd() == -22, (layer, field)
            setattr(getattr(net, layer), field, 0)
    net.noise = None
    assert act() == -22 and upd() == -22
    net.noise, net.target_noise = 4096, None
    assert upd() == -22
    net.target_noise = 4096
    for f in ("out_q", "err", "slot0"):
        keep = getattr(io, f)
        setattr(io, f, None)
        assert act() == -22, f
        setattr(io, f, keep)
    for f in ("out_loss_vec", "out_prio", "out_weights", "out_q_next", "out_target", "idx", "prob", "beta", "grad"):
        keep = getattr(uo, f)
        setattr(uo, f, None)
        assert upd() == -22, f
        setattr(uo, f, keep)


# ------------------------------------------------------------------------------------------ the network walk
def test_shape_and_fill_layers_follow_the_network():
    """rainbow_mlp.shape names the entry's network and refuses its neighbours; fill_layers writes the sixteen parameter offsets and
    the twelve noise offsets where the flat buffer and the noise block have them."""
    import deeprl_amd as d
    from deeprl_amd import rainbow_mlp
    d.select_device(-1)
    mk = lambda n=50, hidden=(64, 64), gate=torch.relu, noisy=True: d.RainbowNet(
        2, n, d.FCBody(4, hidden, gate=gate, noisy_linear=noisy), noisy_linear=noisy)
    net = mk()
    assert rainbow_mlp.shape(net) == (4, 2, 64, 1, 50) and rainbow_mlp.shape(mk(51, (16, 16), torch.tanh)) == (4, 2, 16, 2, 51)
    assert rainbow_mlp.shape(mk(hidden=(64, 32))) is None and rainbow_mlp.shape(mk(hidden=(64,))) is None
    assert rainbow_mlp.shape(mk(noisy=False)) is None and rainbow_mlp.shape(mk(gate=torch.sigmoid)) is None
    assert rainbow_mlp.shape(d.CategoricalNet(2, 50, d.FCBody(4))) is None
    assert rainbow_mlp.shape(d.RainbowNet(2, 50, d.FCBody(4), noisy_linear=True)) is None      # (a plain body under noisy heads)
    # the flat buffer of the test: the parameters in named_parameters() order; the noise row: the draw order at multiples of 4
    offs, off = {}, 0
    for k, p in net.named_parameters():
        offs[id(p)] = off
        off += p.numel()
    slices, off = {}, 0
    for lname, m in net.noisy_layers():
        for b in rainbow_mlp.NOISE:
            slices[(lname, b)] = (off, getattr(m, b).numel())
            off += (getattr(m, b).numel() + 3) // 4 * 4
    assert [l for l, _ in net.noisy_layers()] == list(R.DRAW_ORDER)
    want, _ = K.noise_layout(64, 50, False)
    assert {"%s.%s" % k: v[0] for k, v in slices.items()} == want
    s = rainbow_mlp.fill_layers(rainbow_mlp.Net(), net, lambda p: offs[id(p)], slices)
    named = dict(net.named_parameters())
    for field, layer in zip(rainbow_mlp.LAYERS, R.LAYERS):
        got = getattr(s, field)
        assert [got.w_mu, got.w_sigma, got.b_mu, got.b_sigma] == [offs[id(named["%s.%s" % (layer, p)])] for p in R.PARAMS]
        assert [got.e_in, got.e_out, got.e_b] == [want["%s.%s" % (layer, b)] for b in R.NOISE]
    assert len({(getattr(s, f).w_mu) for f in rainbow_mlp.LAYERS}) == 4


# ------------------------------------------------------------------------------------------ the cases
def test_act_cases_are_the_stated_ones():
    grid = {(hid, g, n, k) for hid in (16, 64) for g in ("relu", "tanh") for n in (2, 50, 51) for k in (1, 4, 8)}
    assert grid <= {c[:4] for c in K.ACT_CASES} and len(set(K.ACT_CASES)) == len(K.ACT_CASES)
    assert any(c[5] + c[3] > c[4] for c in K.ACT_CASES)                  # a slot range that wraps the ring
    assert any(c[6] < c[3] and c[7] for c in K.ACT_CASES)                # episodes end inside the launch; padded buffers


@pytest.mark.parametrize("case", K.ACT_CASES, ids=K.act_id)
def test_act_cases_have_margin_and_cover_their_edges(case):
    hidden, gate, n, k_len, capacity, slot0, horizon, padded, _ = case
    want, env, start = K.restated_act(case)
    assert want["margin"] >= K.MARGIN and want["fp32_same_actions"]
    assert not start["explore"].any()                                    # epsilon is 0 under noisy layers: every transition is greedy
    rows = start["noise_rows"]
    assert len(rows) == k_len and all(not np.array_equal(rows[0][k], r[k]) for r in rows[1:] for k in R.NOISE_KEYS)
    if horizon < k_len:
        assert want["events"] and (want["ring"]["masks"] == 0).any()
    if slot0 + k_len > capacity:
        assert want["ring"]["actions"][0] >= 0 and want["ring"]["actions"][capacity - 1] >= 0
    assert (want["ring"]["actions"] >= 0).sum() == k_len


def test_flip_case_alternates_on_the_noise_alone():
    """The noise-row case: one parameter set, the action alternating 0, 1, 0, 1, ... through the noise rows; under row 0 alone or
    row K - 1 alone the restatement chooses otherwise somewhere."""
    want, env, start = K.flip_case()
    k_len = K.FLIP["k"]
    assert list(want["action"]) == [k % 2 for k in range(k_len)] and want["margin"] >= 100 * K.MARGIN
    for fixed in (0, k_len - 1):
        e, raw = K.make_env(K.ENV_SEED, 200)
        got = R.act(start["params"], [start["noise_rows"][fixed]] * k_len, e, raw, k_len, start["explore"], start["random_action"],
                    R.new_ring(64), 0, start["spec"], gate=K.FLIP["gate"])
        assert not np.array_equal(got["action"], want["action"])


def test_update_cases_are_the_stated_ones():
    part = [c for c in K.UPDATE_CASES if c[5] == "partial"]
    assert {(c[0], c[3]) for c in part} >= {(n, b) for n in (2, 50, 51) for b in (1, 15, 16, 17, 32, 33, K.MAX_B)}
    for n in (2, 50, 51):
        mine = [c for c in part if c[0] == n]
        assert {c[4] for c in mine} == {False, True} and {1, 3} <= {c[6] for c in mine} and {0.4, 1.0} <= {c[7] for c in mine}
    assert (50, 64, "relu", 32, True, "partial", 3, 0.4, K.DISCOUNT, None) in K.UPDATE_CASES      # the entry's own update
    assert {c[5] for c in K.UPDATE_CASES} == {"partial", "action0", "clamps", "terminal", "on_atoms"}
    assert {(c[1], c[2]) for c in K.UPDATE_CASES} >= {(h, g) for h in (16, 32, 64) for g in ("relu", "tanh")}
    assert any(K.update_padded(c) for c in K.UPDATE_CASES) and any(c[6] == K.MAX_N_STEP for c in K.UPDATE_CASES)


@pytest.mark.parametrize("case", K.UPDATE_CASES, ids=K.update_id)
def test_update_cases_have_margin_and_cover_their_edges(case):
    n, hidden, gate, batch, double_q, kind, n_step, beta, discount, _ = case
    u, rg = K.restated_update(case), K.make_ring(kind)
    spec, idx, mb = u["spec"], u["idx"], u["batch"]
    assert u["argmax_margin"] >= K.MARGIN and u["fp32_same_argmax"]
    assert gate != "relu" or u["min_preact"] >= K.PREACT_MARGIN
    assert len(idx) == batch and all(K.valid_index(int(i), rg["pos"], rg["size"], n_step) for i in idx)
    assert any(not np.array_equal(u["noise"][k], u["target_noise"][k]) for k in R.NOISE_KEYS)
    assert any(not np.array_equal(u["params"][k], u["target_params"][k]) for k in R.KEYS)
    masks, rewards = rg["ring"]["masks"], rg["ring"]["rewards"]
    if kind == "partial":
        assert np.unique(rewards[:rg["size"]]).size > 3                  # non-unit rewards
        if batch >= 4 and n_step == 3:
            # a terminal at every position of a row's window: the folded reward and the mask product stop there
            assert masks[idx[0]] == 0 and masks[idx[1] + 1] == 0 and masks[idx[2] + 2] == 0
            assert masks[idx[1]] == 1 and masks[idx[2]] == 1 and masks[idx[2] + 1] == 1
            assert (mb["mask"] == 0).any() and (mb["mask"] == 1).any()
        if batch >= 6:
            assert idx[3] == 0 and idx[5] == idx[2]
    if batch >= 2:
        assert u["prob"][0] <= 1e-6 and u["prob"][1] >= 0.9 and u["weights"][0] == 1.0 and u["weights"].min() < 0.1
    z = R.atoms(spec)
    tz = mb["reward"][:, None].astype(np.float64) + (discount ** n_step) * mb["mask"][:, None] * z[None].astype(np.float64)
    if kind == "clamps":
        assert (tz > spec["v_max"]).any() and (tz < spec["v_min"]).any()
    if kind == "terminal":
        assert (mb["mask"] == 0).all()
    if kind == "on_atoms":
        delta = (spec["v_max"] - spec["v_min"]) / (n - 1)
        b = (np.clip(tz, spec["v_min"], spec["v_max"]) - spec["v_min"]) / delta
        assert np.array_equal(b, np.round(b))
    if kind == "action0":
        assert not mb["action"].any()
        assert u["grads"]["fc_advantage.weight_mu"][n:].any()      # (the other action's rows still move: the dueling mean)
    assert np.all(np.isfinite(u["loss_vec"])) and np.isclose(u["target"].sum(-1), 1.0, atol=1e-6).all()


# ------------------------------------------------------------------------------------------ eligibility
class _Rec:
    def __init__(self):
        self.warnings = []

    def info(self, *a, **k):
        pass

    def warning(self, msg, *a, **k):
        self.warnings.append(str(msg))


def _stub(d, cls=None, replay=None, replay_kw=None, **cfg):
    """What rainbow_mlp.why_not reads of an agent, built without a device."""
    from deeprl_amd.optim import FlatParams, FusedOptimizer
    from deeprl_amd.replay import PrioritizedReplay, ReplayWrapper
    cls = cls or d.CategoricalDQNAgent
    agent = cls.__new__(cls)
    c = d.Config()
    c.merge(dict(game=GAME, tag="rainbow_feat_stub"))
    c.sgd_update_frequency, c.batch_size, c.n_step, c.history_length, c.double_q, c.async_actor = 4, 32, 3, 1, True, True
    c.categorical_n_atoms, c.categorical_v_min, c.categorical_v_max, c.noisy_linear, c.discount = 50, -100, 100, True, 0.99
    c.fused_rainbow_feature = True
    for k, v in cfg.items():
        setattr(c, k, v)
    net = lambda: d.RainbowNet(2, 50, d.FCBody(4, noisy_linear=c.noisy_linear), noisy_linear=c.noisy_linear)
    agent.config, agent.logger = c, _Rec()
    agent.network, agent.target_network = net(), net()
    agent.optimizer = torch.optim.RMSprop(agent.network.parameters(), 0.001)
    agent._fused = FusedOptimizer.adopt(agent.optimizer)
    agent._target_flat = FlatParams(list(agent.target_network.parameters()))
    kw = dict(dict(memory_size=100, batch_size=c.batch_size, n_step=3, discount=0.99, history_length=1), **(replay_kw or {}))
    agent.replay = replay or ReplayWrapper(PrioritizedReplay, kw, False)

    class Actor:
        _state, _task = None, d.Task(GAME, seed=3)
    agent.actor = Actor()
    return agent


def test_why_not_names_the_first_reason():
    """rainbow_mlp.why_not walks dqn_mlp.why_not's list with a PrioritizedReplay, an n-step window and noisy layers REQUIRED; the
    two sibling kinds keep refusing all three with the strings their own suites pin."""
    import deeprl_amd as d
    from deeprl_amd import dist_mlp, dqn_mlp, rainbow_mlp
    from deeprl_amd.replay import ReplayWrapper, UniformReplay
    d.select_device(-1)
    why = rainbow_mlp.why_not
    assert why(_stub(d, fused_rainbow_feature=False)) == "config.fused_rainbow_feature is not on"
    assert why(_stub(d, cls=d.DQNAgent)) == "the agent is a DQNAgent, not a CategoricalDQNAgent"
    uni = ReplayWrapper(UniformReplay, dict(memory_size=100, batch_size=32, n_step=3, discount=0.99), False)
    assert why(_stub(d, replay=uni)) == "the replay is not a PrioritizedReplay"
    forced = _stub(d)
    forced._inner_replay().ordered_updates = True
    assert why(forced) == "the replay has ordered_updates forced"
    long = "n_step is not between 1 and 8, or the replay's is not the configuration's"
    assert why(_stub(d, n_step=9, replay_kw=dict(n_step=9))) == long and why(_stub(d, n_step=1)) == long
    assert why(_stub(d, replay_kw=dict(history_length=2))) == "history_length is not 1"
    assert why(_stub(d, noisy_linear=False)) == "noisy_linear is off"
    # (without a device the noisy layers cannot be on csrc/noisy.hip: the walk ends there; the GPU suite walks on)
    assert why(_stub(d)) == "the noisy layers are not on csrc/noisy.hip (config.fused_noisy)"
    # the siblings on the same agent: today's reasons, word for word
    for kind, switch in ((dqn_mlp.Kind, "fused_dqn_feature"), (dist_mlp.Kind, "fused_dist_feature")):
        agent = _stub(d, cls=d.DQNAgent if kind is dqn_mlp.Kind else None, **{switch: True})
        assert dqn_mlp.why_not(agent, kind=kind) == "the replay is a PrioritizedReplay"
        agent.replay = ReplayWrapper(UniformReplay, dict(memory_size=100, batch_size=32, n_step=3, discount=0.99), False)
        assert dqn_mlp.why_not(agent, kind=kind) == "n_step is not 1"
        agent.replay = ReplayWrapper(UniformReplay, dict(memory_size=100, batch_size=32), False)
        agent.config.n_step = 1
        assert dqn_mlp.why_not(agent, kind=kind) == "noisy_linear is on"
    assert (dqn_mlp.Kind.PRIORITIZED, dqn_mlp.Kind.MAX_N_STEP, dqn_mlp.Kind.NOISY) == (False, 1, False)
    assert (dist_mlp.Kind.PRIORITIZED, dist_mlp.Kind.MAX_N_STEP, dist_mlp.Kind.NOISY) == (False, 1, False)


def test_step_overrides_only_what_differs():
    """rainbow_mlp.Step is dqn_mlp.Step but for the staged block's tail, the draws, the net struct, the update and the commit."""
    from deeprl_amd import dqn_mlp, rainbow_mlp
    own = {k for k in vars(rainbow_mlp.Step) if not k.startswith("__") or k == "__init__"}
    assert own == {"KIND", "__init__", "make_outputs", "net_struct", "update", "module_update", "prepare", "after_learn", "staged_tail"}
    assert rainbow_mlp.Step.step is dqn_mlp.Step.step and rainbow_mlp.Step.act is dqn_mlp.Step.act
