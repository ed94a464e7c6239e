"""Host-side pieces of the hot path against the reference's own code, through what it returned on the same inputs
(tests/golden/crosscheck.json, written by tests/golden/make_golden_crosscheck.py from the reference; inputs:
tests/golden/crosscheck_cases.py): schedules, epsilon_greedy's RNG order (a4), random_sample's minibatch
permutation (a22), Storage feed / placeholder / extract (a7), Config defaults and merge, generate_tag."""
import json

import numpy as np
import pytest
import torch

from golden import crosscheck_cases as C


@pytest.fixture(scope="module")
def ref():
    """What the reference returned on the cases of crosscheck_cases.py."""
    with open(C.CROSSCHECK_JSON) as f:
        return json.load(f)


def test_schedules(ref):
    import deeprl_amd as d
    want = ref["host_utils"]["schedules"]
    assert len(want) == len(C.SCHEDULE_ARGS)
    for args, values in zip(C.SCHEDULE_ARGS, want):
        a = d.LinearSchedule(*args)
        assert [a(steps) for steps in C.SCHEDULE_STEPS] == values, args
    assert d.ConstantSchedule(0.3)(5) == ref["host_utils"]["constant_schedule"]


def test_epsilon_greedy_consumes_the_same_random_numbers(ref):
    import deeprl_amd as d
    want = ref["host_utils"]["epsilon_greedy"]
    cases = list(C.epsilon_greedy_cases())
    assert len(cases) == len(want)
    for (shape, eps, q), w in zip(cases, want):
        assert list(shape) == w["shape"] and eps == w["eps"]
        np.random.seed(11)
        a = d.epsilon_greedy(eps, q)
        tail_a = np.random.randint(1 << 30)
        assert np.array_equal(np.asarray(a), np.asarray(w["action"])) and tail_a == w["tail"]


def test_random_sample_batches(ref):
    import deeprl_amd as d
    want = ref["host_utils"]["random_sample"]
    assert [(w["n"], w["b"]) for w in want] == [tuple(c) for c in C.RANDOM_SAMPLE_CASES]
    for (n, b), w in zip(C.RANDOM_SAMPLE_CASES, want):
        np.random.seed(n)
        x = [np.asarray(v).copy() for v in d.random_sample(np.arange(n), b)]
        y = [np.asarray(v) for v in w["batches"]]
        assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))


def test_storage_feed_placeholder_extract(ref):
    import deeprl_amd as d
    t_len, n = 5, 3
    want = ref["host_utils"]["storage"]
    a = d.Storage(t_len)
    for row in C.storage_rows(t_len, n):
        a.feed(row)
    a.placeholder()
    assert a.advantage == want["advantage"] == [None] * t_len
    ea = a.extract(C.STORAGE_KEYS)
    assert list(ea._fields) == want["fields"]
    for x, y in zip(ea, want["values"]):
        assert torch.equal(x, torch.tensor(y, dtype=x.dtype)) and x.shape == (t_len * n, 1)
    assert want["bad_key_raises"] == "RuntimeError"
    with pytest.raises(RuntimeError):
        a.feed({"no_such_key": 1})


def test_config_defaults_merge_and_tag(ref):
    import deeprl_amd as d
    want = ref["host_utils"]["config"]
    a = d.Config()
    for k in want["keys"]:
        assert hasattr(a, k), "Config lacks attribute %s" % k
    for k, v in want["plain"].items():
        va = getattr(a, k)
        assert va == v, (k, va, v)
    a.merge(dict(game="X-v0", n_step=3, tag="t"))
    assert [a.game, a.n_step, a.tag] == want["merged"]
    pa = dict(game="G", run=2, lr=0.1, fn=len)
    d.generate_tag(pa)
    assert pa["tag"] == want["tag"]


# ---------------------------------------------------------------------------------------------------------------
# loss oracles against the reference's own compute_loss on RANDOM shapes / seeds (the committed fixtures cover
# fixed cases).  The generator drove the reference agents as unbound methods on a stand-in, as tests/golden/make_golden.py does.
@pytest.mark.parametrize("seed", range(6))
def test_loss_oracles_equal_live_reference_on_random_cases(ref, seed):
    import torch.nn.functional as F
    from oracle import loss_oracle as L
    want = ref["loss_cases"][seed]
    c = C.loss_case(seed)
    double_q, gamma_n = c["double_q"], c["gamma_n"]
    tr = c["tr"]
    act, rew, msk = torch.tensor(tr["action"]), torch.tensor(tr["reward"], dtype=torch.float32), torch.tensor(tr["mask"], dtype=torch.float32)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    # --- DQN
    q, qt, qo = c["q"].requires_grad_(True), c["qt"], c["qo"]
    got = L.dqn_td_error(q, qt, act, rew, msk, gamma_n, q_next_online=qo if double_q else None)
    assert torch.equal(got, f32(want["dqn"]))
    gg, = torch.autograd.grad(L.dqn_reduce(got), q)
    assert torch.equal(gg, f32(want["dqn_grad"]))
    # --- C51
    n_atoms, vmin, vmax = c["n_atoms"], c["vmin"], c["vmax"]
    atoms = torch.tensor(np.linspace(vmin, vmax, n_atoms), dtype=torch.float32)
    assert torch.equal(atoms, f32(want["atoms"]))
    lg, lt, lo = c["lg"].requires_grad_(True), c["lt"], c["lo"]
    got = L.c51_kl(F.log_softmax(lg, dim=-1), F.softmax(lt, dim=-1), act, rew, msk, gamma_n, atoms, vmin, vmax,
                   prob_next_online=F.softmax(lo, dim=-1) if double_q else None)
    np.testing.assert_allclose(got.detach().numpy(), np.asarray(want["c51"], dtype=np.float32), rtol=1e-6, atol=1e-6)
    # --- QR-DQN
    th, tt = c["th"].requires_grad_(True), c["tt"]
    got = L.qr_loss(th, tt, act, rew, msk, gamma_n)
    np.testing.assert_allclose(got.detach().numpy(), np.asarray(want["qr"], dtype=np.float32), rtol=1e-6, atol=1e-6)


def test_network_modules_have_the_reference_names_and_initial_values(ref, monkeypatch):
    """Same seed -> same state_dict (names, order, shapes, initial values) as the reference's modules: checkpoints
    interchange key by key.  Covers the heads the on-policy / DQN-family goldens do not construct (Dueling, Rainbow +
    NoisyLinear, OptionCritic, DDPG, TD3).  Names, order, shapes exactly; values through crosscheck_cases.value_digest
    within float32 rounding (the recording was made on another host CPU).  (Forward passes need the HIP kernels:
    tests/test_gpu_more_agents.py.)"""
    import deeprl_amd as d
    d.select_device(-1)
    # the noisy layers draw their first noise in the constructor: at the default scale of both libraries, as recorded
    # (whatever an earlier test of the session set)
    monkeypatch.setattr(d.Config, "NOISY_LAYER_STD", 0.1)
    makers = C.module_makers(d)
    want = ref["modules"]["state_dicts"]
    assert len(makers) == len(want)
    z = np.load(C.MODULES_NPZ, allow_pickle=False)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # as the generator ran: orthogonal_'s QR may block differently on more threads
    try:
        for i, (mk, w) in enumerate(zip(makers, want)):
            torch.manual_seed(1)
            C.assert_state_dict_records_match(C.state_dict_record(mk().state_dict()), w, C.modules_npz_values(z, "sd%d" % i))
    finally:
        torch.set_num_threads(threads)


def test_noisy_layers_draw_their_noise_like_the_reference(ref, monkeypatch):
    """NoisyLinear.reset_noise / RainbowNet.reset_noise (network_utils.py:73-80, network_heads.py:72-76): same generator
    words, same layer order, same factorised epsilon as the reference's modules, and the generator ends at the same place."""
    import deeprl_amd as d
    d.select_device(-1)
    monkeypatch.setattr(d.Config, "NOISY_LAYER_STD", 0.5)
    (meta, values), tail = C.noisy_rainbow_record(d)
    want = ref["modules"]["noisy_rainbow"]
    C.assert_state_dict_records_match((meta, values), want["state_dict"],
                                      C.modules_npz_values(np.load(C.MODULES_NPZ, allow_pickle=False), "noisy"))
    assert torch.equal(torch.tensor(tail), torch.tensor(want["tail"]))


def test_random_processes_consume_np_random_like_the_reference(ref):
    import deeprl_amd as d
    for name in ("OrnsteinUhlenbeckProcess", "GaussianProcess"):
        mine, want = C.random_process_record(d, name), ref["modules"]["random_processes"][name]
        assert np.array_equal(np.asarray(mine["samples"]), np.asarray(want["samples"])) and mine["tail"] == want["tail"]


def test_run_steps_cadence_equals_reference(ref):
    """run_steps (misc.py:19-35): the same sequence of save / log / eval / step / switch_task / close calls for an agent
    whose step() advances total_steps by 4."""
    import deeprl_amd as d
    assert C.run_steps_trace(d.run_steps, d.Config) == ref["host_utils"]["run_steps"]
