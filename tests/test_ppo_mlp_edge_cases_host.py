"""CPU proofs about tests/ppo_mlp_edge_cases.py, before anything runs on a GPU: every case reaches the path it is named for and
the case tables name every instantiation of csrc/ppo_mlp.hip's launchers; the float32 CPU run of the reference stays within 0.3 x
every bar against the float64 run on every case's inputs (the inputs carry the bars); every KL gate of the float64 run is clear of
the limit; the std sweep has rows on both sides of the clip range and an approx_kl float32 can carry; the pack restatement equals
a direct gather; oracle.rollout's new forward_dtype keyword leaves its default output as it was."""
import numpy as np
import pytest
import torch

import ppo_mlp_edge_cases as E
from oracle import ppo_mlp_oracle as O


def _ids(cases):
    return [c["name"] for c in cases]


DUMPED = E.UPDATE_CASES + E.STD_CASES      # the cases whose first minibatch the GPU tests compare through the debug instantiation


# ------------------------------------------------------------------------------------------------ the tables
def test_update_table_names_every_instantiation_and_every_edge():
    shapes = [E.update_shape(c) for c in E.UPDATE_CASES]
    assert {s['product'] for s in shapes} == {(16, 0, 0), (32, 0, 0), (64, 0, 0), (64, 0, 17), (64, 0, 11)}
    assert {s['debug'] for s in shapes} == {(16, 1, 0), (32, 1, 0), (64, 1, 0)}
    for hidden in (16, 32):
        assert {s['S'] for s in shapes if s['H'] == hidden} == {1, 15, 16, 17, 33, 64}
    assert {s['S'] for s in shapes if s['H'] == 64} == {1, 11, 16, 17, 32, 33, 48}
    assert {1, 4, 5, 16} <= {s['A'] for s in shapes}
    assert {1, 15, 16, 17, 33, 63, 64} <= {s['MB'] for s in shapes}
    assert any(s['n'] < s['MB'] and s['n'] == 3 and s['MB'] == 64 for s in shapes)
    assert any(s['n'] == 1 for s in shapes)
    assert any(s['rows_last'] == 1 and s['per_epoch'] > 1 for s in shapes)
    assert any(s['MB'] == 33 and s['rows_last'] == 16 and s['MT_last'] < s['MT'] for s in shapes)
    assert all(s['total'] <= 6 for s in shapes)
    # a compiled-in observation size skips MFMA steps only at 17 (k tile 1 holds one column); at 11 every step of its one tile runs
    assert {s['SC']: len(s['skipped']) for s in shapes if s['SC']} == {17: 3, 11: 0}
    assert all(E.supported(s['S'], s['A'], s['H'], s['MB']) for s in shapes)
    assert E.update_lds_floats(64, 48) <= E.LDS_FLOATS_MAX < E.update_lds_floats(64, 49)
    assert len(E.CASES_BY_NAME) == len(E.ALL_UPDATE_CASES) and len({c['seed'] for c in E.ALL_UPDATE_CASES}) == len(E.ALL_UPDATE_CASES)
    assert not E.BAR_OVERRIDES and all(g in E.BAR_GROUPS for _, g in E.BAR_OVERRIDES)        # (an override needs its float32 figure and the reason beside it: see the module's docstring)
    assert [c['std0'] for c in E.STD_CASES] == [-3.0, -2.0, 0.5413, 5.0, 19.5, 20.5]
    assert E.WARM_CASE['steps0'] == (5000, 4990) and E.CONTINUATION_CASE['launches'] == 2
    assert E.GATE_MIDWAY_CASE['H'] in (16, 32) and E.GATE_CLOSED_CASE['target_kl'] == 0.01
    assert [w for _, w in E.UPDATE_REFUSALS] == ["state 0", "state 65", "hidden 64 with state 49: LDS", "action 0", "action 17", "hidden 48",
                                                 "minibatch 0", "minibatch 65", "actor without std", "eps 0", "beta1 1"]


@pytest.mark.parametrize("c", E.ALL_UPDATE_CASES, ids=_ids(E.ALL_UPDATE_CASES))
def test_update_case_reaches_its_path(c):
    assert c['path'](E.update_shape(c)), E.update_shape(c)


def test_rollout_table_names_every_instantiation_and_every_edge():
    shapes = {c['name']: E.rollout_shape(c) for c in E.ROLLOUT_CASES}
    assert {s['H'] for s in shapes.values()} == {16, 32, 64}
    got = sorted((s['H'], s['N'], s['S'], s['A'], s['T'], s['horizon']) for s in shapes.values())
    for want in [(16, 1, 1, 1, 1, 1), (16, 64, 17, 16, 3, 2), (32, 33, 64, 5, 2, 5), (64, 64, 48, 4, 2, 3), (64, 9, 11, 3, 6, 4)]:
        assert want in got
    assert [s for s in shapes.values() if s['env0'] == 7 and s['n_global'] == 40]
    assert [s for s in shapes.values() if s['rms_update'] == 0]
    assert {s['tiers'] for s in shapes.values()} == {1, 3} and max(s['comps'] for s in shapes.values()) == 3072
    assert any(s['pow2'] and s['chunks'] > 1 for s in shapes.values()) and any(s['chunks'] == 5 for s in shapes.values())
    assert any(s['idle_heads'] > 0 and s['H'] == 16 and s['N'] > 16 for s in shapes.values())
    assert any(s['rows_a'] % 64 == 0 for s in shapes.values()) and any(0 < s['rows_a'] % 64 and s['blocks'] > 1 for s in shapes.values())
    for c in E.ROLLOUT_CASES:
        assert c['path'](shapes[c['name']]), shapes[c['name']]
        assert E.supported(c['S'], c['A'], c['H'], 1) and 1 <= c['N'] <= 64
    assert [w for _, w in E.ROLLOUT_REFUSALS] == ["n_env 0", "n_env 65", "t_len 0", "horizon 0", "n_global < n_env"]


def test_pack_and_stand_alone_tables():
    for c in E.PACK_CASES:
        assert c['path'](E.pack_shape(c)), E.pack_shape(c)
    assert [(c['S'], c['A'], c['MB'], c['n'], c['epochs']) for c in E.PACK_CASES] == [(1, 1, 1, 1, 1), (17, 6, 64, 200, 2), (64, 16, 1, 190, 2)]
    assert E.RMS_CASES == [(1, 1), (3, 257), (2, 4096)] and E.RMS_REFUSED_D == 4097
    assert any(d > 256 for _, d in E.RMS_CASES) and 2 * 4096 * 8 == 64 * 1024
    assert E.GAUSS_CASES == [(1, 1), (40, 32), (64, 16)] and E.GAUSS_REFUSED_A == 33 and sum(n * a > 256 for n, a in E.GAUSS_CASES) == 2
    assert E.ENV_CASES == [(1030, 1, 1, 1), (3, 64, 2, 7), (5, 63, 16, 2)] and E.ENV_REFUSED_S == 65
    assert any(n > E.ENV_GRID_CAP for n, _, _, _ in E.ENV_CASES)


# ------------------------------------------------------------------------------------------------ the inputs carry the bars
@pytest.mark.parametrize("c", E.ALL_UPDATE_CASES, ids=_ids(E.ALL_UPDATE_CASES))
def test_float32_reference_run_stays_within_a_fraction_of_every_bar_and_gates_are_clear(c):
    """A condition, not a measurement: a case whose float32 CPU run of the reference exceeds 0.3 x a bar gets another seed."""
    wide, narrow = E.reference(c), E.run_reference(c, torch.float32)
    assert len(wide['launches']) == c['launches']
    for got, want in zip(narrow['launches'], wide['launches']):
        assert got['steps'] == want['steps'] and got['counts'] == want['counts']
        for group, (r, name) in E.compare_state(got, want).items():
            assert r <= E.HOST_FRACTION * E.bar(c['name'], group), (group, name, r)
    if c in DUMPED:
        for key, r in E.compare_first(narrow['first'], wide['first']).items():
            assert r <= E.HOST_FRACTION * E.bar(c['name'], "inter"), (key, r)
        # the first minibatch means something: a gradient in every tensor of the critic, and in the actor's std
        assert all(float(np.abs(g).max()) > 0 for g in wide['first']['critic_grads']) and float(np.abs(wide['first']['actor_grads'][6]).max()) > 0
    per_epoch = (c['n'] + c['MB'] - 1) // c['MB']
    assert len(wide['kls']) == c['launches'] * c['epochs'] * per_epoch
    for kl in wide['kls']:
        assert E.gate_margin(kl, c['target_kl']) >= 1.0, (kl, 1.5 * c['target_kl'])
    assert wide['launches'][-1]['steps'][1] == c['steps0'][1] + len(wide['kls'])


def test_per_minibatch_reference_equals_one_call_over_all_minibatches():
    """The reference is run one minibatch per call (opt_state carried) to see every approx_kl: the same bits as one call."""
    for c in (E.CASES_BY_NAME["h32-s15-a5-mb17-remainder-one-row"], E.GATE_MIDWAY_CASE, E.WARM_CASE):
        a, b = E.reference(c), E.run_reference(c, torch.float64, per_minibatch=False)
        for x, y in zip(a['launches'], b['launches']):
            assert x['steps'] == y['steps'] and x['counts'] == y['counts'] and x['out3'] == y['out3']
            for role in ("actor", "critic"):
                for k in x[role]:
                    assert np.array_equal(x[role][k], y[role][k]) and np.array_equal(x['m'][role][k], y['m'][role][k])
                    assert np.array_equal(x['v'][role][k], y['v'][role][k])


def test_special_update_cases_do_what_they_are_named_for():
    closed = E.reference(E.GATE_CLOSED_CASE)
    assert closed['launches'][0]['counts'] == (0, 3) and 0.06 <= closed['kls'][0] <= 0.1 and min(closed['kls']) >= 2 * 1.5 * 0.01
    inp = E.update_inputs(E.GATE_CLOSED_CASE)
    assert all(np.array_equal(closed['launches'][0]['actor'][k], v.numpy().astype(np.float64)) for k, v in inp['actor'].items())
    mid = E.reference(E.GATE_MIDWAY_CASE)
    opens = [kl <= 1.5 * E.GATE_MIDWAY_CASE['target_kl'] for kl in mid['kls']]
    assert opens[0] and not all(opens) and 3 <= mid['launches'][0]['counts'][0] <= 9 and mid['launches'][0]['counts'][1] == 12
    warm = E.reference(E.WARM_CASE)
    assert warm['launches'][0]['steps'] == (5003, 4993)
    cont = E.reference(E.CONTINUATION_CASE)
    assert cont['launches'][1]['steps'] == (6, 6) and cont['launches'][0]['steps'] == (3, 3)
    (e0, p0), (e1, p1) = E.update_inputs(E.CONTINUATION_CASE)['launches']
    assert not np.array_equal(e0[0].numpy(), e1[0].numpy())          # fresh entries for the second launch


@pytest.mark.parametrize("c", E.STD_CASES, ids=_ids(E.STD_CASES))
def test_std_sweep_stays_where_float32_carries_the_bar(c):
    ref = E.reference(c)
    assert 0.005 <= ref['kls'][0] <= 0.1, ref['kls'][0]
    inside, outside = E.clip_census(c)
    assert inside >= 4 and outside >= 4, (inside, outside)
    std = E.update_inputs(c)['actor']['std'].numpy()
    assert np.all(std == np.float32(c['std0']))                      # the swept value itself, on its side of softplus' threshold
    assert (c['std0'] > 20.0) == (c['std0'] == 20.5)


# ------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("c", E.PACK_CASES[:2], ids=_ids(E.PACK_CASES[:2]))
def test_pack_restatement_equals_a_direct_gather(c):
    inp = E.pack_inputs(c)
    sh = E.pack_shape(c)
    img = E.pack_reference(inp, c['MB']).reshape(c['epochs'], sh['per_epoch'], -1)
    assert img.dtype == np.float32 and img.size == sh['floats']
    S, A, MB, n = c['S'], c['A'], c['MB'], c['n']
    for e in range(c['epochs']):
        for k in range(sh['per_epoch']):
            rows = inp['perm'][e, k * MB:(k + 1) * MB]
            obs = img[e, k, :64 * sh['ldx']].reshape(64, sh['ldx'])
            aux = img[e, k, 64 * sh['ldx']:].reshape(64, 20)
            assert np.array_equal(obs[:len(rows), :S], inp['state'][rows]) and np.array_equal(aux[:len(rows), :A], inp['action'][rows])
            assert np.array_equal(aux[:len(rows), 16:19], np.concatenate([inp['log_pi_a'][rows], inp['advantage'][rows], inp['ret'][rows]], axis=1))
            # everything else is zero
            assert np.count_nonzero(obs) <= len(rows) * S and np.count_nonzero(aux) <= len(rows) * (A + 3)
            assert not obs[len(rows):].any() and not aux[len(rows):].any() and not obs[:, S:].any() and not aux[:, A:16].any() and not aux[:, 19].any()
    assert len(inp['perm'][-1, (sh['per_epoch'] - 1) * MB:]) == sh['rows_last']


# ------------------------------------------------------------------------------------------------ rollout
def test_rollout_forward_dtype_default_reproduces_the_previous_output(golden):
    """tests/golden/oracle_pins/ppo_rollout_f32.npz: oracle.ppo_mlp_oracle.rollout as it was before it took forward_dtype, at two shapes (one a
    shard), every output and the final statistics.  The default (float32 forwards) gives the same bits and dtypes."""
    from oracle.numerics_oracle import MeanStdNormalizerOracle
    g = golden("oracle_pins/ppo_rollout_f32")
    for tag, (n, S, A, H, T, horizon, env0, ng) in dict(a=(5, 17, 6, 64, 12, 5, 0, 5), b=(3, 4, 2, 16, 7, 3, 2, 9)).items():
        actor, critic = O.init_params(S, A, H, seed=12)
        envs = [O.ContinuousEnvOracle(70 + i, S, A, horizon) for i in range(n)]
        raw = np.stack([e.reset() for e in envs])
        norm = MeanStdNormalizerOracle()
        cur = np.asarray(norm(raw), dtype=np.float32)
        w = O.rollout(actor, critic, envs, raw, norm, cur, T, 4, 3, n_global=ng, env0=env0)
        assert sorted(w) == sorted(k[2:] for k in g if k.startswith(tag + "_") and k[2:] not in ("mean", "var"))
        for k, v in w.items():
            assert v.dtype == g[tag + "_" + k].dtype and np.array_equal(v, g[tag + "_" + k]), (tag, k)
        assert np.array_equal(norm.rms.mean, g[tag + "_mean"]) and np.array_equal(norm.rms.var, g[tag + "_var"])


@pytest.mark.parametrize("c", E.ROLLOUT_CASES, ids=_ids(E.ROLLOUT_CASES))
def test_rollout_float32_forwards_stay_within_a_fraction_of_the_bar(c):
    wide, narrow = E.rollout_reference(c), E.run_rollout(c, torch.float32)
    for key, r in E.compare_rollout(narrow['want'], wide['want']).items():
        assert r <= E.HOST_FRACTION * E.bar(c['name'], "rollout"), (key, r)
    w = wide['want']
    assert all(w[k].dtype == np.float32 for k in E.ROLLOUT_KEYS + ("reward", "mask"))
    # rewards, terminals and counters do not depend on the actions: the same in both runs
    assert np.array_equal(w['mask'], narrow['want']['mask']) and np.array_equal(w['reward'], narrow['want']['reward'])
    assert np.array_equal(wide['counters'], narrow['counters'])
    np.testing.assert_allclose(narrow['rms1'], wide['rms1'], rtol=0.3e-7, atol=0)
    if c['horizon'] == 1:
        assert not w['mask'].any()
    elif c['T'] * c['N'] >= 20:
        assert (w['mask'] == 0).any() and (w['mask'] == 1).any()
    if not c['rms_update']:
        assert np.array_equal(wide['rms0'], wide['rms1'])
    else:
        assert wide['rms1'][-1] == wide['rms0'][-1] + c['T'] * c['N']


def test_shard_draws_its_rows_of_the_global_noise():
    c = next(c for c in E.ROLLOUT_CASES if c['env0'])
    for t in range(c['sampler_step0'], c['sampler_step0'] + c['T']):
        whole = O.gauss_noise(c['noise_seed'], t, c['n_global'], np.arange(c['n_global']), c['A'])
        part = O.gauss_noise(c['noise_seed'], t, c['n_global'], c['env0'] + np.arange(c['N']), c['A'])
        assert np.array_equal(part, whole[c['env0']:c['env0'] + c['N']])
        assert not np.array_equal(part, O.gauss_noise(c['noise_seed'], t, c['N'], np.arange(c['N']), c['A']))
