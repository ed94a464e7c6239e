"""The host side of dqn_feature's seed lanes (deeprl_amd/seed_batch.py), without a GPU: the draws from a lane's own RandomState
are the global stream's and leave the global stream alone, the staged block's per-lane layout, the mismatch detector's
reasons, the ctypes mirrors of the two new lane structs."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _schedule():
    from deeprl_amd.support import LinearSchedule
    return LinearSchedule(0.8, 0.1, 30)


@pytest.mark.parametrize("seed", [0, 13, 2 ** 31 - 1])
@pytest.mark.parametrize("actor_steps, exploration_steps", [(0, 100), (6, 8), (50, 8)])     # all below, crossed inside, all behind
def test_plan_from_a_random_state_is_the_global_plan(seed, actor_steps, exploration_steps):
    """plan_actor_epsilon_greedy(..., rng=RandomState(s)) gives what the global function gives after np.random.seed(s): flags,
    random actions, the schedule's position and the generator's tail; the global stream is not touched."""
    from deeprl_amd.support import plan_actor_epsilon_greedy
    np.random.seed(seed)
    s_a = _schedule()
    want = plan_actor_epsilon_greedy(s_a, 8, 2, actor_steps, exploration_steps)
    want_tail = np.random.randint(0, 1 << 30, size=3)
    np.random.seed(seed + 1)
    before = np.random.get_state()
    rs, s_b = np.random.RandomState(seed), _schedule()
    got = plan_actor_epsilon_greedy(s_b, 8, 2, actor_steps, exploration_steps, rng=rs)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == np.bool_ and got[1].dtype == np.int64
    assert s_a.current == s_b.current and np.array_equal(rs.randint(0, 1 << 30, size=3), want_tail)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


@pytest.mark.parametrize("seed", [0, 13])
@pytest.mark.parametrize("pos, size", [(5, 5), (3, 24), (23, 24), (0, 24)])      # filling; wrapped with the cursor at both ends
def test_draw_indices_from_a_random_state_is_the_global_draw(seed, pos, size):
    """UniformReplay.draw_indices(rng=RandomState(s)) / draw_uniform_indices(..., rng) give the indices of the global draw after
    np.random.seed(s) -- the rejection loop included: the cursor rejects candidates in every case -- and the same tail."""
    from deeprl_amd.replay import UniformReplay, draw_uniform_indices
    rp = UniformReplay(memory_size=24, batch_size=10, n_step=1, discount=0.99, history_length=1)
    rp.pos, rp._size = pos, size
    assert rp.size() == size
    np.random.seed(seed)
    want = rp.draw_indices()
    want_tail = np.random.randint(0, 1 << 30, size=3)
    np.random.seed(seed + 1)
    before = np.random.get_state()
    rs = np.random.RandomState(seed)
    got = rp.draw_indices(rng=rs)
    assert np.array_equal(got, want) and np.array_equal(rs.randint(0, 1 << 30, size=3), want_tail)
    assert np.array_equal(draw_uniform_indices(size, pos, 10, 1, 1, np.random.RandomState(seed)), want)
    assert all(rp.valid_index(int(i)) for i in got)
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]


@pytest.mark.parametrize("k, batch", [(4, 10), (1, 1), (8, 256), (3, 17), (8, 5)])
def test_lane_layout(k, batch):
    """One lane's staged block is dqn_mlp.Step's (int64 first slot | int64 indices [batch] | int64 random actions [k] | uint8 flags
    [k]); every field keeps its natural alignment in every lane because the lane stride is the size rounded up to 16 bytes."""
    from deeprl_amd.seed_batch import lane_layout
    lay = lane_layout(k, batch)
    assert lay['idx'] == 8 and lay['rand'] == 8 + 8 * batch and lay['flag'] == lay['rand'] + 8 * k
    assert lay['size'] >= lay['flag'] + k and lay['size'] % 8 == 0 and lay['size'] - (lay['flag'] + k) < 8
    assert lay['stride'] % 16 == 0 and 0 <= lay['stride'] - lay['size'] < 16
    for lane in range(5):
        base = lane * lay['stride']
        assert all((base + lay[f]) % 8 == 0 for f in ('idx', 'rand', 'flag'))
        assert base + lay['flag'] + k <= base + lay['stride']       # (a lane's last flag lies ahead of the next lane's first slot)


def _fake_agent(hidden=16, gate=None, **over):
    from deeprl_amd import nets
    from deeprl_amd.support import Config, LinearSchedule
    f = dict(sgd_update_frequency=4, exploration_steps=6, target_network_update_freq=3, gradient_clip=5, discount=0.99, double_q=False,
             batch=10, memory_size=24, lr=0.001, eps=(0.8, 0.1, 30))
    f.update(over)
    c = Config()
    c.sgd_update_frequency, c.exploration_steps, c.target_network_update_freq = f['sgd_update_frequency'], f['exploration_steps'], f['target_network_update_freq']
    c.gradient_clip, c.discount, c.double_q = f['gradient_clip'], f['discount'], f['double_q']
    c.random_action_prob = LinearSchedule(*f['eps'])
    body = nets.FCBody(4, (hidden, hidden)) if gate is None else nets.FCBody(4, (hidden, hidden), gate=gate)
    net = nets.VanillaNet(2, body)
    rp = types.SimpleNamespace(batch_size=f['batch'], memory_size=f['memory_size'])
    return types.SimpleNamespace(config=c, network=net, optimizer=torch.optim.RMSprop(net.parameters(), f['lr']), _inner_replay=lambda: rp)


@pytest.mark.parametrize("field, over", [("shape", dict(hidden=32)), ("shape", dict(gate=torch.tanh)),
                                         ("sgd_update_frequency", dict(sgd_update_frequency=2)), ("batch", dict(batch=11)),
                                         ("memory_size", dict(memory_size=25)), ("schedule", dict(eps=(0.8, 0.1, 31))),
                                         ("exploration_steps", dict(exploration_steps=7)),
                                         ("target_network_update_freq", dict(target_network_update_freq=4)),
                                         ("gradient_clip", dict(gradient_clip=None)), ("gradient_clip", dict(gradient_clip=4)),
                                         ("discount", dict(discount=0.9)), ("optimizer", dict(lr=0.002)), ("double_q", dict(double_q=True))])
def test_mismatch_detector_names_the_field(field, over):
    from deeprl_amd.seed_batch import first_mismatch, lane_signature
    hidden, gate = over.pop("hidden", 16), over.pop("gate", None)
    same = [lane_signature(_fake_agent()) for _ in range(3)]
    assert first_mismatch(same) is None and first_mismatch(same[:1]) is None
    why = first_mismatch(same[:2] + [lane_signature(_fake_agent(hidden, gate, **over))])
    assert why.startswith("lane 2 differs from lane 0 in %s " % field), why


def test_mismatch_detector_reports_the_first_lane_and_field():
    from deeprl_amd.seed_batch import first_mismatch, lane_signature
    sigs = [lane_signature(_fake_agent()), lane_signature(_fake_agent(batch=11, double_q=True)), lane_signature(_fake_agent(hidden=32))]
    assert first_mismatch(sigs).startswith("lane 1 differs from lane 0 in batch (11, lane 0: 10)")
    centred = _fake_agent()
    centred.optimizer = torch.optim.RMSprop(centred.network.parameters(), 0.001, centered=True)
    assert "in optimizer" in first_mismatch([sigs[0], lane_signature(centred)])


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
@pytest.mark.parametrize("which", ["dra_optim_lane", "dra_copy_lane"])
def test_lane_struct_mirrors_match_the_header(tmp_path, which):
    """tests/test_struct_layouts.py's probe over the two lane structs: size and the offset of every field as gcc lays them out."""
    from deeprl_amd import seed_batch
    mirror = dict(dra_optim_lane=seed_batch.OptimLane, dra_copy_lane=seed_batch.CopyLane)[which]
    names = [f[0] for f in mirror._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "include/deeprl_amd.h"', 'int main(void) {',
           '  printf("%%zu\\n", sizeof(%s));' % which]
    src += ['  printf("%%zu\\n", offsetof(%s, %s));' % (which, f) for f in names] + ['  return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", str(c), "-I", ROOT, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(mirror) and got[1:] == [getattr(mirror, n).offset for n in names]


def test_run_seeds_refuses_other_entries():
    from deeprl_amd import zoo
    with pytest.raises(ValueError, match="only dqn_feature runs its seeds as lanes, a2c_feature has no lane form"):
        zoo.run_seeds("a2c_feature", (1, 2))


def test_more_than_64_seeds_are_refused_before_anything_is_built():
    from deeprl_amd.seed_batch import MAX_LANES, DQNFeatureSeeds

    def make_config(seed):
        raise AssertionError("no lane may be built")
    assert MAX_LANES == 64
    for seeds in (range(65), ()):
        with pytest.raises(ValueError, match="runs 1 to 64 seeds as lanes, not %d" % len(seeds)):
            DQNFeatureSeeds(make_config, seeds)
