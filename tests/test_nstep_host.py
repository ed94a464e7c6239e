"""n-step DQN on pixels, host side (no GPU): the zoo entry against the reference's examples.py::n_step_dqn_pixel, the committed
fixture against a live run of the reference's NStepDQNAgent.step (tests/golden/make_golden_nstep.py), and the device path's
up-front exploration plan (support.plan_epsilon_greedy) against the reference's epsilon_greedy called step by step."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_shim
from golden import crosscheck_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "nstep", "n_step_dqn_pixel.npz")

needs_ref = pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    """These tests seed np.random and switch the package's device; the tests after them see what they saw before."""
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


def _python(code, env=None):
    """Runs `code` in a fresh interpreter (tests/ and the repository root importable; user site-packages ignored as in this
    process) -> its stdout.  The reference is loaded there, never into the test process: importing it installs stand-in modules
    and import hooks that must not leak into the other tests."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, **(env or {}))
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    return subprocess.check_output([sys.executable] + flags + ["-c", code], env=env, cwd=ROOT).decode()


_REF_CONFIG = """
import json, os, sys
import numpy as np
import deeprl_amd as d
from deeprl_amd import launch
import ref_shim
from golden import crosscheck_cases as C
d.select_device(-1)
mod = launch.load_examples(os.path.join(ref_shim.REFERENCE_ROOT, "examples.py"), "ref_examples_nstep")
got = {}
for a in C.ZOO_AGENTS:
    setattr(mod, a, lambda cfg, _a=a: (_a, cfg))
mod.run_steps = lambda pair: got.update(agent=pair[0], cfg=pair[1])
np.random.seed(0)
mod.n_step_dqn_pixel(game=%r)
print(json.dumps(dict(agent=got["agent"], config=C.describe_config(got["cfg"]))))
"""


@needs_ref
def test_zoo_n_step_dqn_pixel_equals_reference_example():
    """examples.py:427-447 run live (agent and run_steps replaced by a capture, as make_golden_crosscheck.py does for the other
    entries) builds the same Config as zoo.config('n_step_dqn_pixel')."""
    import json
    import deeprl_amd as d
    from deeprl_amd import zoo
    game = "BreakoutNoFrameskip-v4"
    rec = json.loads(_python(_REF_CONFIG % game).strip().splitlines()[-1])
    want = rec["config"]
    assert rec["agent"] == zoo.ZOO["n_step_dqn_pixel"]["agent"] == "NStepDQNAgent"
    d.select_device(-1)
    np.random.seed(0)
    have = C.describe_config(zoo.config("n_step_dqn_pixel", game=game))
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert want[k] == have[k], "%s: reference %s, zoo %s" % (k, want[k], have[k])


def _close(fresh, committed):
    """Float arrays of the fixture: the reference's CPU arithmetic (oneDNN convolutions, vectorised reductions) picks its kernels
    by the host's instruction set, so a regeneration on another CPU may differ in the last bits -- within 1e-5 of scale, the bar
    the GPU test holds the device path to.  Everything discrete (actions, generator positions, step counters) is exact."""
    a, b = fresh.astype(np.float64), committed.astype(np.float64)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    return float(np.abs(a - b).max()) <= 1e-5 * scale if b.size else True


@needs_ref
def test_nstep_fixture_is_the_reference_output(tmp_path):
    """tests/golden/make_golden_nstep.py run live: the same keys, the same actions / generator positions / step counts bit for
    bit, and floats bit for bit where this host computes them the same way (within 1e-5 of scale otherwise: see _close)."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable] + flags + [os.path.join(ROOT, "tests", "golden", "make_golden_nstep.py")], env=env,
                          stdout=subprocess.DEVNULL)
    fresh = dict(np.load(os.path.join(str(tmp_path), "nstep", "n_step_dqn_pixel.npz")))
    committed = dict(np.load(FIXTURE))
    assert sorted(fresh) == sorted(committed)
    for k in committed:
        assert fresh[k].dtype == committed[k].dtype and fresh[k].shape == committed[k].shape, k
        if committed[k].dtype.kind in "iub" or k.endswith(("_action", "_rng", "_total_steps", "_mask", "_reward")):
            assert np.array_equal(fresh[k], committed[k]), k
        else:
            assert _close(fresh[k], committed[k]), k


def test_nstep_fixture_exercises_both_branches_and_a_target_sync():
    g = np.load(FIXTURE)
    steps = sorted({int(k[1:k.index("_")]) for k in g.files if k.startswith("s")})
    assert len(steps) >= 3
    greedy = random = 0
    for s in steps:
        q, a = g["s%d_q" % s], g["s%d_action" % s]
        hit = a == np.argmax(q, axis=-1)
        greedy, random = greedy + int(hit.sum()), random + int((~hit).sum())
    assert greedy > 0 and random > 0
    # the target network moves between steps (a sync inside the run) and stays behind the online network at least once
    names = [k[len("s0_target_"):] for k in g.files if k.startswith("s0_target_")]
    moved = [any(not np.array_equal(g["s%d_target_%s" % (s, n)], g["s%d_target_%s" % (s + 1, n)]) for n in names)
             for s in steps[:-1]]
    assert any(moved)
    assert any(not np.array_equal(g["s%d_target_%s" % (s, n)], g["s%d_param_%s" % (s, n)]) for s in steps for n in names)


_REF_EPSILON_GREEDY = """
import json, zlib
import numpy as np
import ref_shim
from deeprl_amd.support import LinearSchedule
eg = ref_shim.load().epsilon_greedy
qs = np.load(%r)
sched = LinearSchedule(0.9, 0.05, 40)
np.random.seed(123)
acts = [eg(sched(qs.shape[1]), qs[t]).tolist() for t in range(qs.shape[0])]
_, key, pos, _, _ = np.random.get_state()
print(json.dumps(dict(actions=acts, pos=int(pos), key=zlib.crc32(np.ascontiguousarray(key).tobytes()), current=sched.current)))
"""


@pytest.mark.parametrize("n_rows,n_actions,t_len", [(4, 4, 5), (16, 6, 5), (3, 18, 7)])
def test_planned_exploration_equals_step_by_step_epsilon_greedy(tmp_path, n_rows, n_actions, t_len):
    """plan_epsilon_greedy draws a whole rollout's exploration first; selecting explore ? random : argmax(q) afterwards gives the
    actions of t_len epsilon_greedy calls on the same q arrays (exact ties included: the lower index) and leaves np.random and
    the schedule where those calls leave them.  The step-by-step side is the reference's torch_utils.epsilon_greedy when the
    reference checkout is present (in a fresh interpreter), and the package's restatement of it as well."""
    import json
    import zlib
    from deeprl_amd.support import LinearSchedule, epsilon_greedy, plan_epsilon_greedy
    rs = np.random.RandomState(n_rows * 100 + n_actions)
    qs = rs.standard_normal((t_len, n_rows, n_actions)).astype(np.float32)
    qs[:, ::2, 1] = qs[:, ::2, 0] = qs[:, ::2].max(axis=-1) + 1.0       # exact ties on the top value in every other row
    qs[0, 0, :] = 0.25                                                  # a row that is one tie
    sides = []
    sched_a = LinearSchedule(0.9, 0.05, 40)
    np.random.seed(123)
    acts = np.stack([epsilon_greedy(sched_a(n_rows), qs[t]) for t in range(t_len)])
    _, key, pos, _, _ = np.random.get_state()
    sides.append((acts, int(pos), zlib.crc32(np.ascontiguousarray(key).tobytes()), sched_a.current))
    if ref_shim.available():
        path = os.path.join(str(tmp_path), "qs.npy")
        np.save(path, qs)
        rec = json.loads(_python(_REF_EPSILON_GREEDY % path).strip().splitlines()[-1])
        sides.append((np.asarray(rec["actions"], dtype=np.int64), rec["pos"], rec["key"], rec["current"]))
    sched_b = LinearSchedule(0.9, 0.05, 40)
    np.random.seed(123)
    explore, rand = plan_epsilon_greedy(sched_b, t_len, n_rows, n_actions, n_rows)
    have = np.where(explore, rand, np.argmax(qs, axis=-1))
    _, key, pos, _, _ = np.random.get_state()
    assert have.dtype == np.int64
    assert explore.any() and (~explore).any()
    for want, w_pos, w_key, w_current in sides:
        assert np.array_equal(have, want)
        assert (int(pos), zlib.crc32(np.ascontiguousarray(key).tobytes())) == (w_pos, w_key)
        assert sched_b.current == w_current
    assert np.all(have[:, ::2][~explore[:, ::2]] == 0)         # tied rows that were greedy took the lower index
