"""Option-critic on pixels, host side (no GPU): the zoo entry against the reference's examples.py::option_critic_pixel, the
committed fixture against a live run of the reference's OptionCriticAgent.step (tests/golden/make_golden_option_critic.py), what
the fixture covers, and the midpoint uniforms the GPU test feeds the device path in place of torch's Categorical draws."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_shim
from golden import crosscheck_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "option_critic", "option_critic_pixel.npz")
STEPS, N_ENVS = 4, 4

needs_ref = pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    """These tests seed np.random and switch the package's device; the tests after them see what they saw before."""
    import deeprl_amd as d
    state, device = np.random.get_state(), d.Config.DEVICE
    yield
    np.random.set_state(state)
    d.Config.DEVICE = device


def _python(code):
    """Runs `code` in a fresh interpreter (tests/ and the repository root importable; user site-packages ignored as in this
    process) -> its stdout.  The reference is loaded there, never into the test process."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ)
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
mod = launch.load_examples(os.path.join(ref_shim.REFERENCE_ROOT, "examples.py"), "ref_examples_oc")
got = {}
for a in C.ZOO_AGENTS:
    setattr(mod, a, lambda cfg, _a=a: (_a, cfg))
mod.run_steps = lambda pair: got.update(agent=pair[0], cfg=pair[1])
np.random.seed(0)
mod.option_critic_pixel(game=%r)
s = got["cfg"].random_option_prob
print(json.dumps(dict(agent=got["agent"], config=C.describe_config(got["cfg"]),
                      option_eps=[type(s).__name__, s.current, s.end, s.inc])))
"""


@needs_ref
def test_zoo_option_critic_pixel_equals_reference_example():
    """examples.py:471-492 run live (agent and run_steps replaced by a capture) builds the same Config as
    zoo.config('option_critic_pixel'), the option epsilon schedule (which describe_config does not cover) included."""
    import json
    import deeprl_amd as d
    from deeprl_amd import zoo
    game = "BreakoutNoFrameskip-v4"
    rec = json.loads(_python(_REF_CONFIG % game).strip().splitlines()[-1])
    want = rec["config"]
    assert rec["agent"] == zoo.ZOO["option_critic_pixel"]["agent"] == "OptionCriticAgent"
    d.select_device(-1)
    np.random.seed(0)
    cfg = zoo.config("option_critic_pixel", game=game)
    have = C.describe_config(cfg)
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert want[k] == have[k], "%s: reference %s, zoo %s" % (k, want[k], have[k])
    s = cfg.random_option_prob
    assert [type(s).__name__, s.current, s.end, s.inc] == rec["option_eps"]


_DISCRETE = ("_option", "_prev_option", "_action", "_fresh", "_continued", "_init", "_mask", "_reward", "_total_steps", "_eps")


def _close(fresh, committed):
    """Floats of the fixture: the reference's CPU arithmetic picks its kernels by the host's instruction set, so a regeneration
    on another CPU may differ in the last bits -- within 1e-5 of scale.  Everything discrete is exact."""
    a, b = fresh.astype(np.float64), committed.astype(np.float64)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    return float(np.abs(a - b).max()) <= 1e-5 * scale if b.size else True


@needs_ref
def test_option_critic_fixture_is_the_reference_output(tmp_path):
    """tests/golden/make_golden_option_critic.py run live (its own assertions included): the same keys, the same decisions,
    initial-state flags, masks, rewards, epsilons and step counts bit for bit, floats within 1e-5 of scale."""
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable] + flags + [os.path.join(ROOT, "tests", "golden", "make_golden_option_critic.py")],
                          env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    fresh = dict(np.load(os.path.join(str(tmp_path), "option_critic", "option_critic_pixel.npz")))
    committed = dict(np.load(FIXTURE))
    assert sorted(fresh) == sorted(committed)
    for k in committed:
        assert fresh[k].dtype == committed[k].dtype and fresh[k].shape == committed[k].shape, k
        if committed[k].dtype.kind in "iub" or k.endswith(_DISCRETE):
            assert np.array_equal(fresh[k], committed[k]), k
        else:
            assert _close(fresh[k], committed[k]), k


def _cat(g, name):
    return np.concatenate([g["s%d_%s" % (s, name)].reshape(-1) for s in range(STEPS)])


def test_option_critic_fixture_exercises_every_branch():
    g = np.load(FIXTURE)
    init, opt, prev = _cat(g, "init"), _cat(g, "option"), _cat(g, "prev_option")
    fresh, cont = _cat(g, "fresh"), _cat(g, "continued")
    assert np.array_equal(opt, np.where(init > 0, fresh, cont))        # init rows take the fresh draw, the others the continued
    assert (init > 0).any() and (init == 0).any()
    assert ((init == 0) & (opt != prev)).any() and ((init == 0) & (opt == prev)).any()   # continued and switched, and kept
    assert (init[N_ENVS:] > 0).any() and (_cat(g, "mask") == 0).any()   # episodes end inside the run
    eps = _cat(g, "eps")
    assert np.all(np.diff(eps) < 0)                                     # a decaying option epsilon: a new value every step
    # the greedy option differs from the drawn one somewhere (epsilon matters) and the actions are not all one
    greedy = np.concatenate([np.argmax(g["s%d_q" % s], axis=-1).reshape(-1) for s in range(STEPS)])
    assert (fresh == greedy).any() and (fresh != greedy).any()
    assert len(set(_cat(g, "action").tolist())) > 1
    # the target network is re-synchronised inside the run and stays behind the online network at least once
    names = [k[len("s0_target_"):] for k in g.files if k.startswith("s0_target_")]
    moved = [any(not np.array_equal(g["s%d_target_%s" % (s, n)], g["s%d_target_%s" % (s + 1, n)]) for n in names)
             for s in range(STEPS - 1)]
    assert any(moved)
    assert any(not np.array_equal(g["s%d_target_%s" % (s, n)], g["s%d_param_%s" % (s, n)]) for s in range(STEPS) for n in names)
    # (1 - init) matters: a row with init = 1 has a non-zero termination advantage, so beta_loss drops a term there
    assert np.any((init > 0) & (np.abs(_cat(g, "beta_advantage")) > 0))


def midpoint_uniforms(p, k):
    """The middle of category k's interval of the probability rows p [..., n] (fp32 running sums in index order)."""
    cdf = np.cumsum(p.astype(np.float32), axis=-1, dtype=np.float32)
    hi = np.take_along_axis(cdf, k[..., None], axis=-1)[..., 0]
    lo = np.where(k > 0, np.take_along_axis(cdf, np.maximum(k - 1, 0)[..., None], axis=-1)[..., 0], np.float32(0))
    return ((lo.astype(np.float64) + hi) / 2).astype(np.float32)


def inv_cdf(p, u):
    """The first k whose fp32 running sum exceeds u, the last index if none does (the device heads' rule)."""
    cdf = np.cumsum(p.astype(np.float32), axis=-1, dtype=np.float32)
    hit = cdf > u[..., None]
    return np.where(hit.any(-1), hit.argmax(-1), p.shape[-1] - 1)


def test_midpoint_uniforms_reproduce_every_recorded_decision():
    g = np.load(FIXTURE)
    for s in range(STEPS):
        for name in ("fresh", "continued", "action"):
            p, k = g["s%d_%s_p" % (s, name)], g["s%d_%s" % (s, name)]
            u = midpoint_uniforms(p, k)
            assert np.array_equal(inv_cdf(p, u), k), (s, name)
            # and with room to spare: every uniform sits at least 5e-4 inside its interval
            cdf = np.cumsum(p.astype(np.float64), axis=-1)
            hi = np.take_along_axis(cdf, k[..., None], axis=-1)[..., 0]
            assert np.all(hi - u >= 4.9e-4), (s, name)
