"""Closed loop: zoo.ddpg_continuous / td3_continuous on 'classic-Pendulum-v0' over the device path (config.fused_dpg_env with
fused_dpg_update, warm_up = 1000) must learn what the reference's own agents learn on the same environment.
tests/golden/dpg_pendulum/learning_reference.json (tests/golden/make_golden_dpg_pendulum.py --learning) holds the random policy's
mean and standard deviation of episode return, the reference's median last-10-episode return over five seeds at 5 000 ... 20 000
steps, `n_learn` -- the first of those step counts at which its gain over the random mean is at least 2 random-policy standard
deviations -- and the bar: the random mean plus half of that gain.  The device path runs n_learn steps under three seeds; the median
of its last-10-episode returns must reach the bar."""
import json
import os

import numpy as np
import pytest
from parity_log import record_parity

from feature_kernel_harness import _Rec, dra  # noqa: F401

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dpg_pendulum", "learning_reference.json")) as _f:
    REF = json.load(_f)
LEARNERS = [a for a in ("ddpg", "td3") if REF[a]["n_learn"] is not None]
SEEDS = (1, 2, 3)


@pytest.mark.parametrize("algo", LEARNERS)
def test_closed_loop_learns(dra, monkeypatch, algo):  # noqa: F811
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: _Rec())
    ref, rnd = REF[algo], REF["random"]
    finals = []
    for seed in SEEDS:
        dra.random_seed(seed)
        agent = zoo.agent(algo + "_continuous", game=REF["game"],
                          overrides=dict(warm_up=REF["warm_up"], fused_dpg_update=True, fused_dpg_env=True))
        assert agent._fused_env() is not None
        for _ in range(ref["n_learn"]):
            agent.step()
        rets = [r for _, r in agent.episodes()]
        agent.close()
        assert len(rets) == ref["n_learn"] // 200
        finals.append(float(np.mean(rets[-REF["last_episodes"]:])))
    median = float(np.median(finals))
    print("%s: last-%d-episode returns %s, median %.1f; bar %.1f (random %.1f +- %.1f, reference median %.1f at %d steps)"
          % (algo, REF["last_episodes"], ["%.1f" % f for f in finals], median, ref["bar"], rnd["mean"], rnd["std"],
             ref["median"][REF["checkpoints"].index(ref["n_learn"])], ref["n_learn"]))
    record_parity("dpg_env_closed_loop_%s" % algo, median_return=median, bar=ref["bar"])
    assert median >= ref["bar"]
