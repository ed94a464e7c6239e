#!/usr/bin/env python
"""Generates tests/golden/crosscheck_dpg.json: the Config the reference's ddpg_continuous / td3_continuous entry points
(examples.py:554-617) build, recorded the way tests/golden/make_golden_crosscheck.py records the other entries -- the reference's
examples.py executed through deeprl_amd.launch's loader with the agent constructors and run_steps replaced by a capture --
and described by tests/golden/crosscheck_dpg_cases.py.

Re-run:  python tests/golden/make_golden_crosscheck_dpg.py   (needs the reference tree)
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402
from golden import crosscheck_cases as C  # noqa: E402
from golden import crosscheck_dpg_cases as D  # noqa: E402


def main():
    import deeprl_amd as d
    from deeprl_amd import launch
    saved = {k: v for k, v in sys.modules.items() if k == "deep_rl" or k.startswith("deep_rl.")}
    for k in list(saved):
        del sys.modules[k]
    d.select_device(-1)
    zoo = {}
    try:
        for name in sorted(D.DPG_GAMES):
            mod = launch.load_examples(os.path.join(ref_shim.REFERENCE_ROOT, "examples.py"), "ref_examples_dpg")
            got = {}
            for a in C.ZOO_AGENTS:
                setattr(mod, a, lambda cfg, _a=a: (_a, cfg))
            mod.run_steps = lambda pair: got.update(agent=pair[0], cfg=pair[1])
            np.random.seed(0)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                getattr(mod, name)(game=D.DPG_GAMES[name])
                zoo[name] = {"agent": got["agent"], "config": D.describe_dpg_config(got["cfg"])}
    finally:
        for k in [k for k in sys.modules if k == "deep_rl" or k.startswith("deep_rl.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    C.dump_json({"zoo": zoo}, D.CROSSCHECK_DPG_JSON)
    print("wrote %s (%.1f KB)" % (D.CROSSCHECK_DPG_JSON, os.path.getsize(D.CROSSCHECK_DPG_JSON) / 1024.0))


if __name__ == "__main__":
    main()
