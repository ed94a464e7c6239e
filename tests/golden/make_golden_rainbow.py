"""Records the Config the reference's own examples.py::rainbow_pixel builds (examples.py:283-336), field by field
(crosscheck_cases.describe_config), into tests/golden/rainbow/rainbow_pixel_config.json.  The agent class and run_steps are
replaced by a capture, as make_golden_crosscheck.py does for the other entries; nothing is trained.

  python tests/golden/make_golden_rainbow.py [output.json]

Needs the reference checkout (tests/ref_shim.py); tests/test_rainbow_host.py compares zoo.config('rainbow_pixel') with the
committed record and, where the reference is present, regenerates the record and compares the two."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GAME = "BreakoutNoFrameskip-v4"
OUT = os.path.join(HERE, "rainbow", "rainbow_pixel_config.json")


def main(out=OUT):
    import numpy as np
    import deeprl_amd as d
    from deeprl_amd import launch
    import ref_shim
    from golden import crosscheck_cases as C
    d.select_device(-1)
    mod = launch.load_examples(os.path.join(ref_shim.REFERENCE_ROOT, "examples.py"), "ref_examples_rainbow")
    got = {}
    for a in C.ZOO_AGENTS:
        setattr(mod, a, lambda cfg, _a=a: (_a, cfg))
    mod.run_steps = lambda pair: got.update(agent=pair[0], cfg=pair[1])
    mod.Config.NOISY_LAYER_STD = 0.1          # the class default; the entry point is what raises it
    np.random.seed(0)
    mod.rainbow_pixel(game=GAME)
    rec = dict(game=GAME, agent=got["agent"], noisy_layer_std=float(mod.Config.NOISY_LAYER_STD),
               config=C.describe_config(got["cfg"]))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return rec


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
