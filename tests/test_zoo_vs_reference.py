"""deeprl_amd/zoo.py (the example configurations as data) against the reference's own examples.py (CPU, no GPU work): each
reference entry point was executed through deeprl_amd.launch's loader with the agent constructor and run_steps replaced by a
capture, and the Config it built was recorded field by field (tests/golden/crosscheck.json, written by
tests/golden/make_golden_crosscheck.py); zoo.config(name) must describe the same.  Also: the launcher's loader / run_entry on
the package's own zoo file."""
import json

import numpy as np
import pytest

from golden import crosscheck_cases as C


@pytest.mark.parametrize("name", sorted(C.ZOO_GAMES))
def test_zoo_entry_equals_reference_example(name):
    import deeprl_amd as d
    from deeprl_amd import zoo
    with open(C.CROSSCHECK_JSON) as f:
        rec = json.load(f)["zoo"][name]
    d.select_device(-1)
    assert rec["agent"] == zoo.ZOO[name]["agent"]
    np.random.seed(0)
    want, have = rec["config"], C.describe_config(zoo.config(name, game=C.ZOO_GAMES[name]))
    assert set(want) == set(have), (sorted(set(want) ^ set(have)))
    for k in sorted(want):
        assert want[k] == have[k], "%s.%s: reference %s, zoo %s" % (name, k, want[k], have[k])


def test_launcher_runs_an_entry_with_capped_steps(tmp_path):
    """load_examples + run_entry on a deep_rl-style file: `async=` is rewritten, deep_rl resolves to the package, and
    max_steps reaches the agent's config before run_steps sees it."""
    import sys
    from deeprl_amd import launch
    saved = {k: v for k, v in sys.modules.items() if k == "deep_rl" or k.startswith("deep_rl.")}
    src = tmp_path / "my_examples.py"
    src.write_text("from deep_rl import *\n"
                   "class FakeAgent:\n"
                   "    def __init__(self, config):\n"
                   "        self.config, self.total_steps, self.closed = config, 0, False\n"
                   "        self.logger = type('L', (), {'info': lambda *a, **k: None})()\n"
                   "    def step(self):\n        self.total_steps += 1\n"
                   "    def switch_task(self):\n        pass\n"
                   "    def close(self):\n        self.closed = True\n"
                   "def entry(**kwargs):\n"
                   "    config = Config()\n    config.merge(kwargs)\n    config.max_steps = int(2e7)\n    config.log_interval = 0\n"
                   "    w = ReplayWrapper(UniformReplay, dict(memory_size=8, batch_size=2), async=True)\n"
                   "    assert w.async_ is True\n"
                   "    run_steps(FakeAgent(config))\n")
    try:
        mod = launch.load_examples(str(src))
        agent = launch.run_entry(mod, "entry", max_steps=37, game="x")
        assert agent.total_steps == 37 and agent.closed and agent.config.game == "x"
    finally:
        for k in [k for k in sys.modules if k == "deep_rl" or k.startswith("deep_rl.")]:
            del sys.modules[k]
        sys.modules.update(saved)
