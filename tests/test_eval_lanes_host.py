"""What the evaluation of seed lanes decides on the host, without a device: zoo.eval_points -- run_seeds(..., evaluate=True)'s
cadence -- against support.run_steps itself, driven by a counting fake agent; and the entries run_seeds refuses."""
import types

import pytest

# (max_steps, eval_interval, environment steps per agent step)
CADENCES = ((20, 5, 1),       # every step lands on total_steps: 0, 5, ..., 20
            (20, 5, 4),       # four steps at a time: the common multiples of 4 and 5 alone
            (21, 5, 4),       # max_steps is not landed on: the run stops at 24, which no evaluation sees
            (20, 6, 4),       # only common multiples of 4 and 6 trigger
            (20, 0, 4),       # an interval of 0 never triggers
            (0, 5, 4))        # evaluates once, at step 0, and stops
WANT = ([0, 5, 10, 15, 20], [0, 20], [0, 20], [0, 12], [], [0])


class _Stop(Exception):
    pass


class _Counting:
    """An agent that counts: step() advances total_steps by k, eval_episodes() records total_steps.  `budget`: the agent steps
    after which step() raises _Stop (support.run_steps reads max_steps 0 as 'no limit'; see the test)."""

    def __init__(self, max_steps, eval_interval, k, budget=None):
        self.config = types.SimpleNamespace(max_steps=max_steps, eval_interval=eval_interval, save_interval=0, log_interval=0, tag="t")
        self.logger = types.SimpleNamespace(info=lambda *a, **kw: None)
        self.total_steps, self.k, self.evaluated, self.closed, self.budget = 0, k, [], False, budget

    def step(self):
        if self.budget is not None:
            if self.budget == 0:
                raise _Stop()
            self.budget -= 1
        self.total_steps += self.k

    def eval_episodes(self):
        self.evaluated.append(self.total_steps)

    def switch_task(self):
        pass

    def close(self):
        self.closed = True


@pytest.mark.parametrize("cadence,want", list(zip(CADENCES, WANT)), ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else None)
def test_eval_points_are_run_steps_cadence(cadence, want):
    """zoo.eval_points(max_steps, eval_interval, k) is the list of total_steps at which support.run_steps calls eval_episodes() on
    an agent whose step() advances total_steps by k -- and the list written down here by hand.  max_steps 0: run_steps reads a
    falsy max_steps as 'no limit' and would not return, while run_seeds and eval_points read it as the bound it is; the fake agent
    then stops the driver at its first step(), and what run_steps evaluated up to there -- once, at step 0 -- is what is
    compared."""
    from deeprl_amd import zoo
    from deeprl_amd.support import run_steps
    max_steps, interval, k = cadence
    agent = _Counting(max_steps, interval, k, budget=None if max_steps else 0)
    if max_steps:
        run_steps(agent)
        assert agent.closed and agent.total_steps >= max_steps and agent.total_steps - k < max_steps
    else:
        with pytest.raises(_Stop):
            run_steps(agent)
        assert agent.total_steps == 0
    got = zoo.eval_points(max_steps, interval, k)
    assert got == agent.evaluated == want
    assert all(type(p) is int for p in got)


def test_run_seeds_with_evaluate_refuses_entries_without_lanes():
    """evaluate=True changes nothing about which entries have lanes: the ValueError is today's, ahead of any device work."""
    from deeprl_amd import zoo
    for name in ("rainbow_feature", "a2c_feature"):
        with pytest.raises(ValueError, match="only dqn_feature runs its seeds as lanes, %s has no lane form" % name):
            zoo.run_seeds(name, (1, 2), evaluate=True)


def test_batch_surface_names_the_evaluation_entries():
    """Every head names its evaluation lane entry, and the header declares it (so _lib binds it and build() checks the export)."""
    from deeprl_amd import _lib, seed_batch
    protos = _lib.parse_header()
    assert {cls.EVAL_LANES for cls in seed_batch.SEED_CLASSES.values()} == {"dra_dqn_mlp_eval_lanes", "dra_dist_mlp_eval_lanes"}
    for name in ("dra_dqn_mlp_eval_lanes", "dra_dist_mlp_eval_lanes"):
        assert len(protos[name]) == 4
    assert len(protos["dra_mlp_eval_lanes_supported"]) == 3
