"""config.fused_eval through the agents (DQNAgent.eval_episodes over dqn_mlp.Step.evaluate): for each of the four cart-pole replay
entries of the zoo the device evaluation against the host evaluation of the same agent with the switch off (the parent commit's
path) and against the fp64 restatement, that evaluation draws nothing and touches nothing, run_steps, the evaluation
environments that have to stay on the host, and save / load.

The agents carry tests/eval_cases.py's AGENT_CASES weights (numpy-seeded, chosen on the CPU under the margin condition) and an
evaluation environment of that module's seed and horizon; exploration_steps is 100, so the first 24 agent steps (96 transitions)
only act and the first evaluation runs on exactly those weights (rainbow_feature: and on the case's noise, planted in the online
network's buffers behind the last acting step).  Every device evaluation also asserts the margin condition on
what the kernel itself computed (the debug out_q)."""
import random

import numpy as np
import pytest
import torch
from feature_kernel_harness import GAME, dra, _Rec, _bits      # noqa: F401  (dra: the fixture)

import eval_cases as C
import eval_restatement as E

pytestmark = pytest.mark.gpu

SWITCHES = {"dqn_feature": dict(fused_dqn_feature=True), "categorical_dqn_feature": dict(fused_dist_feature=True),
            "quantile_regression_dqn_feature": dict(fused_dist_feature=True),
            "rainbow_feature": dict(fused_rainbow_feature=True, fused_rainbow_update=True)}
ENTRIES = tuple(SWITCHES)
EPISODES, EXPLORATION, ACT_STEPS, LEARN_STEPS, SEED = 3, 100, 24, 8, 21


def _agent(d, monkeypatch, entry, fused_eval, eval_env=None, **over):
    import deeprl_amd.agents as agents_mod
    from deeprl_amd import zoo
    rec = _Rec()
    monkeypatch.setattr(agents_mod, "get_logger", lambda *a, **k: rec)
    d.random_seed(SEED)
    torch.manual_seed(SEED)
    random.seed(SEED)
    c = zoo.config(entry, game=GAME, tag="eval_%s_%d" % (entry, fused_eval),
                   overrides=dict(eval_episodes=EPISODES, exploration_steps=EXPLORATION, fused_eval=fused_eval, **SWITCHES[entry], **over))
    c.task_fn = lambda: d.Task(GAME, seed=3, synthetic_done_period=C.HORIZON)
    c.eval_env = eval_env or d.Task(GAME, seed=C.ENV_SEED, synthetic_done_period=C.HORIZON)
    c.log_interval = 10 ** 9
    agent = getattr(d, zoo.ZOO[entry]["agent"])(c)
    assert agent._feature is not None, rec.warnings
    got = C.restated(C.AGENT_CASES[entry])
    with torch.no_grad():
        state = agent.network.state_dict()
        for k, v in got["params"].items():
            state[k].copy_(torch.from_numpy(v))
    agent.sync_target()
    np.random.seed(SEED)
    return agent, rec


def _plant_noise(agent, entry):
    """rainbow_feature: the case's raw noise into the online network's own buffers -- what evaluation runs under -- in place of
    the last acting step's draw (a learning step draws them anew)."""
    from deeprl_amd import rainbow_mlp
    import rainbow_feature_restatement as RR
    got = C.restated(C.AGENT_CASES[entry])
    if got["noise"] is None:
        return
    with torch.no_grad():
        for (_, m), layer in zip(rainbow_mlp.noisy_layers(agent.network), RR.LAYERS):
            for b in RR.NOISE:
                getattr(m, b).copy_(torch.from_numpy(got["noise"]["%s.%s" % (layer, b)]))
            m.noise_changed()
    assert agent.network.noise_block().intact()


def _watch(agent):
    """Every device evaluation of `agent` asserts the margin condition on the kernel's own q -> the list of (margin, bar)."""
    step, seen = agent._feature, []
    step.eval_debug_q = True
    evaluate = step.evaluate

    def checked(n):
        out = evaluate(n)
        q = step.eval_q.cpu().numpy().astype(np.float64)
        assert not np.isnan(q[:step.eval_steps]).any() and np.isnan(q[step.eval_steps:]).all()
        q = q[:step.eval_steps]
        margin, bar = float(np.abs(q[:, 1] - q[:, 0]).min()), E.Q_BAR * max(float(np.abs(q).max()), 1.0)
        print("device evaluation: margin %.3e, bar %.3e" % (margin, bar))
        assert margin >= E.MARGIN_BARS * bar
        seen.append((margin, bar))
        return out
    step.evaluate = checked
    return seen


def _ring_arrays(agent):
    torch.cuda.synchronize()
    rp = agent._inner_replay()
    frames, actions, rewards, masks = rp._ring.arrays()
    n = int(rp.size())          # the rows fed so far (the zoo's ring of 10^4 slots does not fill here; the rest was never written)
    assert n == agent.total_steps
    return dict(frames=frames.view(torch.float64).reshape(-1, 4)[:n].cpu().numpy(), actions=actions.view(torch.int64)[:n].cpu().numpy(),
                rewards=rewards[:n].cpu().numpy(), masks=masks[:n].cpu().numpy())


def _tests(rec):
    return [ln for ln in rec.lines if 'episodic_return_test' in ln]


def _run(d, monkeypatch, entry, fused_eval):
    agent, rec = _agent(d, monkeypatch, entry, fused_eval)
    step = agent._feature
    seen = _watch(agent) if fused_eval else []
    for _ in range(ACT_STEPS):
        agent.step()
    assert agent.total_steps == ACT_STEPS * step.k <= EXPLORATION
    _plant_noise(agent, entry)
    first = agent.eval_episodes()
    counts = (step.eval_launches, step.eval_copies, step.eval_steps)
    lengths = None if step.eval_lengths is None else step.eval_lengths.copy()
    for _ in range(LEARN_STEPS):
        agent.step()
    assert agent.total_steps > EXPLORATION
    torch.cuda.synchronize()
    out = dict(first=first, counts=counts, lengths=lengths, seen=list(seen), total=agent.total_steps, ring=_ring_arrays(agent),
               params={k: v.detach().cpu().numpy().copy() for k, v in agent.network.state_dict().items()},
               target={k: v.detach().cpu().numpy().copy() for k, v in agent.target_network.state_dict().items()},
               rng=np.random.randint(0, 1 << 30, size=3), pyrng=random.random(), torch_rng=torch.rand(3).numpy(),
               warnings=list(rec.warnings))
    out["second"] = agent.eval_episodes()       # on the weights the eight learning steps left
    out["lines"] = _tests(rec)
    out["on_device"] = step._eval_vec not in (None, False)
    agent.close()
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_device_evaluation_equals_host_evaluation_and_touches_nothing(dra, monkeypatch, entry):
    """Two agents from the same seed, config.fused_eval on and off.  After 24 acting steps eval_episodes() logs the same
    episodic_return_test line and returns the same mean -- the restatement's first three episodes --, with exactly one launch and
    one copy on the device side; after 8 more (learning) steps the two agents' parameters, target parameters, replay contents and
    the np.random / python random / torch tails are bit-equal: evaluation draws nothing and touches nothing; a second evaluation,
    on the learned weights, logs the same line again."""
    a, b = _run(dra, monkeypatch, entry, True), _run(dra, monkeypatch, entry, False)
    want = C.restated(C.AGENT_CASES[entry])["runs"]["five"]
    assert a["on_device"] and not b["on_device"] and a["warnings"] == b["warnings"] == []
    assert a["counts"][:2] == (1, 1) and b["counts"] == (0, 0, 0)
    assert list(a["lengths"]) == list(want["lengths"][:EPISODES]) and a["counts"][2] == int(want["lengths"][:EPISODES].sum())
    mean = want["returns"][:EPISODES].mean()
    assert a["first"] == b["first"] == {'episodic_return_test': mean}
    sem = want["returns"][:EPISODES].std() / np.sqrt(EPISODES)
    assert a["lines"][0] == b["lines"][0] == 'steps %d, episodic_return_test %.2f(%.2f)' % (ACT_STEPS * 4, mean, sem)
    assert len(a["seen"]) == 1 and a["total"] == b["total"]
    for k in a["params"]:
        assert np.array_equal(_bits(a["params"][k]), _bits(b["params"][k])), k
        assert np.array_equal(_bits(a["target"][k]), _bits(b["target"][k])), k
    for k in a["ring"]:
        assert np.array_equal(_bits(a["ring"][k]), _bits(b["ring"][k])), k
    assert np.array_equal(a["rng"], b["rng"]) and a["pyrng"] == b["pyrng"] and np.array_equal(a["torch_rng"], b["torch_rng"])
    assert a["second"] == b["second"] and a["lines"] == b["lines"] and len(a["lines"]) == 2


@pytest.mark.parametrize("entry", ("dqn_feature", "rainbow_feature"))
def test_run_steps_evaluates_at_the_same_steps(dra, monkeypatch, entry):
    """run_steps with eval_interval 16 over 64 steps: both agents evaluate at total_steps 0, 16, 32, 48 and 64 and log the same
    lines; the device side made one launch and one copy per evaluation."""
    from deeprl_amd.support import run_steps
    lines = {}
    for fused_eval in (True, False):
        agent, rec = _agent(dra, monkeypatch, entry, fused_eval, eval_interval=16, max_steps=64, save_interval=0)
        seen = _watch(agent) if fused_eval else []
        step = agent._feature
        run_steps(agent)
        lines[fused_eval] = _tests(rec)
        assert (step.eval_launches, step.eval_copies, len(seen)) == ((5, 5, 5) if fused_eval else (0, 0, 0))
    assert lines[True] == lines[False] and [int(ln.replace(',', '').split()[1]) for ln in lines[True]] == [0, 16, 32, 48, 64]


@pytest.mark.parametrize("why", ("stepped", "two_environments"))
def test_ineligible_evaluation_environment_stays_on_the_host(dra, monkeypatch, why):
    """An evaluation environment somebody has stepped, and a task of two environments: ONE warning names the reason, the host
    evaluation runs (the same record as with the switch off), no launch happens."""
    def env():
        task = dra.Task(GAME, num_envs=2 if why == "two_environments" else 1, seed=C.ENV_SEED, synthetic_done_period=C.HORIZON)
        if why == "stepped":
            task.reset()
            task.step([0])
        return task
    out = {}
    for fused_eval in (True, False):
        agent, rec = _agent(dra, monkeypatch, "dqn_feature", fused_eval, eval_env=env())
        first, second = agent.eval_episodes(), agent.eval_episodes()
        out[fused_eval] = (first, second, _tests(rec), list(rec.warnings))
        assert agent._feature.eval_launches == 0 and type(agent.config.eval_env) is dra.Task
        assert float(agent.eval_episode()) > 0
        agent.close()
    assert out[True][:3] == out[False][:3] and out[False][3] == []
    assert len(out[True][3]) == 1 and out[True][3][0].startswith("fused_eval is on but the evaluation environment stays on the host")
    assert ("already been stepped" if why == "stepped" else "not an envs.Task over one envs.CartPole") in out[True][3][0]


def test_save_load_continues_with_the_same_next_evaluation(dra, monkeypatch, tmp_path):
    """24 steps and an evaluation, save(); a fresh agent loads: its evaluation environment holds the saved arrays and its next
    evaluation -- and a single eval_episode() behind it -- are the first agent's.  A side file without the key loads as before."""
    first, _ = _agent(dra, monkeypatch, "dqn_feature", True)
    _watch(first)
    for _ in range(ACT_STEPS):
        first.step()
    first.eval_episodes()
    name = str(tmp_path / "ckpt")
    first.save(name)
    state = first._feature.state_dict()
    assert "eval_env" in state and int(state["eval_env"]["env_counter"][0]) == first._feature.eval_steps > 0
    second, rec2 = _agent(dra, monkeypatch, "dqn_feature", True)
    _watch(second)
    assert second._feature._eval_vec is None
    second.load(name)
    second.total_steps = first.total_steps
    a, b = first._feature._eval_vec, second._feature._eval_vec
    for key in ("env_state", "env_counter", "ep_steps", "ep_return", "env_seed"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert first.eval_episodes() == second.eval_episodes()
    assert first.eval_episode() == second.eval_episode()
    assert np.array_equal(first._feature.eval_lengths, second._feature.eval_lengths)
    assert torch.equal(a.env_state, b.env_state) and torch.equal(a.env_counter, b.env_counter)
    state.pop("eval_env")
    third, _ = _agent(dra, monkeypatch, "dqn_feature", True)
    third._feature.load_state_dict(state)
    assert third._feature._eval_vec is None
    for agent in (first, second, third):
        agent.close()
