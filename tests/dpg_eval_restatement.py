"""Restatement of what the evaluation launch of csrc/dpg_mlp.hip (dra_dpg_eval) and _DeterministicPolicyAgent.eval_episodes under
config.fused_eval compute (TEST INFRASTRUCTURE ONLY): BaseAgent.py:60-77 over DummyVecEnv's auto reset -- reset, the action of the
float32 observation, step, reset on done -- over envs.Pendulum, which is imported, not restated.  The actor is a parameter:
`actor64` (dpg_env_cases: the fp64 forward over the narrowed observation) by default, any other act(obs) -> action where a test
plants a forward of its own.  `evaluate` is the host loop as it runs, episode after episode on ONE environment; `evaluate_rows` is the
kernel's form: episode e on an environment of its own whose counter starts at c0 + e horizon.  tests/test_dpg_eval_host.py pins the
two to each other bit for bit, and `evaluate` to BaseAgent.eval_episodes of the project's own agents and to the reference's
DDPGAgent.eval_episodes, before a GPU test leans on either."""
import numpy as np

import dpg_env_cases as K


def actor_of(params, gate):
    """act(obs) -> the fp64 action [1] of tanh(actor(float32(obs)))."""
    return lambda obs: K.actor64(params, obs, gate)


def episode(env, act):
    """One episode of `env` from reset() to done -> (return, states [horizon + 1][2], actions [horizon]); the environment is left
    behind its auto reset, as DummyVecEnv leaves it."""
    obs = env.reset()
    states, actions = [], []
    while True:
        states.append(np.asarray(env.s, dtype=np.float64).copy())
        a = np.asarray(act(obs)).reshape(-1)
        actions.append(a[0])
        obs, _, done, info = env.step(a)
        if done:
            states.append(np.asarray(env.s, dtype=np.float64).copy())
            ret = float(info['episodic_return'])
            env.reset()
            return ret, np.stack(states), np.asarray(actions)


def _leave(env, returns, states, actions):
    return dict(returns=np.asarray(returns, dtype=np.float64), states=np.stack(states), actions=np.stack(actions),
                steps=int(sum(len(a) for a in actions)), state=np.asarray(env.s, dtype=np.float64).copy(), counter=int(env.c),
                ep_steps=int(env.steps), ep_return=float(env.ret))


def evaluate(act, env, n_episodes):
    """n_episodes episodes of `env` (an envs.Pendulum) one after the other -> dict(returns [n] fp64, states [n][horizon + 1][2],
    actions [n][horizon], steps, and the environment's words afterwards: state, counter, ep_steps, ep_return)."""
    out = [episode(env, act) for _ in range(n_episodes)]
    return _leave(env, *zip(*out))


def evaluate_rows(act, seed, horizon, c0, n_episodes):
    """The same evaluation as n_episodes INDEPENDENT episodes: episode e on a fresh envs.Pendulum whose counter is c0 + e horizon;
    the environment afterwards is one more, reset at c0 + n_episodes horizon."""
    from deeprl_amd.envs import Pendulum
    out = []
    for e in range(n_episodes):
        env = Pendulum(seed, horizon=horizon)
        env.c = c0 + e * horizon
        out.append(episode(env, act))
    last = Pendulum(seed, horizon=horizon)
    last.c = c0 + n_episodes * horizon
    last.reset()
    return _leave(last, *zip(*out))
