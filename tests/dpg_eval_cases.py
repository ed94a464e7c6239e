"""The cases of the DDPG / TD3 evaluation launch (csrc/dpg_mlp.hip dra_dpg_eval), shared by tests/test_dpg_eval_host.py (CPU) and
tests/test_gpu_dpg_eval.py: actor shapes, launches (episodes x horizon), the environment's seed and the junk a launch may start
from.  Parameters are dpg_env_cases.actor_params (fp32-representable, numpy-seeded)."""
import functools

import dpg_env_cases as K
import dpg_eval_restatement as E

# (S, A, H1, H2, gate): the pendulum's sizes over a small relu net, widths that are no multiple of 16 under tanh, the zoo's widths
SHAPES = [(3, 1, 32, 24, 1), (3, 1, 20, 12, 2), (3, 1, 400, 300, 1)]
# label -> (n_episodes, horizon, junk start): one row; a part of a tile; a full tile; a second workgroup with one live row; two
# workgroups, the second a quarter full; every step ends an episode; a non-zero counter with junk in the state and episode words
LAUNCHES = {"one": (1, 12, False), "five": (5, 12, False), "tile": (16, 3, False), "tile_and_one": (17, 3, False),
            "twenty": (20, 12, False), "every_step_ends": (5, 1, False), "junk_start": (5, 12, True)}
ZOO_LAUNCH = (20, 200)          # ddpg_continuous / td3_continuous: eval_episodes x the pendulum's horizon, at SHAPES[0] only
ENV_SEED, PARAM_SEED = 40, 11
JUNK = dict(counter=777, state=(0.75, -3.5), ep_steps=9, ep_return=-123.5)


def shape_id(shape):
    return "H%d_%d_g%d" % shape[2:5]


def make_env(junk, horizon):
    """The host evaluation environment of a launch as nobody has reset it: a fresh envs.Pendulum, or one whose counter, state and
    episode words hold JUNK (what reset() must not let survive)."""
    from deeprl_amd.envs import Pendulum
    import numpy as np
    env = Pendulum(ENV_SEED, horizon=horizon)
    if junk:
        env.c, env.steps, env.ret = JUNK["counter"], JUNK["ep_steps"], JUNK["ep_return"]
        env.s = np.asarray(JUNK["state"], dtype=np.float64)
    return env


def params(shape):
    return K.actor_params(shape, PARAM_SEED)


@functools.lru_cache(maxsize=None)
def restated(shape, label):
    """The fp64 restatement of a launch (computed once per process, shared, never modified)."""
    n, horizon, junk = LAUNCHES[label]
    return E.evaluate(E.actor_of(params(shape), shape[4]), make_env(junk, horizon), n)
