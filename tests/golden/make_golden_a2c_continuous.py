#!/usr/bin/env python
"""Generates tests/golden/a2c_continuous/ by running the REFERENCE's own code (tests/ref_shim.py):

  a2c_continuous_config.json   the Config examples.py::a2c_continuous builds (examples.py:384-404), field by field
                               (crosscheck_cases.describe_config); the agent class and run_steps are replaced by a capture, as
                               make_golden_crosscheck.py does for the other entries; nothing is trained
  a2c_continuous_step.npz      one A2CAgent.step (A2C_agent.py:22-64) on fake_envs.ContinuousTask with
                               GaussianActorCriticNet(actor_body=FCBody relu, critic_body=FCBody relu) and the entry's optimiser
                               and hyper-parameters, at two sizes: the normalised states, sampled actions, log_pi_a, entropy, v,
                               rewards, masks, advantages, returns, and the parameters before and after the update

Re-run:  python tests/golden/make_golden_a2c_continuous.py        (needs the reference checkout; GOLDEN_OUT redirects the output)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from golden import make_golden as G  # noqa: E402  (loads the reference through tests/ref_shim.py)
from golden import crosscheck_cases as C  # noqa: E402
import fake_envs  # noqa: E402
import ref_shim  # noqa: E402

ref = G.ref

GAME = "HalfCheetah-v2"
# tag, rollout length, environments, state_dim, action_dim, hidden, horizon and seed of the fake task
CASES = (("t5n16", 5, 16, 17, 6, 32, 6, 11), ("t3n2", 3, 2, 5, 2, 16, 2, 17))
LR, DISCOUNT, GAE_TAU, ENTROPY_WEIGHT, VALUE_LOSS_WEIGHT, GRADIENT_CLIP = 0.0007, 0.99, 1.0, 0.01, 1.0, 5


def gen_config():
    import deeprl_amd as d
    from deeprl_amd import launch
    d.select_device(-1)
    mod = launch.load_examples(os.path.join(ref_shim.REFERENCE_ROOT, "examples.py"), "ref_examples_a2c_continuous")
    got = {}
    for a in C.ZOO_AGENTS:
        setattr(mod, a, lambda cfg, _a=a: (_a, cfg))
    mod.run_steps = lambda pair: got.update(agent=pair[0], cfg=pair[1])
    np.random.seed(0)
    mod.a2c_continuous(game=GAME)
    return dict(game=GAME, agent=got["agent"], config=C.describe_config(got["cfg"]))


def gen_step():
    out = {}
    for tag, t_len, n_env, s_dim, a_dim, hidden, horizon, env_seed in CASES:
        captured, restore = G._capture_storage("deep_rl.agent.A2C_agent")
        try:
            cfg = G._cfg(discount=DISCOUNT, use_gae=True, gae_tau=GAE_TAU, entropy_weight=ENTROPY_WEIGHT, rollout_length=t_len,
                         gradient_clip=GRADIENT_CLIP, num_workers=n_env, value_loss_weight=VALUE_LOSS_WEIGHT)
            cfg.reward_normalizer = ref.RescaleNormalizer()
            agent = G._Obj()
            agent.config = cfg
            agent.task = fake_envs.ContinuousTask(seed=env_seed, state_dim=s_dim, action_dim=a_dim, horizon=horizon, num_envs=n_env)
            torch.manual_seed(5)
            agent.network = ref.GaussianActorCriticNet(s_dim, a_dim, actor_body=ref.FCBody(s_dim, hidden_units=(hidden, hidden)),
                                                       critic_body=ref.FCBody(s_dim, hidden_units=(hidden, hidden)))
            with torch.no_grad():       # (the heads start at 1e-3 scale and std at 0: move them so that every term matters)
                agent.network.fc_action.weight.mul_(300.0)
                agent.network.fc_critic.weight.mul_(300.0)
                agent.network.std.copy_(torch.linspace(-1.0, 1.5, a_dim))
            p_init = {k: v.detach().numpy().copy() for k, v in agent.network.state_dict().items()}
            agent.optimizer = torch.optim.RMSprop(agent.network.parameters(), lr=LR)
            agent.total_steps = 0
            agent.states = agent.task.reset()
            agent.record_online_return = lambda *a, **k: None
            seen_states = [np.asarray(agent.states).copy()]
            raw_step = agent.task.step

            def logging_step(actions, _raw=raw_step, _log=seen_states):
                o = _raw(actions)
                _log.append(np.asarray(o[0]).copy())
                return o

            agent.task.step = logging_step
            torch.manual_seed(35)  # action sampling stream
            ref.A2CAgent.step(agent)
            st = captured[0]
            k = tag + "_"
            out[k + "cfg"] = np.asarray([DISCOUNT, GAE_TAU, ENTROPY_WEIGHT, VALUE_LOSS_WEIGHT, GRADIENT_CLIP, LR, t_len, n_env,
                                         s_dim, a_dim, hidden])
            out[k + "reward"], out[k + "mask"] = G._stack(st.reward, t_len), G._stack(st.mask, t_len)
            out[k + "v"] = G._stack(st.v, t_len + 1)
            out[k + "log_pi_a"], out[k + "entropy"] = G._stack(st.log_pi_a, t_len), G._stack(st.entropy, t_len)
            out[k + "action"], out[k + "mean"] = G._stack(st.action, t_len), G._stack(st.mean, t_len)
            out[k + "adv"], out[k + "ret"] = G._stack(st.advantage, t_len), G._stack(st.ret, t_len)
            out[k + "states"] = np.stack(seen_states).astype(np.float32)  # [T+1, N, state_dim]: what tensor() hands the network
            assert (out[k + "mask"] == 0).any() and (out[k + "mask"] == 1).any(), tag
            for n, v in p_init.items():
                out[k + "init_" + n] = v
            for n, v in agent.network.state_dict().items():
                out[k + "final_" + n] = v.detach().numpy()
        finally:
            restore()
    return out


def main():
    out_dir = os.path.join(os.environ.get("GOLDEN_OUT", HERE), "a2c_continuous")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "a2c_continuous_config.json")
    with open(path, "w") as f:
        json.dump(gen_config(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % path)
    path = os.path.join(out_dir, "a2c_continuous_step.npz")
    np.savez_compressed(path, **gen_step())
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
