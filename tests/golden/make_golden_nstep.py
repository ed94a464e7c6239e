#!/usr/bin/env python
"""Generates tests/golden/nstep/n_step_dqn_pixel.npz by running the REFERENCE's own NStepDQNAgent.step (NStepDQN_agent.py:25-67;
the network / optimiser of examples.py:427-447) on VanillaNet(NatureConvBody) over 4 synthetic Atari emulators
(tests/fake_envs.PixelVectorTask), initial weights from fake_envs.numpy_params, a seeded np.random: per agent step the rollout's q,
actions, rewards, masks, returns and loss, digests of the parameters after the update, and the np.random position.  The
epsilon schedule makes both random and greedy actions occur, and the target network is re-synchronised inside the run.
Re-run:  python tests/golden/make_golden_nstep.py        (needs the reference checkout; helpers come from make_golden.py)
"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from golden import make_golden as G  # noqa: E402  (loads the reference through tests/ref_shim.py)
from golden.make_golden_cases import digest  # noqa: E402
import fake_envs  # noqa: E402

ref = G.ref

# the setup the GPU test rebuilds (tests/test_gpu_nstep_dqn.py)
N_ENVS, N_ACTIONS, ENV_SEED, DONE_PERIOD = 4, 4, 7, 6
PARAM_SEED, NP_SEED, STEPS, ROLLOUT = 29, 41, 4, 5
EPS = (0.6, 0.1, 300)             # LinearSchedule(start, end, steps): about half the actions random at the start
TARGET_FREQ = 3                   # total_steps // num_workers % 3 == 0: target syncs at rollout steps 3, 6, 9, ...
GAP_MIN = 1e-4                    # a greedy row's top-two q gap, relative to the q scale


def rng_position():
    """np.random's state as (pos, crc32 of the key words): equal <=> the generator is at the same place."""
    _, key, pos, _, _ = np.random.get_state()
    return np.asarray([pos, zlib.crc32(np.ascontiguousarray(key).tobytes())], dtype=np.int64)


def run():
    out = {}
    captured, restore = G._capture_storage("deep_rl.agent.NStepDQN_agent")
    try:
        cfg = G._cfg(discount=0.99, rollout_length=ROLLOUT, gradient_clip=5, num_workers=N_ENVS,
                     target_network_update_freq=TARGET_FREQ)
        cfg.state_normalizer, cfg.reward_normalizer = ref.ImageNormalizer(), ref.SignNormalizer()
        cfg.random_action_prob = ref.LinearSchedule(*EPS)
        p_np = fake_envs.numpy_params(fake_envs.nature_vanilla_shapes(N_ACTIONS), PARAM_SEED)
        agent = G._Obj()
        agent.config = cfg
        agent.task = fake_envs.PixelVectorTask(seed=ENV_SEED, num_envs=N_ENVS, done_period=DONE_PERIOD, n_actions=N_ACTIONS)
        agent.network = ref.VanillaNet(N_ACTIONS, ref.NatureConvBody())
        agent.network.load_state_dict({k: torch.from_numpy(v) for k, v in p_np.items()})
        agent.target_network = ref.VanillaNet(N_ACTIONS, ref.NatureConvBody())
        agent.target_network.load_state_dict(agent.network.state_dict())
        agent.optimizer = torch.optim.RMSprop(agent.network.parameters(), lr=1e-4, alpha=0.99, eps=1e-5)
        agent.total_steps = 0
        agent.states = agent.task.reset()
        agent.record_online_return = lambda *a, **k: None
        np.random.seed(NP_SEED)
        n_random = n_greedy = 0
        for s in range(STEPS):
            eps_before = cfg.random_action_prob.current
            ref.NStepDQNAgent.step(agent)
            st = captured[-1]
            k = "s%d_" % s
            q = G._stack(st.q, ROLLOUT)
            action = G._stack(st.action, ROLLOUT)[..., 0]
            ret = G._stack(st.ret, ROLLOUT)
            out[k + "q"], out[k + "action"], out[k + "ret"] = q, action, ret
            out[k + "reward"], out[k + "mask"] = G._stack(st.reward, ROLLOUT), G._stack(st.mask, ROLLOUT)
            e = st.entries
            out[k + "loss"] = np.asarray(0.5 * (e.q.gather(1, e.action) - e.ret).pow(2).mean().item(), dtype=np.float32)
            out[k + "rng"] = rng_position()
            out[k + "total_steps"] = np.asarray(agent.total_steps)
            for name, v in agent.network.state_dict().items():
                out[k + "param_" + name] = digest(v.detach().numpy())
            for name, v in agent.target_network.state_dict().items():
                out[k + "target_" + name] = digest(v.detach().numpy())
            # greedy rows must not sit on a near tie (the device head's q agrees with the reference's to ~1e-6 of scale)
            scale = max(1.0, float(np.abs(q).max()))
            greedy = np.argmax(q, axis=-1)
            top2 = np.sort(q, axis=-1)[..., -2:]
            is_greedy = action == greedy
            gap = (top2[..., 1] - top2[..., 0])[is_greedy]
            assert gap.size == 0 or gap.min() > GAP_MIN * scale, "step %d: near-tie greedy row (gap %g)" % (s, gap.min())
            n_greedy += int(is_greedy.sum())
            n_random += int((~is_greedy).sum())
            out[k + "eps_before"] = np.asarray(eps_before)
        assert n_random > 0 and n_greedy > 0, (n_random, n_greedy)
        for name, v in p_np.items():
            out["init_" + name] = digest(v)
    finally:
        restore()
    return out


def main():
    out_dir = os.path.join(os.environ.get("GOLDEN_OUT", HERE), "nstep")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "n_step_dqn_pixel.npz")
    np.savez_compressed(path, **run())
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
