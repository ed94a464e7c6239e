#!/usr/bin/env python
"""Generates tests/golden/option_critic/option_critic_pixel.npz by running the REFERENCE's own OptionCriticAgent.step
(OptionCritic_agent.py:52-119; the network / optimiser of examples.py:471-492) on OptionCriticNet(NatureConvBody(), 4,
num_options=4) over 4 synthetic Atari emulators (tests/fake_envs.PixelVectorTask), initial weights from fake_envs.numpy_params,
seeded torch / np.random: every Categorical.sample() the reference draws (fresh option, continued option, action per rollout step)
with its normalised probability row, and per rollout step q, beta, the chosen option's log pi row, option, prev_option, init,
action, entropy, reward, mask, ret, advantage, beta_advantage, eps; per agent step the loss, digests of the parameters after the
update and total_steps.  The option epsilon decays, the target network is re-synchronised inside the run and episodes end inside
it (done_period), so both option branches and (1 - init) matter.
Re-run:  python tests/golden/make_golden_option_critic.py        (needs the reference checkout; helpers come from make_golden.py)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from golden import make_golden as G  # noqa: E402  (loads the reference through tests/ref_shim.py)
from golden.make_golden_cases import digest  # noqa: E402
import fake_envs  # noqa: E402

ref = G.ref

# the setup the GPU test rebuilds (tests/test_gpu_option_critic_pixel.py)
N_ENVS, N_ACTIONS, N_OPTIONS, ENV_SEED, DONE_PERIOD = 4, 4, 4, 7, 6
PARAM_SEED, TORCH_SEED, STEPS, ROLLOUT = 31, 43, 4, 5
EPS = (0.6, 0.1, 200)             # LinearSchedule of the option epsilon: 0.6 -> 0.5 over the run, a new value every step
TARGET_FREQ = 3                   # total_steps // num_workers % 3 == 0: target syncs at rollout steps 3, 6, 9, ...
TERM_REG, ENT_W = 0.01, 0.01
MIN_WIDTH = 1e-3                  # every decision's probability interval
GAP_MIN = 1e-4                    # the top-two q gap of every row, relative to the q scale


def oc_shapes(n_actions, n_options):
    return fake_envs.NATURE_SHAPES + [("fc_q.weight", (n_options, 512)), ("fc_q.bias", (n_options,)),
                                      ("fc_pi.weight", (n_options * n_actions, 512)), ("fc_pi.bias", (n_options * n_actions,)),
                                      ("fc_beta.weight", (n_options, 512)), ("fc_beta.bias", (n_options,))]


def run():
    out = {}
    captured, restore = G._capture_storage("deep_rl.agent.OptionCritic_agent")
    draws = []
    orig_sample = torch.distributions.Categorical.sample

    def recording_sample(self, sample_shape=torch.Size()):
        v = orig_sample(self, sample_shape)
        draws.append((v.detach().numpy().copy(), self.probs.detach().numpy().astype(np.float32).copy()))
        return v

    torch.distributions.Categorical.sample = recording_sample
    try:
        cfg = G._cfg(discount=0.99, rollout_length=ROLLOUT, gradient_clip=5, num_workers=N_ENVS,
                     target_network_update_freq=TARGET_FREQ, termination_regularizer=TERM_REG, entropy_weight=ENT_W)
        cfg.state_normalizer, cfg.reward_normalizer = ref.ImageNormalizer(), ref.SignNormalizer()
        cfg.random_option_prob = ref.LinearSchedule(*EPS)
        p_np = fake_envs.numpy_params(oc_shapes(N_ACTIONS, N_OPTIONS), PARAM_SEED)
        agent = G._Obj()
        agent.config = cfg
        agent.task = fake_envs.PixelVectorTask(seed=ENV_SEED, num_envs=N_ENVS, done_period=DONE_PERIOD, n_actions=N_ACTIONS)
        agent.network = ref.OptionCriticNet(ref.NatureConvBody(), N_ACTIONS, num_options=N_OPTIONS)
        agent.network.load_state_dict({k: torch.from_numpy(v) for k, v in p_np.items()})
        agent.target_network = ref.OptionCriticNet(ref.NatureConvBody(), N_ACTIONS, num_options=N_OPTIONS)
        agent.target_network.load_state_dict(agent.network.state_dict())
        agent.optimizer = torch.optim.RMSprop(agent.network.parameters(), lr=1e-4, alpha=0.99, eps=1e-5)
        agent.total_steps = 0
        agent.worker_index = ref.tensor(np.arange(N_ENVS)).long()
        agent.states = cfg.state_normalizer(agent.task.reset())
        agent.is_initial_states = ref.tensor(np.ones(N_ENVS)).byte()
        agent.prev_options = agent.is_initial_states.clone().long()
        agent.sample_option = lambda *a: ref.OptionCriticAgent.sample_option(agent, *a)
        agent.record_online_return = lambda *a, **k: None
        torch.manual_seed(TORCH_SEED)
        np.random.seed(TORCH_SEED)
        for s in range(STEPS):
            del draws[:]
            ref.OptionCriticAgent.step(agent)
            st = captured[-1]
            k = "s%d_" % s
            assert len(draws) == 3 * ROLLOUT, len(draws)
            out[k + "fresh"] = np.stack([draws[3 * t][0] for t in range(ROLLOUT)]).astype(np.int64)
            out[k + "continued"] = np.stack([draws[3 * t + 1][0] for t in range(ROLLOUT)]).astype(np.int64)
            out[k + "fresh_p"] = np.stack([draws[3 * t][1] for t in range(ROLLOUT)])
            out[k + "continued_p"] = np.stack([draws[3 * t + 1][1] for t in range(ROLLOUT)])
            out[k + "action_p"] = np.stack([draws[3 * t + 2][1] for t in range(ROLLOUT)])
            out[k + "q"] = G._stack(st.q, ROLLOUT)
            out[k + "beta"] = G._stack(st.beta, ROLLOUT)
            out[k + "log_pi"] = G._stack(st.log_pi, ROLLOUT)
            out[k + "entropy"] = G._stack(st.entropy, ROLLOUT)[..., 0]
            for name in ("option", "prev_option", "action"):
                out[k + name] = G._stack(getattr(st, name), ROLLOUT)[..., 0].astype(np.int64)
            out[k + "init"] = G._stack(st.init_state, ROLLOUT)[..., 0]
            out[k + "reward"], out[k + "mask"] = G._stack(st.reward, ROLLOUT)[..., 0], G._stack(st.mask, ROLLOUT)[..., 0]
            out[k + "ret"] = G._stack(st.ret, ROLLOUT)[..., 0]
            out[k + "advantage"] = G._stack(st.advantage, ROLLOUT)[..., 0]
            out[k + "beta_advantage"] = G._stack(st.beta_advantage, ROLLOUT)[..., 0]
            out[k + "eps"] = np.asarray(st.eps[:ROLLOUT], dtype=np.float64)
            e = st.entries
            q_loss = (e.q.gather(1, e.option) - e.ret.detach()).pow(2).mul(0.5).mean()
            pi_loss = (-(e.log_pi.gather(1, e.action) * e.advantage.detach()) - ENT_W * e.entropy).mean()
            beta_loss = (e.beta.gather(1, e.prev_option) * e.beta_advantage.detach() * (1 - e.init_state)).mean()
            out[k + "loss"] = np.asarray([(pi_loss + q_loss + beta_loss).item(), q_loss.item(), pi_loss.item(), beta_loss.item()],
                                         dtype=np.float32)
            out[k + "total_steps"] = np.asarray(agent.total_steps)
            for name, v in agent.network.state_dict().items():
                out[k + "param_" + name] = digest(v.detach().numpy())
            for name, v in agent.target_network.state_dict().items():
                out[k + "target_" + name] = digest(v.detach().numpy())
            check(out, k)
        for name, v in p_np.items():
            out["init_" + name] = digest(v)
    finally:
        torch.distributions.Categorical.sample = orig_sample
        restore()
    branches(out)
    return out


def check(out, k):
    """Decisions a device implementation can reproduce from midpoint uniforms: every drawn category's probability interval is
    at least MIN_WIDTH wide, and no row's greedy option sits on a near tie."""
    for name in ("fresh", "continued", "action"):
        p, idx = out[k + name + "_p"], out[k + name]
        width = np.take_along_axis(p, idx[..., None], axis=-1)[..., 0]
        assert width.min() >= MIN_WIDTH, "%s%s: interval %g" % (k, name, width.min())
    q = out[k + "q"]
    scale = max(1.0, float(np.abs(q).max()))
    top2 = np.sort(q, axis=-1)[..., -2:]
    gap = top2[..., 1] - top2[..., 0]
    assert gap.min() > GAP_MIN * scale, "%s: near-tie greedy option (gap %g)" % (k, gap.min())


def branches(out):
    """Both option branches occur (init rows take the fresh draw, the others the continued one), at least one continued row
    switches away from its previous option, episodes end inside the run, and the epsilon decays."""
    cat = lambda name: np.concatenate([out["s%d_%s" % (s, name)].reshape(-1) for s in range(STEPS)])
    init, opt, prev, fresh, cont = cat("init"), cat("option"), cat("prev_option"), cat("fresh"), cat("continued")
    assert np.array_equal(opt, np.where(init > 0, fresh, cont))
    assert (init > 0).any() and (init == 0).any()
    assert ((init == 0) & (opt != prev)).any(), "no continued-then-switched option"
    assert ((init == 0) & (opt == prev)).any()
    assert (init[N_ENVS:] > 0).any(), "no episode ends inside the run"
    assert np.all(np.diff(cat("eps")) < 0)


def main():
    out_dir = os.path.join(os.environ.get("GOLDEN_OUT", HERE), "option_critic")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "option_critic_pixel.npz")
    np.savez_compressed(path, **run())
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
