#!/usr/bin/env python
"""Agent-level throughput of the other BASELINE.json configs on one MI355X (parity cases, not the bench line):
every agent is built exactly like the reference's examples.py factory it cites, on the synthetic `Task`
environments (CPU numpy emulators stand-ins, like the reference's DummyVecEnv), and `agent.step()` is timed
after a warm-up.  Prints one JSON object per line: agent steps/s, env steps/s, gradient updates/s.

  config 3  ppo_continuous  examples.py:497-523  (HalfCheetah shapes; 1 worker as in the reference, and 16 workers)
  config 2  dqn_pixel examples.py:55-97 through the agent API with a HOST emulator (fused learner attached by
            DQNAgent; `_generic` = config.fused_learner False, the autograd path the other agents use)
  config 4  dqn_pixel + PrioritizedReplay (examples.py:55-97 with replay_cls=PrioritizedReplay),
            categorical_dqn_pixel examples.py:195-226, quantile_regression_dqn_pixel examples.py:129-160
            rainbow_pixel examples.py:283-336 (PER + double Q + noisy dueling C51; `_modules` = config.fused_noisy False and
            config.graph_update False: materialised noisy weights through the plain GEMM, eager launches)
  config 5  a2c_pixel examples.py:361-381 (16 workers), ppo_pixel examples.py:525-550 (8 workers)
            a2c_continuous examples.py:384-404 (16 workers; `_host` = config.device_env False: python environments, module head)
            a2c_feature examples.py:340-358 (5 workers, classic-CartPole-v0; `_host` = config.device_env False: python
            environments, one module forward per step)
            n_step_dqn_pixel examples.py:427-447 (16 workers), option_critic_pixel examples.py:471-492 (16 workers)
            n_step_dqn_feature examples.py:408-424 (5 workers, classic-CartPole-v0, config.fused_nstep_feature True;
            `_module_update` = config.fused_nstep_update False; `_host` = the switch off: python environments)
            option_critic_feature examples.py:450-468 (5 workers, classic-CartPole-v0, config.fused_oc_feature True;
            `_module_update` = config.fused_oc_update False; `_host` = the switch off: python environments)
  config 1  dqn_feature examples.py:11-52 (one classic-CartPole-v0 environment, config.fused_dqn_feature True;
            `_module_update` = config.fused_dqn_update False; `_host` = the switch off: the python environment and ring feeds)
            dqn_feature_per / dqn_feature_nstep: the same entry with n_step 3 over a PrioritizedReplay / a UniformReplay
            (config.fused_dqn_replay_feature True and config.fused_dqn_replay_update True; `_module_update` =
            config.fused_dqn_replay_update False; `_host` = the switch off)
            categorical_dqn_feature examples.py:164-193, quantile_regression_dqn_feature examples.py:101-127 (the same, with
            config.fused_dist_feature True and config.fused_dist_update True; `_module_update` = config.fused_dist_update False; `_host` = the switch off)
            rainbow_feature examples.py:231-280 (noisy RainbowNet, 50 atoms, n_step 3, PrioritizedReplay, double_q, minibatch 32;
            config.fused_rainbow_feature True and config.fused_rainbow_update True; `_module_update` = config.fused_rainbow_update
            False; `_host` = the switch off)
  ddpg_continuous examples.py:554-583, td3_continuous examples.py:587-617 (one host environment, (400, 300) relu MLPs, Adam 1e-3,
            minibatch 100, a 1M ring; warm_up shortened to 1000 so that the timed window is all updates; the default is
            config.fused_dpg_update True: csrc/dpg_mlp.hip; `_modules` = the switch off: torch modules and optimisers)

Evaluation (config.fused_eval, csrc/eval_act.h) is timed by cases of its own, named explicitly with --cases (EVAL_CASES):
  <entry>_eval  for the four cart-pole replay entries: ONE agent on its device path, past its warm-up; eval_episodes() with
            config.fused_eval off (the host loop: the parent's path) and on (one launch, one copy), three timed calls each behind an
            untimed one, as microseconds per evaluated environment step (host: the environment's own step counter; device:
            out_steps), min-max over the calls
  dqn_feature_run_steps_eval  run_steps of dqn_feature over 25 000 steps (evaluations at 0, 5 000, ..., 25 000), the same seed with
            the switch off and on, three runs each: wall time and the share of it spent inside eval_episodes()
  ddpg_continuous_eval, td3_continuous_eval  the same for the two continuous entries on classic-Pendulum-v0 (fused_dpg_update and
            fused_dpg_env on, (400, 300) networks, 1 500 agent steps of training): eval_episodes() of 20 x 200 steps, the host loop
            against the one launch of csrc/dpg_mlp.hip's dra_dpg_eval
  ddpg_pendulum_run_steps_eval  run_steps of the zoo's ddpg_continuous on the pendulum over 20 000 steps (evaluations at 0, 10 000 and
            20 000), the same seed with the switch off and on, three runs each

Seed lanes (deeprl_amd/seed_batch.py), named explicitly with --cases too (SEED_CASES):
  dqn_feature_seeds1 / 4 / 16 / 64  the dqn_feature case's configuration once per seed, the seeds as lanes of the same launches;
            env_steps_per_s is the aggregate over the lanes, prepare_us_per_lane_step the host's draws and staging per lane and agent
            step (time.perf_counter around DQNFeatureSeeds.prepare)
  categorical_dqn_feature_seeds1 / 4 / 16, quantile_regression_dqn_feature_seeds1 / 4 / 16  the same over the two distributional cases
            (the lanes always run the update kernel: their single baselines are categorical_dqn_feature -- and its faster single form,
            categorical_dqn_feature_module_update -- and quantile_regression_dqn_feature)
  <a seeds case>_device_draws (SEED_DRAW_CASES: dqn_feature 1 / 4 / 16 / 64, the distributional two 4 / 16)  the same lanes with
            device_draws=True: prepare_us_per_lane_step is then the common block and the counters alone
  dqn_feature_nstep_seeds1 / 4 / 16 / 64, and each with _device_draws  the dqn_feature_nstep case's configuration (n_step 3 over a
            UniformReplay, config.fused_dqn_replay_feature) once per seed as lanes (seed_batch.DQNReplayFeatureSeeds); the single
            baseline is dqn_feature_nstep
  <a seeds case>_eval (SEED_EVAL_CASES: dqn_feature 1 / 4 / 16 / 64, the distributional two 1 / 4 / 16)  the lanes built with
            eval_lanes=True and trained for 5 000 agent steps (20 000 environment steps per lane); then eval_episodes = 10 of every
            lane as ONE launch and one copy (batch.evaluate) against the alternative that needs no lane kernel, a loop over the lanes
            of the single launch (each lane Step's own evaluate: one launch and one synchronising copy per lane).  Three alternating
            repeats from the same start of the evaluation environments each, the returns required equal to the bit; microseconds
            per evaluation (all lanes), min-max over the repeats
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deeprl_amd as d  # noqa: E402
import deeprl_amd.agents as agents_mod  # noqa: E402
from deeprl_amd import zoo  # noqa: E402


class _Quiet:
    def info(self, *a, **k):
        pass

    def add_scalar(self, *a, **k):
        pass

    def add_histogram(self, *a, **k):
        pass


def dqn_family(kind, replay_cls, ring=200_000, fused=True, device=False, async_actor=None, **switches):
    c = d.Config()
    c.merge(dict(game="synthetic-atari", log_level=0, tag="bench", n_step=1, replay_cls=replay_cls, async_replay=False,
                 fused_learner=fused, device_env=device, **switches))     # device=False: HOST emulator; True: device-resident environment
    c.task_fn = lambda: d.Task(c.game, seed=1)
    c.eval_env = c.task_fn()
    if kind == "dqn":
        c.optimizer_fn = lambda p: torch.optim.RMSprop(p, lr=0.00025, alpha=0.95, eps=0.01, centered=True)
        c.network_fn = lambda: d.VanillaNet(c.action_dim, d.NatureConvBody(in_channels=4))
        c.gradient_clip = 5
        agent_cls = d.DQNAgent
    elif kind == "c51":
        c.optimizer_fn = lambda p: torch.optim.Adam(p, lr=0.00025, eps=0.01 / 32)
        c.categorical_v_max, c.categorical_v_min, c.categorical_n_atoms = 10, -10, 51
        c.network_fn = lambda: d.CategoricalNet(c.action_dim, c.categorical_n_atoms, d.NatureConvBody())
        c.gradient_clip = 0.5
        agent_cls = d.CategoricalDQNAgent
    elif kind == "rainbow":
        d.Config.NOISY_LAYER_STD = 0.5
        c.noisy_linear = True
        c.optimizer_fn = lambda p: torch.optim.Adam(p, lr=0.000625, eps=1.5e-4)
        c.categorical_v_max, c.categorical_v_min, c.categorical_n_atoms = 10, -10, 51
        c.network_fn = lambda: d.RainbowNet(c.action_dim, c.categorical_n_atoms, d.NatureConvBody(noisy_linear=True),
                                            noisy_linear=True)
        c.gradient_clip = 10
        agent_cls = d.CategoricalDQNAgent
    else:
        c.optimizer_fn = lambda p: torch.optim.Adam(p, lr=0.00005, eps=0.01 / 32)
        c.num_quantiles = 200
        c.network_fn = lambda: d.QuantileNet(c.action_dim, c.num_quantiles, d.NatureConvBody())
        c.gradient_clip = 5
        agent_cls = d.QuantileRegressionDQNAgent
    c.random_action_prob = d.LinearSchedule(1.0, 0.01, 1e6)
    c.batch_size = 32
    c.discount = 0.99
    c.history_length = 4
    kw = dict(memory_size=ring, batch_size=c.batch_size, n_step=c.n_step, discount=c.discount, history_length=4)
    c.replay_fn = lambda: d.ReplayWrapper(c.replay_cls, kw, c.async_replay)
    c.replay_eps, c.replay_alpha = 0.01, 0.5
    c.replay_beta = d.LinearSchedule(0.4, 1.0, 2e7)
    c.state_normalizer = d.ImageNormalizer()
    c.reward_normalizer = d.SignNormalizer()
    c.target_network_update_freq = 10000
    c.exploration_steps = 300          # the update phase is what is timed
    c.sgd_update_frequency = 4
    c.double_q = kind == "rainbow"
    c.async_actor = bool(device) if async_actor is None else bool(async_actor)   # the reference's default for the pixel DQN family
    c.max_steps = int(2e7)
    return agent_cls(c), dict(env_per_step=4, updates_per_step=1)


def a2c_pixel(workers=16, device=True, **switches):
    c = d.Config()
    c.merge(dict(game="BreakoutNoFrameskip-v4", log_level=0, tag="bench", device_env=device, **switches))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, lr=1e-4, alpha=0.99, eps=1e-5)
    c.network_fn = lambda: d.CategoricalActorCriticNet(c.state_dim, c.action_dim, d.NatureConvBody())
    c.state_normalizer = d.ImageNormalizer()
    c.reward_normalizer = d.SignNormalizer()
    c.discount, c.use_gae, c.gae_tau, c.entropy_weight, c.rollout_length, c.gradient_clip = 0.99, True, 1.0, 0.01, 5, 5
    c.max_steps = int(2e7)
    return d.A2CAgent(c), dict(env_per_step=5 * workers, updates_per_step=1)


def a2c_continuous(workers=16, device=True, **switches):
    c = d.Config()
    c.merge(dict(game="synthetic-continuous-HalfCheetah", log_level=0, tag="bench", device_env=device, **switches))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, lr=0.0007)
    c.network_fn = lambda: d.GaussianActorCriticNet(c.state_dim, c.action_dim, actor_body=d.FCBody(c.state_dim),
                                                    critic_body=d.FCBody(c.state_dim))
    c.discount, c.use_gae, c.gae_tau, c.entropy_weight, c.rollout_length, c.gradient_clip = 0.99, True, 1.0, 0.01, 5, 5
    c.max_steps = int(2e7)
    return d.A2CAgent(c), dict(env_per_step=5 * workers, updates_per_step=1)


def a2c_feature(workers=5, device=True, **switches):
    import torch.nn.functional as F
    c = d.Config()
    c.merge(dict(game="classic-CartPole-v0", log_level=0, tag="bench", device_env=device, **switches))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, 0.001)
    c.network_fn = lambda: d.CategoricalActorCriticNet(c.state_dim, c.action_dim, d.FCBody(c.state_dim, gate=F.tanh))
    c.discount, c.use_gae, c.gae_tau, c.entropy_weight, c.rollout_length, c.gradient_clip = 0.99, True, 0.95, 0.01, 5, 0.5
    return d.A2CAgent(c), dict(env_per_step=5 * workers, updates_per_step=1)


def dpg_continuous(kind, fused=True, game="synthetic-continuous-HalfCheetah", device=False):
    """device: config.fused_dpg_env -- the environment on the device, one acting launch per transition (csrc/dpg_mlp.hip
    dra_dpg_env_act); game 'classic-Pendulum-v0': envs.Pendulum, the family's learning check."""
    c = d.Config()
    c.merge(dict(game=game, log_level=0, tag="bench", fused_dpg_update=fused, fused_dpg_env=device))
    c.task_fn = lambda: d.Task(c.game, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    adam = lambda p: torch.optim.Adam(p, lr=1e-3)
    body = lambda n: d.FCBody(n, (400, 300), gate=torch.relu)
    if kind == "ddpg":
        c.network_fn = lambda: d.DeterministicActorCriticNet(c.state_dim, c.action_dim, actor_body=body(c.state_dim),
                                                             critic_body=body(c.state_dim + c.action_dim), actor_opt_fn=adam,
                                                             critic_opt_fn=adam)
        c.replay_fn = lambda: d.UniformReplay(memory_size=int(1e6), batch_size=100)
        c.random_process_fn = lambda: d.OrnsteinUhlenbeckProcess(size=(c.action_dim,), std=d.LinearSchedule(0.2))
    else:
        c.network_fn = lambda: d.TD3Net(c.action_dim, actor_body_fn=lambda: body(c.state_dim),
                                        critic_body_fn=lambda: body(c.state_dim + c.action_dim), actor_opt_fn=adam, critic_opt_fn=adam)
        c.replay_fn = lambda: d.ReplayWrapper(d.UniformReplay, dict(memory_size=int(1e6), batch_size=100))
        c.random_process_fn = lambda: d.GaussianProcess(size=(c.action_dim,), std=d.LinearSchedule(0.1))
        c.td3_noise, c.td3_noise_clip, c.td3_delay = 0.2, 0.5, 2
    c.discount, c.warm_up, c.target_network_mix, c.max_steps = 0.99, 1000, 5e-3, int(1e6)
    agent = (d.DDPGAgent if kind == "ddpg" else d.TD3Agent)(c)
    return agent, dict(env_per_step=1, updates_per_step=1, warm=1100)


def n_step_dqn_pixel(workers=16, device=True, **switches):
    c = d.Config()
    c.merge(dict(game="BreakoutNoFrameskip-v4", log_level=0, tag="bench", device_env=device, **switches))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, lr=1e-4, alpha=0.99, eps=1e-5)
    c.network_fn = lambda: d.VanillaNet(c.action_dim, d.NatureConvBody())
    c.random_action_prob = d.LinearSchedule(1.0, 0.05, 1e6)
    c.state_normalizer = d.ImageNormalizer()
    c.reward_normalizer = d.SignNormalizer()
    c.discount, c.target_network_update_freq, c.rollout_length, c.gradient_clip = 0.99, 10000, 5, 5
    c.max_steps = int(2e7)
    return d.NStepDQNAgent(c), dict(env_per_step=5 * workers, updates_per_step=1)


def n_step_dqn_feature(workers=5, **switches):
    c = d.Config()
    c.merge(dict(game="classic-CartPole-v0", log_level=0, tag="bench", **switches))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, 0.001)
    c.network_fn = lambda: d.VanillaNet(c.action_dim, d.FCBody(c.state_dim))
    c.random_action_prob = d.LinearSchedule(1.0, 0.1, 1e4)
    c.discount, c.target_network_update_freq, c.rollout_length, c.gradient_clip = 0.99, 200, 5, 5
    return d.NStepDQNAgent(c), dict(env_per_step=5 * workers, updates_per_step=1)


def dqn_feature(**switches):
    return d.DQNAgent(dqn_feature_config(**switches)), dict(env_per_step=4, updates_per_step=1, warm=300)


def dqn_feature_seeds(n, device_draws=False, eval_lanes=False):
    """dqn_feature_seedsN: N seeds of the dqn_feature case as lanes of the same launches (deeprl_amd/seed_batch.py), the
    environments seeded 1 .. N; env_steps_per_s is the AGGREGATE over the lanes.  device_draws: the lanes' np.random draws taken
    by dra_np_mt_draw_lanes (the _device_draws cases)."""
    from deeprl_amd.seed_batch import DQNFeatureSeeds
    batch = DQNFeatureSeeds(lambda seed: dqn_feature_config(task_seed=seed), range(1, n + 1), device_draws=device_draws,
                            eval_lanes=eval_lanes)
    return batch, dict(env_per_step=4 * n, updates_per_step=n, warm=300, lanes=n)


def dqn_feature_nstep_seeds(n, device_draws=False):
    """dqn_feature_nstep_seedsN: N seeds of the dqn_feature_nstep case (n_step 3) as lanes of the same launches
    (seed_batch.DQNReplayFeatureSeeds: the batch sets fused_dqn_replay_feature), as dqn_feature_seeds."""
    from deeprl_amd.seed_batch import DQNReplayFeatureSeeds
    batch = DQNReplayFeatureSeeds(lambda seed: dqn_feature_config(task_seed=seed, n_step=3, fused_dqn_replay_update=True), range(1, n + 1),
                                  device_draws=device_draws)
    return batch, dict(env_per_step=4 * n, updates_per_step=n, warm=300, lanes=n)


def dqn_feature_config(task_seed=1, **switches):
    c = d.Config()
    # (switches may name the entry's own replay options too: n_step, replay_cls -- the dqn_feature_per / _nstep cases)
    c.merge(dict(dict(game="classic-CartPole-v0", log_level=0, tag="bench", n_step=1, replay_cls=d.UniformReplay, async_replay=False),
                 **switches))
    c.task_fn = lambda: d.Task(c.game, seed=task_seed)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, 0.001)
    c.network_fn = lambda: d.VanillaNet(c.action_dim, d.FCBody(c.state_dim))
    c.history_length, c.batch_size, c.discount = 1, 10, 0.99
    kw = dict(memory_size=int(1e4), batch_size=c.batch_size, n_step=c.n_step, discount=c.discount, history_length=1)
    c.replay_fn = lambda: d.ReplayWrapper(c.replay_cls, kw, c.async_replay)
    c.replay_eps, c.replay_alpha, c.replay_beta = 0.01, 0.5, d.LinearSchedule(0.4, 1.0, 1e5)      # (examples.py:39-41)
    c.random_action_prob = d.LinearSchedule(1.0, 0.1, 1e4)
    c.target_network_update_freq, c.exploration_steps, c.double_q = 200, 1000, False
    c.sgd_update_frequency, c.gradient_clip, c.async_actor = 4, 5, False
    # (warm, in dqn_feature(): past exploration_steps -- 250 agent steps -- and the graph captures, so that the timed window is all
    # updates)
    return c


def dist_feature(head, **switches):
    cls = d.CategoricalDQNAgent if head == "categorical" else d.QuantileRegressionDQNAgent
    # (warm: past exploration_steps -- 25 agent steps -- and the graph captures, so that the timed window is all updates)
    return cls(dist_feature_config(head, **switches)), dict(env_per_step=4, updates_per_step=1, warm=120)


def dist_feature_seeds(head, n, device_draws=False, eval_lanes=False):
    """categorical_dqn_feature_seedsN / quantile_regression_dqn_feature_seedsN: N seeds of the dist_feature case as lanes of the same
    launches (deeprl_amd/seed_batch.py: the batch sets fused_dist_feature and fused_dist_update), the environments seeded 1 .. N;
    env_steps_per_s is the AGGREGATE over the lanes."""
    from deeprl_amd import seed_batch
    cls = seed_batch.CategoricalDQNFeatureSeeds if head == "categorical" else seed_batch.QuantileRegressionDQNFeatureSeeds
    batch = cls(lambda seed: dist_feature_config(head, task_seed=seed), range(1, n + 1), device_draws=device_draws, eval_lanes=eval_lanes)
    return batch, dict(env_per_step=4 * n, updates_per_step=n, warm=120, lanes=n)


def dist_feature_config(head, task_seed=1, **switches):
    c = d.Config()
    c.merge(dict(game="classic-CartPole-v0", log_level=0, tag="bench", **switches))
    c.task_fn = lambda: d.Task(c.game, seed=task_seed)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, 0.001)
    if head == "categorical":
        c.categorical_v_max, c.categorical_v_min, c.categorical_n_atoms = 100, -100, 50
        c.network_fn = lambda: d.CategoricalNet(c.action_dim, c.categorical_n_atoms, d.FCBody(c.state_dim))
    else:
        c.num_quantiles = 20
        c.network_fn = lambda: d.QuantileNet(c.action_dim, c.num_quantiles, d.FCBody(c.state_dim))
    c.batch_size, c.discount = 10, 0.99
    kw = dict(memory_size=int(1e4), batch_size=c.batch_size)
    c.replay_fn = lambda: d.ReplayWrapper(d.UniformReplay, kw, False)
    c.random_action_prob = d.LinearSchedule(1.0, 0.1, 1e4)
    c.target_network_update_freq, c.exploration_steps = 200, 100
    c.sgd_update_frequency, c.gradient_clip = 4, 5
    return c


def rainbow_feature(**switches):
    agent = zoo.agent("rainbow_feature", game="classic-CartPole-v0", tag="bench", async_replay=False, **switches)
    # (warm: past exploration_steps -- 250 agent steps -- and the graph captures, so that the timed window is all updates)
    return agent, dict(env_per_step=4, updates_per_step=1, warm=300)


def option_critic_pixel(workers=16, device=True, **switches):
    c = d.Config()
    c.merge(dict(game="BreakoutNoFrameskip-v4", log_level=0, tag="bench", device_env=device, **switches))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, lr=1e-4, alpha=0.99, eps=1e-5)
    c.network_fn = lambda: d.OptionCriticNet(d.NatureConvBody(), c.action_dim, num_options=4)
    c.random_option_prob = d.LinearSchedule(0.1)
    c.state_normalizer = d.ImageNormalizer()
    c.reward_normalizer = d.SignNormalizer()
    c.discount, c.target_network_update_freq, c.rollout_length, c.gradient_clip = 0.99, 10000, 5, 5
    c.entropy_weight, c.termination_regularizer = 0.01, 0.01
    c.max_steps = int(2e7)
    return d.OptionCriticAgent(c), dict(env_per_step=5 * workers, updates_per_step=1)


def option_critic_feature(workers=5, **switches):
    c = d.Config()
    c.merge(dict(game="classic-CartPole-v0", log_level=0, tag="bench", **switches))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.RMSprop(p, 0.001)
    c.network_fn = lambda: d.OptionCriticNet(d.FCBody(c.state_dim), c.action_dim, num_options=2)
    c.random_option_prob = d.LinearSchedule(1.0, 0.1, 1e4)
    c.discount, c.target_network_update_freq, c.rollout_length, c.gradient_clip = 0.99, 200, 5, 5
    c.termination_regularizer, c.entropy_weight = 0.01, 0.01
    return d.OptionCriticAgent(c), dict(env_per_step=5 * workers, updates_per_step=1)


def ppo_continuous(workers=1, device=True, fused=True):
    c = d.Config()
    c.merge(dict(game="synthetic-continuous-HalfCheetah", log_level=0, tag="bench", device_env=device, fused_ppo_mlp=fused))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.network_fn = lambda: d.GaussianActorCriticNet(c.state_dim, c.action_dim, actor_body=d.FCBody(c.state_dim, gate=torch.tanh),
                                                    critic_body=d.FCBody(c.state_dim, gate=torch.tanh))
    c.actor_opt_fn = lambda p: torch.optim.Adam(p, 3e-4)
    c.critic_opt_fn = lambda p: torch.optim.Adam(p, 1e-3)
    c.discount, c.use_gae, c.gae_tau, c.gradient_clip = 0.99, True, 0.95, 0.5
    c.rollout_length, c.optimization_epochs, c.mini_batch_size, c.ppo_ratio_clip = 2048, 10, 64, 0.2
    c.log_interval, c.max_steps, c.target_kl = 2048, 3e6, 0.01
    c.state_normalizer = d.MeanStdNormalizer()
    n_mb = 10 * (2048 * workers // 64)
    return d.PPOAgent(c), dict(env_per_step=2048 * workers, updates_per_step=n_mb)


def ppo_pixel(workers=8, device=True, **switches):
    c = d.Config()
    c.merge(dict(game="BreakoutNoFrameskip-v4", log_level=0, tag="bench", skip=False, device_env=device, **switches))
    c.num_workers = workers
    c.task_fn = lambda: d.Task(c.game, num_envs=c.num_workers, seed=1)
    c.eval_env = d.Task(c.game, seed=2)
    c.optimizer_fn = lambda p: torch.optim.Adam(p, lr=2.5e-4)
    c.network_fn = lambda: d.CategoricalActorCriticNet(c.state_dim, c.action_dim, d.NatureConvBody())
    c.state_normalizer = d.ImageNormalizer()
    c.reward_normalizer = d.SignNormalizer()
    c.discount, c.use_gae, c.gae_tau, c.entropy_weight, c.gradient_clip = 0.99, True, 0.95, 0.01, 0.5
    c.rollout_length, c.optimization_epochs = 128, 4
    c.mini_batch_size = c.rollout_length * c.num_workers // 4
    c.ppo_ratio_clip, c.shared_repr, c.max_steps = 0.1, True, int(2e7)
    c.log_interval = c.rollout_length * c.num_workers
    return d.PPOAgent(c), dict(env_per_step=128 * workers, updates_per_step=16)


CASES = {
    "dqn_pixel_uniform": lambda: dqn_family("dqn", d.UniformReplay),                      # fused learner attached
    "dqn_pixel_uniform_host_async": lambda: dqn_family("dqn", d.UniformReplay, async_actor=True),   # host emulator, async actor
    "dqn_pixel_uniform_generic": lambda: dqn_family("dqn", d.UniformReplay, fused=False),  # autograd path
    "dqn_pixel_per": lambda: dqn_family("dqn", d.PrioritizedReplay),
    "c51_pixel_uniform": lambda: dqn_family("c51", d.UniformReplay),
    "c51_pixel_per": lambda: dqn_family("c51", d.PrioritizedReplay),
    "qr_dqn_pixel_uniform": lambda: dqn_family("qr", d.UniformReplay),
    "rainbow_pixel_per": lambda: dqn_family("rainbow", d.PrioritizedReplay),      # noisy layers on csrc/noisy.hip, captured actor forward + PER update
    # environment, actor forward (batch 4, one noise draw per row), argmax and ring feed on the device: deeprl_amd/noisy_actor.py
    "rainbow_pixel_per_device": lambda: dqn_family("rainbow", d.PrioritizedReplay, device=True, device_noisy_actor=True),
    "rainbow_pixel_per_modules": lambda: dqn_family("rainbow", d.PrioritizedReplay, fused_noisy=False, graph_update=False),
    "dqn_pixel_per_device": lambda: dqn_family("dqn", d.PrioritizedReplay, device=True),
    "dqn_pixel_per_device_sync": lambda: dqn_family("dqn", d.PrioritizedReplay, device=True, async_actor=False),
    "dqn_pixel_uniform_device": lambda: dqn_family("dqn", d.UniformReplay, device=True),
    "c51_pixel_uniform_device": lambda: dqn_family("c51", d.UniformReplay, device=True),
    "c51_pixel_per_device": lambda: dqn_family("c51", d.PrioritizedReplay, device=True),
    "qr_dqn_pixel_uniform_device": lambda: dqn_family("qr", d.UniformReplay, device=True),
    "a2c_pixel_16": lambda: a2c_pixel(16),                      # device-resident environments (the default)
    "a2c_pixel_16_host": lambda: a2c_pixel(16, device=False),   # host emulators
    "a2c_pixel_16_recompute": lambda: a2c_pixel(16, reuse_rollout_activations=False),   # the update recomputes conv1-3 (rounds 2-5)
    "ppo_pixel_8": lambda: ppo_pixel(8),
    "n_step_dqn_pixel_16": lambda: n_step_dqn_pixel(16),                      # device-resident rollout + one captured graph
    "n_step_dqn_pixel_16_host": lambda: n_step_dqn_pixel(16, device=False),   # host emulators (the reference's loop)
    "option_critic_pixel_16": lambda: option_critic_pixel(16),                      # device-resident rollout + one captured graph
    "option_critic_pixel_16_host": lambda: option_critic_pixel(16, device=False),   # host emulators (the reference's loop)
    "a2c_pixel_16_nofc4head": lambda: a2c_pixel(16, fuse_fc4_head=False),      # fc4 finish / policy head as separate autograd nodes
    "ppo_pixel_8_nofc4head": lambda: ppo_pixel(8, fuse_fc4_head=False),
    "a2c_pixel_16_gemv": lambda: a2c_pixel(16, rollout_fc4_slices=False),       # rollout fc4 as the eight-wave GEMV (module path)
    "ppo_pixel_8_gemv": lambda: ppo_pixel(8, rollout_fc4_slices=False),
    "a2c_pixel_16_modules": lambda: a2c_pixel(16, fused_rollout=False),         # rollout through network.forward (5 launches / step)
    "ppo_pixel_8_modules": lambda: ppo_pixel(8, fused_rollout=False),
    "ppo_pixel_8_host": lambda: ppo_pixel(8, device=False),
    "a2c_continuous": lambda: a2c_continuous(16),                      # device-resident rollout (csrc/a2c_mlp.hip) + one captured graph
    "a2c_continuous_host": lambda: a2c_continuous(16, device=False),   # 16 python environments stepped one by one, module head
    "a2c_feature": lambda: a2c_feature(5),                      # device-resident cart-poles (csrc/cat_mlp.hip) + one captured graph
    "a2c_feature_host": lambda: a2c_feature(5, device=False),   # 5 python cart-poles stepped one by one, one module forward per step
    # device-resident cart-poles, one rollout and one update launch (csrc/q_mlp.hip) + one captured graph
    "n_step_dqn_feature": lambda: n_step_dqn_feature(5, fused_nstep_feature=True),
    "n_step_dqn_feature_module_update": lambda: n_step_dqn_feature(5, fused_nstep_feature=True, fused_nstep_update=False),
    "n_step_dqn_feature_host": lambda: n_step_dqn_feature(5),   # 5 python cart-poles stepped one by one, one module forward per step
    # device-resident cart-poles, one rollout and one update launch (csrc/oc_mlp.hip) + one captured graph
    "option_critic_feature": lambda: option_critic_feature(5, fused_oc_feature=True),
    "option_critic_feature_module_update": lambda: option_critic_feature(5, fused_oc_feature=True, fused_oc_update=False),
    "option_critic_feature_host": lambda: option_critic_feature(5),   # 5 python cart-poles, one module forward and three draws per step
    # one device-resident cart-pole feeding the HBM replay ring, one acting and one update launch (csrc/dqn_mlp.hip) + captured graphs
    "dqn_feature": lambda: dqn_feature(fused_dqn_feature=True),
    "dqn_feature_module_update": lambda: dqn_feature(fused_dqn_feature=True, fused_dqn_update=False),
    "dqn_feature_host": lambda: dqn_feature(),   # the switch off: the python cart-pole, four module forwards and ring feeds per step
    # dqn_feature with its replay options (n_step 3; _per: a PrioritizedReplay) on the same path under config.fused_dqn_replay_feature
    # (dra_dqn_replay_mlp_update); _host: the switch off, the parent's path for these options
    "dqn_feature_per": lambda: dqn_feature(n_step=3, replay_cls=d.PrioritizedReplay, fused_dqn_replay_feature=True, fused_dqn_replay_update=True),
    "dqn_feature_per_module_update": lambda: dqn_feature(n_step=3, replay_cls=d.PrioritizedReplay, fused_dqn_replay_feature=True,
                                                         fused_dqn_replay_update=False),
    "dqn_feature_per_host": lambda: dqn_feature(n_step=3, replay_cls=d.PrioritizedReplay),
    "dqn_feature_nstep": lambda: dqn_feature(n_step=3, fused_dqn_replay_feature=True, fused_dqn_replay_update=True),
    "dqn_feature_nstep_module_update": lambda: dqn_feature(n_step=3, fused_dqn_replay_feature=True, fused_dqn_replay_update=False),
    "dqn_feature_nstep_host": lambda: dqn_feature(n_step=3),
    # the two distributional entries on the same path (csrc/dist_mlp.hip): 50 atoms on [-100, 100] / 20 quantiles
    "categorical_dqn_feature": lambda: dist_feature("categorical", fused_dist_feature=True, fused_dist_update=True),
    "categorical_dqn_feature_module_update": lambda: dist_feature("categorical", fused_dist_feature=True, fused_dist_update=False),
    "categorical_dqn_feature_host": lambda: dist_feature("categorical"),   # the switch off: the python cart-pole, module forwards, ops.c51_loss
    "quantile_regression_dqn_feature": lambda: dist_feature("quantile", fused_dist_feature=True, fused_dist_update=True),
    "quantile_regression_dqn_feature_module_update": lambda: dist_feature("quantile", fused_dist_feature=True, fused_dist_update=False),
    "quantile_regression_dqn_feature_host": lambda: dist_feature("quantile"),   # the switch off
    # rainbow_feature on the same Step (csrc/rainbow_mlp.hip): noisy layers, PER, n_step 3, double_q
    "rainbow_feature": lambda: rainbow_feature(fused_rainbow_feature=True, fused_rainbow_update=True),
    "rainbow_feature_module_update": lambda: rainbow_feature(fused_rainbow_feature=True, fused_rainbow_update=False),
    "rainbow_feature_host": lambda: rainbow_feature(),   # the switch off: the python cart-pole, per transition a noise draw and four noisy modules
    "ppo_continuous_1": lambda: ppo_continuous(1),
    "ppo_continuous_16": lambda: ppo_continuous(16),                                  # device environments + persistent kernels
    "ppo_continuous_16_host": lambda: ppo_continuous(16, device=False),               # host environments, persistent update kernel
    "ppo_continuous_16_generic": lambda: ppo_continuous(16, device=False, fused=False),   # round-4 path
    "ddpg_continuous": lambda: dpg_continuous("ddpg"),                          # fused update + acting forward (csrc/dpg_mlp.hip)
    "ddpg_continuous_modules": lambda: dpg_continuous("ddpg", fused=False),     # torch modules, two torch.optim.Adam
    "td3_continuous": lambda: dpg_continuous("td3"),
    "td3_continuous_modules": lambda: dpg_continuous("td3", fused=False),
    "ddpg_continuous_device": lambda: dpg_continuous("ddpg", device=True),      # + the environment and the ring feed on the device
    "td3_continuous_device": lambda: dpg_continuous("td3", device=True),
    "ddpg_pendulum": lambda: dpg_continuous("ddpg", game="classic-Pendulum-v0", device=True),
    "ddpg_pendulum_host": lambda: dpg_continuous("ddpg", game="classic-Pendulum-v0"),
    "td3_pendulum": lambda: dpg_continuous("td3", game="classic-Pendulum-v0", device=True),
    "td3_pendulum_host": lambda: dpg_continuous("td3", game="classic-Pendulum-v0"),
}


# an entry's seeds as lanes of one launch: run only when named in --cases (the default set is CASES)
SEED_CASES = {"dqn_feature_seeds%d" % n: (lambda n=n: dqn_feature_seeds(n)) for n in (1, 4, 16, 64)}
SEED_CASES.update({"categorical_dqn_feature_seeds%d" % n: (lambda n=n: dist_feature_seeds("categorical", n)) for n in (1, 4, 16)})
SEED_CASES.update({"quantile_regression_dqn_feature_seeds%d" % n: (lambda n=n: dist_feature_seeds("quantile", n)) for n in (1, 4, 16)})
SEED_CASES.update({"dqn_feature_nstep_seeds%d" % n: (lambda n=n: dqn_feature_nstep_seeds(n)) for n in (1, 4, 16, 64)})

# the same with the lanes' draws taken on the device (seed_batch.py, device_draws=True): a dict of their own, named in --cases
SEED_DRAW_CASES = {"dqn_feature_seeds%d_device_draws" % n: (lambda n=n: dqn_feature_seeds(n, True)) for n in (1, 4, 16, 64)}
SEED_DRAW_CASES.update({"categorical_dqn_feature_seeds%d_device_draws" % n: (lambda n=n: dist_feature_seeds("categorical", n, True))
                        for n in (4, 16)})
SEED_DRAW_CASES.update({"quantile_regression_dqn_feature_seeds%d_device_draws" % n: (lambda n=n: dist_feature_seeds("quantile", n, True))
                        for n in (4, 16)})
SEED_DRAW_CASES.update({"dqn_feature_nstep_seeds%d_device_draws" % n: (lambda n=n: dqn_feature_nstep_seeds(n, True)) for n in (1, 4, 16, 64)})


# the continuous entries evaluate on the pendulum, on their device path, the zoo's 20 episodes (of 200 steps) a time
DPG_EVAL = {"ddpg_continuous_eval": "ddpg_pendulum", "td3_continuous_eval": "td3_pendulum"}


def _eval_agent(name):
    entry = DPG_EVAL.get(name, name[:-len("_eval")])
    agent, meta = CASES[entry]()
    if name in DPG_EVAL:
        agent.config.eval_episodes = 20
    return agent, meta


def _eval_side(agent):
    """What holds an agent's device evaluation and its counters: dqn_mlp.Step, or dpg_mlp.Update."""
    return getattr(agent, '_feature', None) or agent._fused_dpg()


def _fresh_eval_env(agent, seed=2):
    agent.config.eval_env = d.Task(agent.config.game, seed=seed)
    return agent.config.eval_env


def run_eval_case(name, tag, calls=3, warm=5000):
    """<entry>_eval: see the module's docstring.  The agent trains for `warm` agent steps first, so that the evaluated episodes
    are those of a run under way, not a fresh network's few steps (the continuous entries: 1 500 steps, 500 past their warm-up)."""
    agent, meta = _eval_agent(name)
    warm = 1500 if name in DPG_EVAL else warm
    for _ in range(warm):
        agent.step()
    torch.cuda.synchronize()
    cfg, step = agent.config, _eval_side(agent)
    cfg.fused_eval = True
    _fresh_eval_env(agent)
    agent.eval_episodes()                       # (not timed: the environment's move onto the device, the first launch)
    host_task = _fresh_eval_env(agent)          # (the device side keeps its own from here on)
    cfg.fused_eval = False
    agent.eval_episodes()                       # (not timed either)
    out = {**tag, "case": name, "episodes": int(cfg.eval_episodes), "calls": calls, "trained_agent_steps": warm}
    got = dict(host=([], [], []), device=([], [], []))
    for _ in range(calls):                      # the two sides alternate
        for side, switch in (("host", False), ("device", True)):
            cfg.fused_eval = switch
            before = int(host_task.env.envs[0].c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mean = agent.eval_episodes()['episodic_return_test']
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            n = int(step.eval_steps) if switch else int(host_task.env.envs[0].c) - before
            us, steps, means = got[side]
            us.append(dt * 1e6 / n)
            steps.append(n)
            means.append(float(mean))
    assert step.eval_launches == calls + 1 == step.eval_copies
    for side, (us, steps, means) in got.items():
        out.update({side + "_us_per_step": [round(min(us), 2), round(max(us), 2)], side + "_steps": steps, side + "_mean_return": means})
    out["host_over_device"] = [round(min(got["host"][0]) / max(got["device"][0]), 1), round(max(got["host"][0]) / min(got["device"][0]), 1)]
    print(json.dumps(out), flush=True)
    agent.close()


def run_steps_eval_case(name, tag, runs=3, max_steps=25000):
    """dqn_feature_run_steps_eval / ddpg_pendulum_run_steps_eval: see the module's docstring."""
    import random
    from deeprl_amd.support import run_steps
    pendulum = name.startswith("ddpg_pendulum")
    max_steps = 20000 if pendulum else max_steps
    out = {**tag, "case": name, "max_steps": max_steps, "runs": runs}
    for side, switch in (("host_eval", False), ("device_eval", True)):
        wall, inside, last = [], [], []
        for _ in range(runs):
            d.random_seed(0)
            torch.manual_seed(0)
            random.seed(0)
            if pendulum:
                agent = zoo.agent("ddpg_continuous", game="classic-Pendulum-v0", tag="bench", max_steps=max_steps, fused_dpg_update=True,
                                  fused_dpg_env=True, fused_eval=switch)
            else:
                agent = zoo.agent("dqn_feature", game="classic-CartPole-v0", tag="bench", async_replay=False, max_steps=max_steps,
                                  fused_dqn_feature=True, fused_eval=switch)
            spent, means, evaluate = [0.0], [], agent.eval_episodes

            def timed():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = evaluate()
                torch.cuda.synchronize()
                spent[0] += time.perf_counter() - t0
                means.append(float(got['episodic_return_test']))
                return got
            agent.eval_episodes = timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(agent)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            inside.append(spent[0])
            last.append(means)
        out.update({side + "_wall_s": [round(min(wall), 3), round(max(wall), 3)],
                    side + "_inside_eval_s": [round(min(inside), 3), round(max(inside), 3)],
                    side + "_eval_share": [round(min(i / w for i, w in zip(inside, wall)), 3), round(max(i / w for i, w in zip(inside, wall)), 3)],
                    side + "_mean_returns": last[0]})
    print(json.dumps(out), flush=True)


def run_eval_lanes_case(name, tag, calls=3, warm=5000):
    """<a seeds case>_eval: see the module's docstring.  Both sides step the SAME device environments, so each repeat's two sides
    start from one snapshot of them (restored outside the timed windows); the next repeat goes on from where the loop side ended."""
    batch, meta = SEED_EVAL_CASES[name]()
    for _ in range(warm):
        batch.step()
    batch.drain_episodes()
    n_ep, lanes = int(batch.cfg.eval_episodes), meta["lanes"]
    batch.evaluate(n_ep)                             # (not timed: the first launch of either kernel, the blocks' allocation)
    for st in batch.steps_:
        st.evaluate(n_ep)
    got = dict(lanes_launch=[], lane_loop=[])
    steps, longest = [], []
    for _ in range(calls):
        start = [vec.state_dict() for vec in batch.eval_vecs]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        together = batch.evaluate(n_ep)
        torch.cuda.synchronize()
        got["lanes_launch"].append((time.perf_counter() - t0) * 1e6)
        lengths, per_lane = batch.eval_lengths.copy(), batch.eval_steps.copy()
        for vec, state in zip(batch.eval_vecs, start):
            vec.load_state_dict(state)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_by_one = [st.evaluate(n_ep) for st in batch.steps_]
        torch.cuda.synchronize()
        got["lane_loop"].append((time.perf_counter() - t0) * 1e6)
        if not (np.array_equal(together.view(np.uint64), np.asarray(one_by_one).view(np.uint64))
                and all(np.array_equal(lengths[k], st.eval_lengths) for k, st in enumerate(batch.steps_))):
            raise AssertionError("%s: the lane launch and the loop over the single launches returned different episodes" % name)
        steps.append(int(per_lane.sum()))
        longest.append(int(per_lane.max()))
    assert batch.eval_launches == calls + 1 == batch.eval_copies
    out = {**tag, "case": name, "lanes": lanes, "episodes": n_ep, "calls": calls, "trained_agent_steps": warm, "eval_steps_all_lanes": steps,
           "eval_steps_longest_lane": longest, "mean_return": [round(float(together.mean()), 2)]}
    for side, us in got.items():
        out[side + "_us_per_evaluation"] = [round(min(us), 1), round(max(us), 1)]
    out["lanes_launch_us_per_longest_lane_step"] = [round(min(u / n for u, n in zip(got["lanes_launch"], longest)), 2),
                                                    round(max(u / n for u, n in zip(got["lanes_launch"], longest)), 2)]
    out["loop_over_lanes_launch"] = [round(min(got["lane_loop"]) / max(got["lanes_launch"]), 2),
                                     round(max(got["lane_loop"]) / min(got["lanes_launch"]), 2)]
    print(json.dumps(out), flush=True)
    batch.close()


# the lanes' evaluation in one launch against a loop over the lanes of the single launch: named in --cases
SEED_EVAL_CASES = {"dqn_feature_seeds%d_eval" % n: (lambda n=n: dqn_feature_seeds(n, eval_lanes=True)) for n in (1, 4, 16, 64)}
SEED_EVAL_CASES.update({"categorical_dqn_feature_seeds%d_eval" % n: (lambda n=n: dist_feature_seeds("categorical", n, eval_lanes=True))
                        for n in (1, 4, 16)})
SEED_EVAL_CASES.update({"quantile_regression_dqn_feature_seeds%d_eval" % n: (lambda n=n: dist_feature_seeds("quantile", n, eval_lanes=True))
                        for n in (1, 4, 16)})

EVAL_CASES = {"dqn_feature_eval": run_eval_case, "categorical_dqn_feature_eval": run_eval_case,
              "quantile_regression_dqn_feature_eval": run_eval_case, "rainbow_feature_eval": run_eval_case,
              "dqn_feature_run_steps_eval": run_steps_eval_case,
              "ddpg_continuous_eval": run_eval_case, "td3_continuous_eval": run_eval_case,
              "ddpg_pendulum_run_steps_eval": run_steps_eval_case, **{name: run_eval_lanes_case for name in SEED_EVAL_CASES}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--repeats", type=int, default=1,
                    help="walk the whole case list this many times; the lines then carry the pass's number as 'repeat'")
    a = ap.parse_args()
    agents_mod.get_logger = lambda *x, **k: _Quiet()
    d.select_device(0)
    d.random_seed(0)
    for repeat in range(1, a.repeats + 1):
        run_cases(a, dict(repeat=repeat) if a.repeats > 1 else {})


def run_cases(a, tag):
    for name in a.cases.split(","):
        try:
            if name in EVAL_CASES:
                EVAL_CASES[name](name, tag)
                continue
            agent, meta = {**CASES, **SEED_CASES, **SEED_DRAW_CASES}[name]()
            warm = 120 if "dqn" in name or "c51" in name or "rainbow" in name else 4      # DQN family: past exploration_steps; on-policy: past graph capture
            warm = meta.get("warm", warm)                                                 # (replay actor-critics: past warm_up)
            for _ in range(warm):
                agent.step()
            torch.cuda.synchronize()
            if "lanes" in meta:                 # the draws and the staging of a step, host time: prepare_us_per_lane_step
                spent, prepare = [0.0], agent.prepare

                def timed_prepare():
                    t0 = time.perf_counter()
                    learn = prepare()
                    spent[0] += time.perf_counter() - t0
                    return learn
                agent.prepare = timed_prepare
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < a.seconds or n < 2:
                agent.step()
                n += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            line_tag = tag
            if "lanes" in meta:
                line_tag = dict(tag, lanes=meta["lanes"], prepare_us_per_step=round(spent[0] / n * 1e6, 2),
                                prepare_us_per_lane_step=round(spent[0] / (n * meta["lanes"]) * 1e6, 2))
            print(json.dumps({**line_tag, "case": name, "agent_steps": n, "seconds": round(dt, 2), "agent_steps_per_s": round(n / dt, 2),
                              "env_steps_per_s": round(n * meta["env_per_step"] / dt, 1),
                              "updates_per_s": round(n * meta["updates_per_step"] / dt, 1)}), flush=True)
            if hasattr(agent, "close"):
                agent.close()
            if os.environ.get("BENCH_AGENTS_SETTLE"):
                del agent
                import gc
                gc.collect()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
        except Exception as e:
            import traceback
            print(json.dumps({**tag, "case": name, "error": repr(e), "trace": traceback.format_exc()[-600:]}), flush=True)


if __name__ == "__main__":
    main()
