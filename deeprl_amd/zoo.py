"""Ready-made experiment configurations: the hyper-parameters of the reference's examples.py entry points, as DATA.

`ZOO[name]` holds what examples.py sets field by field (cited per entry); `config(name, **kw)` turns an entry into a
`Config`, `agent(name, **kw)` builds the agent, `run(name, **kw)` is `run_steps(agent)`.  Module-level functions with
the reference's names (`dqn_pixel(game=...)`, ...) make this file usable wherever examples.py is
(`python -m deeprl_amd.launch deeprl_amd/zoo.py dqn_pixel game=BreakoutNoFrameskip-v4`).

Keyword arguments are merged into the Config first, like examples.py does (`config.merge(kwargs)`); two extras are
applied LAST so that short runs are possible without editing a table: `max_steps=` and `overrides={field: value}`.
tests/test_zoo_vs_reference.py checks every entry against the Config the reference's own function builds.
"""
import torch
import torch.nn.functional as F

# absolute imports: this file is also executed as a plain examples file by deeprl_amd.launch
from deeprl_amd import agents as A, nets as N
from deeprl_amd.envs import Task
from deeprl_amd.normalizers import ImageNormalizer, MeanStdNormalizer, SignNormalizer
from deeprl_amd.random_process import GaussianProcess, OrnsteinUhlenbeckProcess
from deeprl_amd.replay import PrioritizedReplay, ReplayWrapper, UniformReplay
from deeprl_amd.support import Config, LinearSchedule, generate_tag, run_steps


def _rmsprop(**kw):
    return lambda params: torch.optim.RMSprop(params, **kw)


def _adam(**kw):
    return lambda params: torch.optim.Adam(params, **kw)


# name -> spec.  `kw`: kwargs.setdefault(...) of the entry point; `fields`: plain Config fields; the callables receive
# the Config under construction (they are evaluated lazily, exactly where examples.py uses a lambda).
ZOO = {
    # examples.py:11-52
    "dqn_feature": dict(
        agent="DQNAgent", kw=dict(log_level=0, n_step=1, replay_cls=UniformReplay, async_replay=True),
        task=lambda c: Task(c.game), eval_task="same", optimizer=_rmsprop(lr=0.001),
        network=lambda c: N.VanillaNet(c.action_dim, N.FCBody(c.state_dim)),
        fields=dict(history_length=1, batch_size=10, discount=0.99, max_steps=1e5, replay_eps=0.01, replay_alpha=0.5,
                    target_network_update_freq=200, exploration_steps=1000, double_q=False, sgd_update_frequency=4,
                    gradient_clip=5, eval_interval=int(5e3), async_actor=False),
        replay=dict(memory_size=int(1e4), with_n_step=True), eps=(1.0, 0.1, 1e4), beta=(0.4, 1.0)),
    # examples.py:55-97
    "dqn_pixel": dict(
        agent="DQNAgent", kw=dict(log_level=0, n_step=1, replay_cls=UniformReplay, async_replay=True),
        task=lambda c: Task(c.game), eval_task="same",
        optimizer=_rmsprop(lr=0.00025, alpha=0.95, eps=0.01, centered=True),
        network=lambda c: N.VanillaNet(c.action_dim, N.NatureConvBody(in_channels=c.history_length)),
        fields=dict(batch_size=32, discount=0.99, history_length=4, max_steps=int(2e7), replay_eps=0.01, replay_alpha=0.5,
                    target_network_update_freq=10000, exploration_steps=50000, sgd_update_frequency=4, gradient_clip=5,
                    double_q=False, async_actor=True),
        normalizers=(ImageNormalizer, SignNormalizer),
        replay=dict(memory_size=int(1e6), with_n_step=True), eps=(1.0, 0.01, 1e6), beta=(0.4, 1.0)),
    # examples.py:101-127 (fused_dist_feature=True moves the cart-pole, the replay's feed and the update onto the device: csrc/dist_mlp.hip)
    "quantile_regression_dqn_feature": dict(
        agent="QuantileRegressionDQNAgent", kw=dict(log_level=0), task=lambda c: Task(c.game), eval_task="same",
        optimizer=_rmsprop(lr=0.001),
        network=lambda c: N.QuantileNet(c.action_dim, c.num_quantiles, N.FCBody(c.state_dim)),
        fields=dict(batch_size=10, discount=0.99, target_network_update_freq=200, exploration_steps=100, num_quantiles=20,
                    gradient_clip=5, sgd_update_frequency=4, eval_interval=int(5e3), max_steps=1e5),
        replay=dict(memory_size=int(1e4), fixed_cls=UniformReplay, fixed_async=True), eps=(1.0, 0.1, 1e4)),
    # examples.py:164-193 (fused_dist_feature=True: as above)
    "categorical_dqn_feature": dict(
        agent="CategoricalDQNAgent", kw=dict(log_level=0), task=lambda c: Task(c.game), eval_task="same",
        optimizer=_rmsprop(lr=0.001),
        network=lambda c: N.CategoricalNet(c.action_dim, c.categorical_n_atoms, N.FCBody(c.state_dim)),
        fields=dict(batch_size=10, discount=0.99, target_network_update_freq=200, exploration_steps=100,
                    categorical_v_max=100, categorical_v_min=-100, categorical_n_atoms=50, gradient_clip=5,
                    sgd_update_frequency=4, eval_interval=int(5e3), max_steps=1e5),
        replay=dict(memory_size=int(1e4), fixed_cls=UniformReplay, fixed_async=True), eps=(1.0, 0.1, 1e4)),
    # examples.py:129-161
    "quantile_regression_dqn_pixel": dict(
        agent="QuantileRegressionDQNAgent", kw=dict(log_level=0), task=lambda c: Task(c.game), eval_task="same",
        optimizer=_adam(lr=0.00005, eps=0.01 / 32),
        network=lambda c: N.QuantileNet(c.action_dim, c.num_quantiles, N.NatureConvBody()),
        fields=dict(batch_size=32, discount=0.99, target_network_update_freq=10000, exploration_steps=50000,
                    sgd_update_frequency=4, gradient_clip=5, num_quantiles=200, max_steps=int(2e7)),
        normalizers=(ImageNormalizer, SignNormalizer),
        replay=dict(memory_size=int(1e6), history_length=4, fixed_cls=UniformReplay, fixed_async=True), eps=(1.0, 0.01, 1e6)),
    # examples.py:196-227
    "categorical_dqn_pixel": dict(
        agent="CategoricalDQNAgent", kw=dict(log_level=0), task=lambda c: Task(c.game), eval_task="same",
        optimizer=_adam(lr=0.00025, eps=0.01 / 32),
        network=lambda c: N.CategoricalNet(c.action_dim, c.categorical_n_atoms, N.NatureConvBody()),
        fields=dict(batch_size=32, discount=0.99, target_network_update_freq=10000, exploration_steps=50000,
                    categorical_v_max=10, categorical_v_min=-10, categorical_n_atoms=51, sgd_update_frequency=4,
                    gradient_clip=0.5, max_steps=int(2e7)),
        normalizers=(ImageNormalizer, SignNormalizer),
        replay=dict(memory_size=int(1e6), history_length=4, fixed_cls=UniformReplay, fixed_async=True), eps=(1.0, 0.01, 1e6)),
    # examples.py:231-280 (noisy_linear is set on the Config behind merge(kwargs), not through setdefault: a field; NOISY_LAYER_STD
    # stays at the class's value.  fused_rainbow_feature=True moves the cart-pole, the replay's feed and the update onto the device:
    # csrc/rainbow_mlp.hip)
    "rainbow_feature": dict(
        agent="CategoricalDQNAgent", kw=dict(log_level=0, n_step=3, replay_cls=PrioritizedReplay, async_replay=True),
        task=lambda c: Task(c.game), eval_task="same", optimizer=_rmsprop(lr=0.001),
        network=lambda c: N.RainbowNet(c.action_dim, c.categorical_n_atoms, N.FCBody(c.state_dim, noisy_linear=c.noisy_linear),
                                       noisy_linear=c.noisy_linear),
        fields=dict(max_steps=1e5, noisy_linear=True, categorical_v_max=100, categorical_v_min=-100, categorical_n_atoms=50,
                    discount=0.99, batch_size=32, replay_eps=0.01, replay_alpha=0.5, target_network_update_freq=200,
                    exploration_steps=1000, double_q=True, sgd_update_frequency=4, eval_interval=int(5e3), async_actor=True,
                    gradient_clip=10),
        replay=dict(memory_size=int(1e4), with_n_step=True, history_length=1), eps=(1.0, 0.1, 1e4), beta=(0.4, 1)),
    # examples.py:283-336 (Config.NOISY_LAYER_STD is a CLASS attribute the entry point raises to 0.5 when it runs)
    "rainbow_pixel": dict(
        agent="CategoricalDQNAgent",
        kw=dict(log_level=0, n_step=1, replay_cls=PrioritizedReplay, async_replay=True, noisy_linear=True),
        task=lambda c: Task(c.game), eval_task="same", class_fields=dict(NOISY_LAYER_STD=0.5),
        optimizer=_adam(lr=0.000625, eps=1.5e-4),
        network=lambda c: N.RainbowNet(c.action_dim, c.categorical_n_atoms, N.NatureConvBody(noisy_linear=c.noisy_linear),
                                       noisy_linear=c.noisy_linear),
        fields=dict(max_steps=int(2e7), categorical_v_max=10, categorical_v_min=-10, categorical_n_atoms=51, batch_size=32,
                    discount=0.99, history_length=4, replay_eps=0.01, replay_alpha=0.5, target_network_update_freq=2000,
                    exploration_steps=20000, sgd_update_frequency=4, double_q=True, async_actor=True, gradient_clip=10),
        normalizers=(ImageNormalizer, SignNormalizer),
        replay=dict(memory_size=int(1e6), with_n_step=True), eps=(1, 0.01, 25e4), beta=(0.4, 1.0)),
    # examples.py:340-358
    "a2c_feature": dict(
        agent="A2CAgent", kw=dict(log_level=0), pre_fields=dict(num_workers=5),
        task=lambda c: Task(c.game, num_envs=c.num_workers), eval_task=lambda c: Task(c.game),
        optimizer=_rmsprop(lr=0.001),
        network=lambda c: N.CategoricalActorCriticNet(c.state_dim, c.action_dim, N.FCBody(c.state_dim, gate=F.tanh)),
        fields=dict(discount=0.99, use_gae=True, gae_tau=0.95, entropy_weight=0.01, rollout_length=5, gradient_clip=0.5)),
    # examples.py:361-381
    "a2c_pixel": dict(
        agent="A2CAgent", kw=dict(log_level=0), pre_fields=dict(num_workers=16),
        task=lambda c: Task(c.game, num_envs=c.num_workers), eval_task=lambda c: Task(c.game),
        optimizer=_rmsprop(lr=1e-4, alpha=0.99, eps=1e-5),
        network=lambda c: N.CategoricalActorCriticNet(c.state_dim, c.action_dim, N.NatureConvBody()),
        fields=dict(discount=0.99, use_gae=True, gae_tau=1.0, entropy_weight=0.01, rollout_length=5, gradient_clip=5,
                    max_steps=int(2e7)),
        normalizers=(ImageNormalizer, SignNormalizer)),
    # examples.py:384-404
    "a2c_continuous": dict(
        agent="A2CAgent", kw=dict(log_level=0), pre_fields=dict(num_workers=16),
        task=lambda c: Task(c.game, num_envs=c.num_workers), eval_task=lambda c: Task(c.game),
        optimizer=_rmsprop(lr=0.0007),
        network=lambda c: N.GaussianActorCriticNet(c.state_dim, c.action_dim, actor_body=N.FCBody(c.state_dim),
                                                   critic_body=N.FCBody(c.state_dim)),
        fields=dict(discount=0.99, use_gae=True, gae_tau=1.0, entropy_weight=0.01, rollout_length=5, gradient_clip=5,
                    max_steps=int(2e7))),
    # examples.py:408-424 (fused_nstep_feature=True moves the cart-poles and the update onto the device: csrc/q_mlp.hip)
    "n_step_dqn_feature": dict(
        agent="NStepDQNAgent", kw=dict(log_level=0), pre_fields=dict(num_workers=5),
        task=lambda c: Task(c.game, num_envs=c.num_workers), eval_task=lambda c: Task(c.game),
        optimizer=_rmsprop(lr=0.001),
        network=lambda c: N.VanillaNet(c.action_dim, N.FCBody(c.state_dim)),
        fields=dict(discount=0.99, target_network_update_freq=200, rollout_length=5, gradient_clip=5),
        eps=(1.0, 0.1, 1e4)),
    # examples.py:427-447
    "n_step_dqn_pixel": dict(
        agent="NStepDQNAgent", kw=dict(log_level=0), pre_fields=dict(num_workers=16),
        task=lambda c: Task(c.game, num_envs=c.num_workers), eval_task=lambda c: Task(c.game),
        optimizer=_rmsprop(lr=1e-4, alpha=0.99, eps=1e-5),
        network=lambda c: N.VanillaNet(c.action_dim, N.NatureConvBody()),
        fields=dict(discount=0.99, target_network_update_freq=10000, rollout_length=5, gradient_clip=5, max_steps=int(2e7)),
        eps=(1.0, 0.05, 1e6), normalizers=(ImageNormalizer, SignNormalizer)),
    # examples.py:450-468 (fused_oc_feature=True moves the cart-poles, the option choice and the update onto the device: csrc/oc_mlp.hip)
    "option_critic_feature": dict(
        agent="OptionCriticAgent", kw=dict(log_level=0), pre_fields=dict(num_workers=5),
        task=lambda c: Task(c.game, num_envs=c.num_workers), eval_task=lambda c: Task(c.game),
        optimizer=_rmsprop(lr=0.001),
        network=lambda c: N.OptionCriticNet(N.FCBody(c.state_dim), c.action_dim, num_options=2),
        fields=dict(discount=0.99, target_network_update_freq=200, rollout_length=5, termination_regularizer=0.01,
                    entropy_weight=0.01, gradient_clip=5),
        option_eps=(1.0, 0.1, 1e4)),
    # examples.py:471-492
    "option_critic_pixel": dict(
        agent="OptionCriticAgent", kw=dict(log_level=0), pre_fields=dict(num_workers=16),
        task=lambda c: Task(c.game, num_envs=c.num_workers), eval_task=lambda c: Task(c.game),
        optimizer=_rmsprop(lr=1e-4, alpha=0.99, eps=1e-5),
        network=lambda c: N.OptionCriticNet(N.NatureConvBody(), c.action_dim, num_options=4),
        fields=dict(discount=0.99, target_network_update_freq=10000, rollout_length=5, gradient_clip=5, max_steps=int(2e7),
                    entropy_weight=0.01, termination_regularizer=0.01),
        option_eps=(0.1,), normalizers=(ImageNormalizer, SignNormalizer)),
    # examples.py:525-550
    "ppo_pixel": dict(
        agent="PPOAgent", kw=dict(skip=False), pre_fields=dict(num_workers=8),
        task=lambda c: Task(c.game, num_envs=c.num_workers), eval_task=lambda c: Task(c.game),
        optimizer=_adam(lr=2.5e-4),
        network=lambda c: N.CategoricalActorCriticNet(c.state_dim, c.action_dim, N.NatureConvBody()),
        fields=dict(discount=0.99, use_gae=True, gae_tau=0.95, entropy_weight=0.01, gradient_clip=0.5, rollout_length=128,
                    optimization_epochs=4, ppo_ratio_clip=0.1, shared_repr=True, max_steps=int(2e7)),
        derived=lambda c: dict(mini_batch_size=c.rollout_length * c.num_workers // 4,
                               log_interval=c.rollout_length * c.num_workers),
        normalizers=(ImageNormalizer, SignNormalizer)),
    # examples.py:494-522
    "ppo_continuous": dict(
        agent="PPOAgent", kw=dict(log_level=0), task=lambda c: Task(c.game), eval_task="same",
        network=lambda c: N.GaussianActorCriticNet(c.state_dim, c.action_dim, actor_body=N.FCBody(c.state_dim, gate=torch.tanh),
                                                   critic_body=N.FCBody(c.state_dim, gate=torch.tanh)),
        actor_opt=_adam(lr=3e-4), critic_opt=_adam(lr=1e-3),
        fields=dict(discount=0.99, use_gae=True, gae_tau=0.95, gradient_clip=0.5, rollout_length=2048, optimization_epochs=10,
                    mini_batch_size=64, ppo_ratio_clip=0.2, log_interval=2048, max_steps=3e6, target_kl=0.01),
        normalizers=(MeanStdNormalizer, None)),
    # examples.py:554-579 (the network owns its two optimisers; a plain UniformReplay, no wrapper.  fused_dpg_update=True runs the
    # update on csrc/dpg_mlp.hip, fused_dpg_env=True with it moves an envs.Pendulum / SyntheticContinuous task onto the device)
    "ddpg_continuous": dict(
        agent="DDPGAgent", kw=dict(log_level=0), task=lambda c: Task(c.game), eval_task="same",
        network=lambda c: N.DeterministicActorCriticNet(
            c.state_dim, c.action_dim, actor_body=N.FCBody(c.state_dim, (400, 300), gate=F.relu),
            critic_body=N.FCBody(c.state_dim + c.action_dim, (400, 300), gate=F.relu),
            actor_opt_fn=_adam(lr=1e-3), critic_opt_fn=_adam(lr=1e-3)),
        random_process=lambda c: OrnsteinUhlenbeckProcess(size=(c.action_dim,), std=LinearSchedule(0.2)),
        fields=dict(max_steps=int(1e6), eval_interval=int(1e4), eval_episodes=20, discount=0.99, warm_up=int(1e4),
                    target_network_mix=5e-3),
        replay=dict(memory_size=int(1e6), batch_size=100, plain_cls=UniformReplay)),
    # examples.py:583-617
    "td3_continuous": dict(
        agent="TD3Agent", kw=dict(log_level=0), task=lambda c: Task(c.game), eval_task="same",
        network=lambda c: N.TD3Net(
            c.action_dim, actor_body_fn=lambda: N.FCBody(c.state_dim, (400, 300), gate=F.relu),
            critic_body_fn=lambda: N.FCBody(c.state_dim + c.action_dim, (400, 300), gate=F.relu),
            actor_opt_fn=_adam(lr=1e-3), critic_opt_fn=_adam(lr=1e-3)),
        random_process=lambda c: GaussianProcess(size=(c.action_dim,), std=LinearSchedule(0.1)),
        fields=dict(max_steps=int(1e6), eval_interval=int(1e4), eval_episodes=20, discount=0.99, td3_noise=0.2,
                    td3_noise_clip=0.5, td3_delay=2, warm_up=int(1e4), target_network_mix=5e-3),
        replay=dict(memory_size=int(1e6), batch_size=100, fixed_cls=UniformReplay, fixed_async=True)),
}


def config(name, **kwargs):
    spec = ZOO[name]
    max_steps = kwargs.pop("max_steps", None)
    overrides = kwargs.pop("overrides", None) or {}
    generate_tag(kwargs)
    for k, v in spec.get("kw", {}).items():
        kwargs.setdefault(k, v)
    c = Config()
    c.merge(kwargs)
    for k, v in spec.get("pre_fields", {}).items():
        setattr(c, k, v)
    c.task_fn = lambda: spec["task"](c)
    c.eval_env = c.task_fn() if spec.get("eval_task") == "same" else spec["eval_task"](c)
    for k, v in spec.get("class_fields", {}).items():      # what the entry point sets on the Config CLASS
        setattr(Config, k, v)
    if "optimizer" in spec:
        c.optimizer_fn = spec["optimizer"]
    if "actor_opt" in spec:
        c.actor_opt_fn, c.critic_opt_fn = spec["actor_opt"], spec["critic_opt"]
    c.network_fn = lambda: spec["network"](c)
    for k, v in spec.get("fields", {}).items():
        setattr(c, k, v)
    if "derived" in spec:
        for k, v in spec["derived"](c).items():
            setattr(c, k, v)
    if "eps" in spec:
        c.random_action_prob = LinearSchedule(*spec["eps"])
    if "option_eps" in spec:        # option-critic's epsilon over options (OptionCritic_agent.py:55)
        c.random_option_prob = LinearSchedule(*spec["option_eps"])
    if "random_process" in spec:    # the deterministic-policy agents' exploration noise (DDPG_agent.py:22)
        c.random_process_fn = lambda: spec["random_process"](c)
    if "beta" in spec:
        c.replay_beta = LinearSchedule(spec["beta"][0], spec["beta"][1], c.max_steps)
    norm = spec.get("normalizers")
    if norm:
        if norm[0] is not None:
            c.state_normalizer = norm[0]()
        if norm[1] is not None:
            c.reward_normalizer = norm[1]()
    rp = spec.get("replay")
    if rp:
        kw = dict(memory_size=rp["memory_size"], batch_size=rp["batch_size"] if "batch_size" in rp else c.batch_size)
        if rp.get("with_n_step"):
            # (rainbow_feature hands the replay a literal history_length and leaves the Config's alone)
            kw.update(n_step=c.n_step, discount=c.discount, history_length=rp.get("history_length", c.history_length))
        elif "history_length" in rp:
            kw.update(history_length=rp["history_length"])
        c.replay_kwargs = kw
        if "plain_cls" in rp:       # (ddpg_continuous hands the agent the replay itself, not a wrapper)
            plain = rp["plain_cls"]
            c.replay_fn = lambda: plain(**kw)
        else:
            cls = rp.get("fixed_cls") or c.replay_cls
            flag = rp["fixed_async"] if "fixed_async" in rp else c.async_replay
            c.replay_fn = lambda: ReplayWrapper(cls, kw, flag)
    if max_steps is not None:
        c.max_steps = max_steps
    for k, v in overrides.items():
        setattr(c, k, v)
    return c


def agent(name, **kwargs):
    return getattr(A, ZOO[name]["agent"])(config(name, **kwargs))


def run(name, **kwargs):
    ag = agent(name, **kwargs)
    run_steps(ag)
    return ag


def eval_points(max_steps, eval_interval, steps_per_agent_step):
    """The total_steps at which a run of `max_steps` environment steps evaluates, in support.run_steps' order -- evaluate when due,
    then stop at max_steps, then step -- with the interval tested on total_steps exactly: an agent whose step() advances
    total_steps by `steps_per_agent_step` only triggers on the multiples of eval_interval that it lands on.  There is one at step
    0, and one at the step the run stops at when that is a multiple; eval_interval 0 never evaluates.  Pure: run_seeds' cadence,
    pinned without a device."""
    points, total = [], 0
    while True:
        if eval_interval and total % eval_interval == 0:
            points.append(total)
        if total >= max_steps:
            return points
        total += steps_per_agent_step


def run_seeds(name, seeds, device_draws=False, evaluate=False, **kwargs):
    """`name` once per seed, the seeds as lanes of the same device launches (deeprl_amd/seed_batch.py): per seed, random_seed(seed),
    torch.manual_seed(seed) and config(name, <the entry's switch>=True, **kwargs) over Task(game, seed=seed), stepped until
    config.max_steps environment steps of EVERY lane -> per seed the list of (step, episodic_return) pairs of its training
    episodes, each what the single run of that seed gives.  With `evaluate` off (the default) there is no evaluation on this path:
    eval_interval is forced to 0.
    Three entries have a lane form (seed_batch.SEED_CLASSES): dqn_feature (fused_dqn_feature; n_step 1 and a UniformReplay),
    categorical_dqn_feature and quantile_regression_dqn_feature (fused_dist_feature, and fused_dist_update=True unless kwargs set
    it: the lanes always run the update kernel, so a categorical lane is the single run with fused_dist_update=True, not the
    single run's unset default, which is the module update).  Anything else raises a ValueError that names the reason.
    `fused_dqn_replay_feature=True` among the kwargs picks the class from seed_batch.REPLAY_SEED_CLASSES instead: dqn_feature with
    an n-step window, `n_step=N` (1..8) over a UniformReplay, each lane the single run of its seed with the same two keywords (both
    travel to config() as they do for a single agent).  A PrioritizedReplay stays refused there too, by name.  Without that keyword
    nothing changes: n_step > 1 is refused as before.
    `device_draws=True` (off by default) draws every lane's np.random stream on the device, word for word (seed_batch.py's
    docstring; csrc/np_mt.hip): the same (step, return) lists, without the per-lane host draws.
    `evaluate=True` keeps the entry's eval_interval and eval_episodes (kwargs and overrides still apply), builds the batch with
    eval_lanes=True and runs support.run_steps' order -- evaluate when due (total_steps % eval_interval == 0 exactly: eval_points),
    then stop at max_steps, then step --, every evaluation ONE launch for all lanes (batch.eval_episodes(): each lane's logger gets
    its 'episodic_return_test' line) -> (episodes, evaluations): `episodes` as above, evaluations[k] the list of (total_steps,
    returns fp64 [eval_episodes]) of seed k, each what the single run of that seed with fused_eval=True evaluates."""
    from deeprl_amd.seed_batch import REPLAY_SEED_CLASSES, SEED_CLASSES
    if name not in SEED_CLASSES:
        raise ValueError("run_seeds: besides categorical_dqn_feature and quantile_regression_dqn_feature only dqn_feature runs its "
                         "seeds as lanes, %s has no lane form" % name)
    cls = SEED_CLASSES[name]
    if kwargs.get("fused_dqn_replay_feature") is True:
        if name not in REPLAY_SEED_CLASSES:
            raise ValueError("run_seeds: fused_dqn_replay_feature is dqn_feature's switch, %s has no lane form under it" % name)
        cls = REPLAY_SEED_CLASSES[name]
    switch = {cls.MODULE.Kind.SWITCH: True}

    def make_config(seed):
        c = config(name, **dict(switch, **kwargs))
        c.task_fn = lambda: Task(c.game, seed=seed)
        if not evaluate:
            c.eval_interval = 0
        return c

    batch = cls(make_config, seeds, device_draws=device_draws, eval_lanes=bool(evaluate))
    try:
        out, evals = [[] for _ in batch.seeds], [[] for _ in batch.seeds]
        cfg = batch.lane(0).config
        max_steps = cfg.max_steps
        if not max_steps:
            raise ValueError("run_seeds steps until config.max_steps, which is not set")
        while True:
            if evaluate and cfg.eval_interval and batch.total_steps % cfg.eval_interval == 0:
                batch.eval_episodes()
                for k, got in enumerate(evals):
                    got.append((batch.total_steps, batch.eval_returns[k].copy()))
            if batch.total_steps >= max_steps:
                break
            batch.step()
            if batch.agent_steps % 1024 == 0:
                for k, got in enumerate(out):
                    got += batch.episodes(k)
        for k, got in enumerate(out):
            got += batch.episodes(k)
        return (out, evals) if evaluate else out
    finally:
        batch.close()


def _entry(name):
    def fn(**kwargs):
        return run(name, **kwargs)
    fn.__name__ = name
    fn.__doc__ = "run_steps(%s(config)) with the hyper-parameters of the reference's examples.py::%s" % (ZOO[name]["agent"], name)
    return fn


for _n in ZOO:
    globals()[_n] = _entry(_n)
del _n
