"""What tests/golden/make_golden_crosscheck_dpg.py records of the reference's ddpg_continuous / td3_continuous entry points
(examples.py:554-617) and tests/test_dpg_env_host.py compares deeprl_amd.zoo with: crosscheck_cases.describe_config does not see
what these two entries add -- a network that owns its two optimisers, a replay handed over without a wrapper, the random process,
warm_up / target_network_mix / the td3_* fields (plain fields: they are in `plain`)."""
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CROSSCHECK_DPG_JSON = os.path.join(HERE, "crosscheck_dpg.json")
DPG_GAMES = {"ddpg_continuous": "HalfCheetah-v2", "td3_continuous": "HalfCheetah-v2"}
_PLAIN = (int, float, bool, str, type(None))


def _schedule(s):
    return None if s is None else (type(s).__name__, getattr(s, "inc", None), getattr(s, "current", None), getattr(s, "end", None),
                                   getattr(s, "val", None))


def _opt(opt):
    return (type(opt).__name__, {k: v for k, v in opt.defaults.items() if isinstance(v, (int, float, bool, tuple))},
            sum(p.numel() for g in opt.param_groups for p in g["params"]))


def describe_dpg_config(cfg):
    """Everything comparable about one of the two Configs without a GPU, as {field: repr(value)}."""
    out = {k: v for k, v in vars(cfg).items() if isinstance(v, _PLAIN) and not k.startswith("_")}
    out.pop("tag", None)
    out["normalizers"] = (type(cfg.state_normalizer).__name__, getattr(cfg.state_normalizer, "coef", None),
                          type(cfg.reward_normalizer).__name__, getattr(cfg.reward_normalizer, "coef", None))
    for name in ("optimizer_fn", "actor_opt_fn", "critic_opt_fn"):
        out[name] = getattr(cfg, name, None) is not None
    rp = cfg.replay_fn()
    wrapped = hasattr(rp, "replay_cls")
    kw = dict(rp.replay_kwargs) if wrapped else dict(memory_size=rp.memory_size, batch_size=rp.batch_size)
    out["replay"] = ((rp.replay_cls if wrapped else type(rp)).__name__, sorted(kw.items()), bool(rp.async_) if wrapped else None)
    torch.manual_seed(0)
    net = cfg.network_fn()
    out["network"] = (type(net).__name__, [(k, tuple(v.shape)) for k, v in net.state_dict().items()])
    out["network_opts"] = (_opt(net.actor_opt), _opt(net.critic_opt))
    proc = cfg.random_process_fn()
    out["random_process"] = (type(proc).__name__, tuple(proc.size), _schedule(proc.std), getattr(proc, "theta", None),
                             getattr(proc, "dt", None), getattr(proc, "x0", None), getattr(proc, "mu", None))
    task = cfg.task_fn()
    out["task"] = (task.name, task.state_dim, task.action_dim, getattr(getattr(task, "env", None), "num_envs", None))
    out["eval_env"] = (cfg.eval_env.name, getattr(getattr(cfg.eval_env, "env", None), "num_envs", None))
    return {k: repr(v) for k, v in out.items()}
