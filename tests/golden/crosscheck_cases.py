"""Inputs and helpers shared by tests/golden/make_golden_crosscheck.py (which runs them through the reference's own code and
records what it returns) and the CPU tests that compare the package / the oracle with those records
(test_host_utils_vs_reference.py, test_zoo_vs_reference.py, test_dropin_surface.py, test_oracle_vs_golden.py).  Everything
here draws its inputs from fixed seeds, so the generator and the tests see the same cases."""
import dis
import hashlib
import json
import os
import random
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CROSSCHECK_JSON = os.path.join(HERE, "crosscheck.json")
REPLAY_STREAMS_NPZ = os.path.join(HERE, "replay_streams.npz")
MODULES_NPZ = os.path.join(HERE, "crosscheck_modules.npz")
FIXTURE_DIGESTS_JSON = os.path.join(HERE, "fixture_digests.json")


def digest(a):
    """sha256 of an array's dtype, shape and bytes (C order): equal digests <=> bit-identical arrays."""
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a))
    h = hashlib.sha256()
    h.update(("%s|%s|" % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def np_rng_digest(state=None):
    """Digest of numpy's global generator state (key, position, cached gaussian)."""
    st = np.random.get_state() if state is None else state
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(st[1]).tobytes())
    h.update(repr(st[2:]).encode())
    return h.hexdigest()


def py_rng_digest(state=None):
    st = random.getstate() if state is None else state
    return hashlib.sha256(repr(st).encode()).hexdigest()


# ------------------------------------------------------------------------------------------------ host utilities
SCHEDULE_ARGS = ((1.0, 0.1, 7), (0.4, 1.0, 5), (0.5, None, None), (1.0, 0.01, 1e6))
SCHEDULE_STEPS = (1, 1, 3, 1, 10, 1)
EPS_SHAPES = ((1, 4), (8, 6), (5,))
EPS_VALUES = (0.0, 0.3, 1.0)
RANDOM_SAMPLE_CASES = ((64, 16), (70, 16), (5, 8))
STORAGE_KEYS = ["v", "log_pi_a", "reward", "mask"]


def epsilon_greedy_cases():
    rs = np.random.RandomState(0)
    for shape in EPS_SHAPES:
        q = rs.standard_normal(shape)
        for eps in EPS_VALUES:
            yield shape, eps, q


def storage_rows(t_len=5, n=3):
    """The rows fed to Storage(t_len), in feed order."""
    rs = np.random.RandomState(3)
    rows = []
    for t in range(t_len + 1):
        rows.append({"v": torch.tensor(rs.standard_normal((n, 1)).astype(np.float32)),
                     "log_pi_a": torch.tensor(rs.standard_normal((n, 1)).astype(np.float32))})
        if t < t_len:
            rows.append({"reward": torch.tensor(rs.standard_normal((n, 1)).astype(np.float32)),
                         "mask": torch.tensor((rs.rand(n, 1) > 0.2).astype(np.float32))})
    return rows


def loss_case(seed):
    """Inputs of one random loss case (DQN, C51, QR-DQN) in the order they are drawn."""
    rs = np.random.RandomState(500 + seed)
    c = {}
    b, a = int(rs.randint(2, 40)), int(rs.randint(2, 19))
    n_step, double_q = int(rs.randint(1, 4)), bool(rs.randint(0, 2))
    c.update(b=b, a=a, n_step=n_step, double_q=double_q, gamma_n=0.99 ** n_step)
    state = rs.standard_normal((b, 3)).astype(np.float32)
    c["tr"] = dict(state=state, action=rs.randint(0, a, size=b).astype(np.int64), reward=np.sign(rs.standard_normal(b)),
                   next_state=state + 1, mask=(rs.rand(b) > 0.3).astype(np.int32))
    t32 = lambda *s, scale=1.0: torch.tensor((rs.standard_normal(s) * scale).astype(np.float32))
    c["q"], c["qt"], c["qo"] = t32(b, a), t32(b, a), t32(b, a)
    n_atoms = int(rs.choice([11, 21, 51]))
    c.update(n_atoms=n_atoms, vmin=-10.0, vmax=10.0)
    c["lg"], c["lt"], c["lo"] = t32(b, a, n_atoms), t32(b, a, n_atoms, scale=2.0), t32(b, a, n_atoms, scale=2.0)
    nq = int(rs.choice([5, 17, 50]))
    c["nq"] = nq
    c["th"], c["tt"] = t32(b, a, nq), t32(b, a, nq, scale=1.5)
    return c


def module_makers(n):
    """Modules of the library `n` (the package or the reference) whose state_dicts must agree name by name."""
    adam = lambda p: torch.optim.Adam(p, 1e-3)
    return [
        lambda: n.NoisyLinear(7, 5),
        lambda: n.DuelingNet(3, n.FCBody(4, (8,))),
        lambda: n.RainbowNet(3, 5, n.FCBody(4, (8,), noisy_linear=True), True),
        lambda: n.OptionCriticNet(n.FCBody(4, (8,)), 2, 3),
        lambda: n.DeterministicActorCriticNet(4, 2, adam, adam, actor_body=n.FCBody(4, (8,)), critic_body=n.FCBody(6, (8,))),
        lambda: n.TD3Net(2, lambda: n.FCBody(4, (8,)), lambda: n.FCBody(6, (8,)), adam, adam),
        lambda: n.VanillaNet(4, n.NatureConvBody()),
        lambda: n.CategoricalActorCriticNet(4, 3, n.FCBody(4, (8,))),
        lambda: n.GaussianActorCriticNet(4, 2, actor_body=n.FCBody(4, (8,)), critic_body=n.FCBody(4, (8,))),
    ]


def value_digest(t, samples=4096):
    """A tensor's values: [fp64 sum, fp64 sum of squares] + every element (tensors of up to `samples` elements) or about
    `samples` evenly strided ones.  Initial values come out of LAPACK's QR (orthogonal_) and vectorised CPU kernels whose
    last bits depend on the host CPU, so they are compared within float32 rounding, not bit for bit."""
    a = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64).reshape(-1)
    stride = max(1, -(-a.size // samples))
    return np.concatenate([[a.sum(), np.square(a).sum()], a[::stride]])


def state_dict_record(sd):
    """([[name, shape, dtype], ...], {name: value_digest})"""
    return [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()], {k: value_digest(v) for k, v in sd.items()}


def assert_state_dict_records_match(mine, want_meta, want_values, rtol=1e-5, atol=1e-6):
    """Names, order, shapes and dtypes exactly; values within float32 rounding (value_digest)."""
    meta, values = mine
    assert meta == want_meta
    for k, _, _ in meta:
        np.testing.assert_allclose(values[k], want_values[k], rtol=rtol, atol=atol, err_msg=k)


def modules_npz_values(z, prefix):
    """{name: value_digest} of one recorded state_dict in crosscheck_modules.npz (keys '<prefix>|<name>')."""
    return {k.split("|", 1)[1]: z[k] for k in z.files if k.split("|", 1)[0] == prefix}


def fixture_file_digest(z):
    """One digest of a whole .npz fixture: every key in order, each array's digest (object arrays: their str)."""
    h = hashlib.sha256()
    for k in sorted(z.files):
        a = z[k]
        h.update(("%s=%s;" % (k, str(a) if a.dtype == object else digest(a))).encode())
    return h.hexdigest()


def dump_json(data, path):
    """JSON, one line per second-level entry (compact inside), keys sorted."""
    dumps = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))
    items = []
    for k in sorted(data):
        v = data[k]
        if isinstance(v, dict):
            items.append("%s: {\n%s\n}" % (json.dumps(k), ",\n".join("%s: %s" % (json.dumps(k2), dumps(v[k2])) for k2 in sorted(v))))
        else:
            items.append("%s: %s" % (json.dumps(k), dumps(v)))
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(items) + "\n}\n")


def noisy_rainbow_record(lib):
    """RainbowNet with noisy layers: three reset_noise() calls after seeding, then three more torch.rand draws."""
    torch.manual_seed(2)
    net = lib.RainbowNet(3, 5, lib.FCBody(4, (8,), noisy_linear=True), True)
    for _ in range(3):
        net.reset_noise()
    return state_dict_record(net.state_dict()), torch.rand(3).tolist()


def random_process_record(lib, name):
    np.random.seed(3)
    p = getattr(lib, name)(size=(3,), std=lib.LinearSchedule(0.2))
    xs = np.asarray([p.sample().copy() for _ in range(40)])
    p.reset_states()
    return {"samples": xs.tolist(), "tail": float(np.random.rand())}


def run_steps_trace(run_steps, config_cls):
    """The save / log / eval / step / switch_task / close calls run_steps makes for an agent whose step() advances
    total_steps by 4."""
    calls = []

    class Agent:
        def __init__(self):
            self.config = config_cls()
            self.config.tag, self.config.save_interval, self.config.log_interval = "t", 8, 12
            self.config.eval_interval, self.config.max_steps = 16, 40
            self.total_steps = 0
            self.logger = type("L", (), {"info": lambda s, m: calls.append("log " + m.split(",")[0])})()

        def save(self, name):
            calls.append("save " + name)

        def eval_episodes(self):
            calls.append("eval %d" % self.total_steps)

        def step(self):
            self.total_steps += 4
            calls.append("step")

        def switch_task(self):
            calls.append("switch")

        def close(self):
            calls.append("close")

    run_steps(Agent())
    return calls


# ------------------------------------------------------------------------------------------------ examples.py
ZOO_GAMES = {"dqn_feature": "CartPole-v0", "dqn_pixel": "BreakoutNoFrameskip-v4",
             "quantile_regression_dqn_pixel": "BreakoutNoFrameskip-v4", "categorical_dqn_pixel": "BreakoutNoFrameskip-v4",
             "a2c_pixel": "BreakoutNoFrameskip-v4", "ppo_pixel": "BreakoutNoFrameskip-v4", "ppo_continuous": "HalfCheetah-v2"}
ZOO_AGENTS = ["DQNAgent", "CategoricalDQNAgent", "QuantileRegressionDQNAgent", "A2CAgent", "PPOAgent", "NStepDQNAgent",
              "OptionCriticAgent", "DDPGAgent", "TD3Agent"]
_PLAIN = (int, float, bool, str, type(None))


def _schedule(s):
    return None if s is None else (type(s).__name__, getattr(s, "inc", None), getattr(s, "current", None), getattr(s, "end", None),
                                   getattr(s, "val", None))


def describe_config(cfg):
    """Everything comparable about a Config without a GPU, as {field: repr(value)}."""
    out = {k: v for k, v in vars(cfg).items() if isinstance(v, _PLAIN) and not k.startswith("_")}
    out.pop("tag", None)
    out.pop("replay_kwargs", None)
    out["eps_schedule"] = _schedule(cfg.random_action_prob)
    out["beta_schedule"] = _schedule(getattr(cfg, "replay_beta", None))
    out["normalizers"] = (type(cfg.state_normalizer).__name__, getattr(cfg.state_normalizer, "coef", None),
                          type(cfg.reward_normalizer).__name__)
    out["replay_cls"] = getattr(getattr(cfg, "replay_cls", None), "__name__", None)
    dummy = [torch.nn.Parameter(torch.zeros(3))]
    for name in ("optimizer_fn", "actor_opt_fn", "critic_opt_fn"):
        fn = getattr(cfg, name, None)
        if fn is not None:
            opt = fn(dummy)
            out[name] = (type(opt).__name__, {k: v for k, v in opt.defaults.items() if isinstance(v, (int, float, bool, tuple))})
    if cfg.replay_fn is not None:
        rw = cfg.replay_fn()
        out["replay"] = (rw.replay_cls.__name__, dict(rw.replay_kwargs), bool(rw.async_))
    net = cfg.network_fn()
    out["network"] = (type(net).__name__, [(k, tuple(v.shape)) for k, v in net.state_dict().items()])
    task = cfg.task_fn()
    out["task"] = (task.name, task.state_dim, task.action_dim, getattr(getattr(task, "env", None), "num_envs", None))
    out["eval_env"] = (cfg.eval_env.name, getattr(getattr(cfg.eval_env, "env", None), "num_envs", None))
    return {k: repr(v) for k, v in out.items()}


EXAMPLES_IN_SCOPE = ["ddpg_continuous", "td3_continuous", "option_critic_feature", "option_critic_pixel", "dqn_feature", "dqn_pixel",
                     "quantile_regression_dqn_feature", "quantile_regression_dqn_pixel", "categorical_dqn_feature",
                     "categorical_dqn_pixel", "rainbow_feature", "rainbow_pixel", "a2c_feature", "a2c_pixel", "a2c_continuous",
                     "n_step_dqn_feature", "n_step_dqn_pixel", "ppo_continuous", "ppo_pixel"]


def global_names(fn):
    """Every global name a function (and the functions / lambdas nested in it) loads."""
    names = set()
    todo = [fn.__code__]
    while todo:
        code = todo.pop()
        for ins in dis.get_instructions(code):
            if ins.opname in ("LOAD_GLOBAL", "LOAD_NAME"):
                names.add(ins.argval)
        todo += [c for c in code.co_consts if isinstance(c, types.CodeType)]
    return names


# ------------------------------------------------------------------------------------------------ replay streams
REPLAY_SEEDS = (0, 1, 2, 3)
REPLAY_KINDS = ("uniform", "prioritized")       # in this order, on one generator per seed


def replay_params(seed):
    """A random replay configuration (capacity, history, n-step, discount) and the generator its streams continue from."""
    rs = np.random.RandomState(100 + seed)
    cap = int(rs.randint(40, 200))
    h, n = int(rs.randint(1, 5)), int(rs.randint(1, 4))
    gamma = float(rs.choice([1.0, 0.99, 0.5]))
    return rs, dict(cap=cap, b=8, h=h, n=n, gamma=gamma)


def replay_events(rs, p, kind):
    """Random feed / sample / update_priorities interleaving (wrap-around, terminals): ("feed", (frame, action, reward,
    mask)), ("sample", None) and, for the prioritized kind, ("prio", priorities) after every sample."""
    fed = 0
    for step in range(3 * p["cap"]):
        frame = rs.randint(0, 256, size=(3, 3)).astype(np.uint8)
        act, rew, msk = int(rs.randint(0, 4)), float(rs.randint(-1, 2)), int(rs.rand() > 0.2)
        yield "feed", (frame, act, rew, msk)
        fed += 1
        if fed > p["h"] + p["n"] + 4 and step % 7 == 0:
            yield "sample", None
            if kind == "prioritized":
                yield "prio", (rs.rand(p["b"]).astype(np.float32) * 2 + 0.1)
