#!/usr/bin/env python
"""Generates the cross-check fixtures of the CPU tests that compare the package and the oracle with the REFERENCE's own code
(imported read-only through tests/ref_shim.py), so that those tests run without the reference tree:

  tests/golden/crosscheck.json      host utilities (schedules, epsilon_greedy, random_sample, Storage, Config, generate_tag,
                                    run_steps), the loss cases, module state_dicts / noise draws / random processes (digests),
                                    the Config every examples.py entry builds (zoo) and the global names every entry loads
  tests/golden/crosscheck_modules.npz  the value digests of those module state_dicts
  tests/golden/replay_streams.npz   the reference's UniformReplay / PrioritizedReplay on random feed / sample / update streams
  tests/golden/fixture_digests.json one digest per tests/golden/*.npz file (every array in it) as tests/golden/make_golden.py writes them

Inputs: tests/golden/crosscheck_cases.py.  Re-run:  python tests/golden/make_golden_crosscheck.py   (needs the reference tree)
"""
import builtins
import glob
import json
import os
import random
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402
from golden import crosscheck_cases as C  # noqa: E402

torch.set_num_threads(1)


def t2l(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).tolist()


# ------------------------------------------------------------------------------------------------ host utilities
def host_utils(ref):
    out = {}
    out["schedules"] = []
    for args in C.SCHEDULE_ARGS:
        sch = ref.LinearSchedule(*args)
        out["schedules"].append([sch(s) for s in C.SCHEDULE_STEPS])
    out["constant_schedule"] = ref.ConstantSchedule(0.3)(5)
    eg = []
    for shape, eps, q in C.epsilon_greedy_cases():
        np.random.seed(11)
        b = ref.epsilon_greedy(eps, q)
        tail = int(np.random.randint(1 << 30))
        eg.append({"shape": list(shape), "eps": eps, "action": t2l(b), "tail": tail})
    out["epsilon_greedy"] = eg
    rsmp = []
    for n, b in C.RANDOM_SAMPLE_CASES:
        np.random.seed(n)
        rsmp.append({"n": n, "b": b, "batches": [t2l(np.asarray(v).copy()) for v in ref.random_sample(np.arange(n), b)]})
    out["random_sample"] = rsmp
    st = ref.Storage(5)
    for row in C.storage_rows():
        st.feed(row)
    st.placeholder()
    ex = st.extract(C.STORAGE_KEYS)
    try:
        st.feed({"no_such_key": 1})
        raised = None
    except Exception as e:  # noqa: BLE001
        raised = type(e).__name__
    out["storage"] = {"advantage": [a for a in st.advantage], "fields": list(ex._fields), "values": [t2l(x) for x in ex],
                      "bad_key_raises": raised}
    cfg = ref.Config()
    plain, keys = {}, []
    for k, v in vars(cfg).items():
        if k.startswith("_Config__") or k == "parser":
            continue
        keys.append(k)
        if isinstance(v, (int, float, str, bool, type(None))):
            plain[k] = v
    cfg.merge(dict(game="X-v0", n_step=3, tag="t"))
    pb = dict(game="G", run=2, lr=0.1, fn=len)
    ref.generate_tag(pb)
    out["config"] = {"keys": keys, "plain": plain, "merged": [cfg.game, cfg.n_step, cfg.tag], "tag": pb["tag"]}
    out["run_steps"] = C.run_steps_trace(ref.run_steps, ref.Config)
    return out


class _Obj:
    pass


class _FakeNet:
    def __init__(self, outs):
        self.outs, self.k = list(outs), 0

    def __call__(self, x):
        o = self.outs[self.k % len(self.outs)]
        self.k += 1
        return o


def _cfg(ref, **kw):
    c = ref.Config()
    c.state_normalizer = ref.RescaleNormalizer()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def loss_cases(ref):
    import torch.nn.functional as F
    out = []
    for seed in range(6):
        c = C.loss_case(seed)
        b, n_step, double_q = c["b"], c["n_step"], c["double_q"]
        tr = ref.Transition(**c["tr"])
        rec = {}
        q = c["q"].clone().requires_grad_(True)
        ag = _Obj()
        ag.config = _cfg(ref, discount=0.99, n_step=n_step, double_q=double_q)
        ag.target_network = _FakeNet([dict(q=c["qt"])])
        ag.network = _FakeNet([dict(q=c["qo"]), dict(q=q)] if double_q else [dict(q=q)])
        want = ref.DQNAgent.compute_loss(ag, tr)
        gw, = torch.autograd.grad(ref.DQNAgent.reduce_loss(ag, want), q)
        rec["dqn"], rec["dqn_grad"] = t2l(want), t2l(gw)
        n_atoms, vmin, vmax = c["n_atoms"], c["vmin"], c["vmax"]
        mk = lambda z: dict(prob=F.softmax(z, dim=-1), log_prob=F.log_softmax(z, dim=-1))
        ag = _Obj()
        ag.config = _cfg(ref, discount=0.99, n_step=n_step, double_q=double_q, categorical_v_min=vmin, categorical_v_max=vmax,
                         categorical_n_atoms=n_atoms)
        ag.atoms = ref.tensor(np.linspace(vmin, vmax, n_atoms))
        ag.delta_atom = (vmax - vmin) / float(n_atoms - 1)
        ag.batch_indices = ref.range_tensor(b)
        lg = c["lg"].clone().requires_grad_(True)
        ag.target_network = _FakeNet([mk(c["lt"])])
        ag.network = _FakeNet([mk(c["lo"]), mk(lg)] if double_q else [mk(lg)])
        rec["c51"], rec["atoms"] = t2l(ref.CategoricalDQNAgent.compute_loss(ag, tr)), t2l(ag.atoms)
        nq = c["nq"]
        ag = _Obj()
        ag.config = _cfg(ref, discount=0.99, n_step=n_step, num_quantiles=nq)
        ag.batch_indices = ref.range_tensor(b)
        ag.cumulative_density = ref.tensor((2 * np.arange(nq) + 1) / (2.0 * nq)).view(1, -1)
        th = c["th"].clone().requires_grad_(True)
        ag.target_network = _FakeNet([dict(quantile=c["tt"])])
        ag.network = _FakeNet([dict(quantile=th)])
        rec["qr"] = t2l(ref.QuantileRegressionDQNAgent.compute_loss(ag, tr))
        out.append(rec)
    return out


def modules(ref):
    """Names / shapes / dtypes (JSON) and value digests (crosscheck_modules.npz, '<record>|<name>') of the module state_dicts."""
    out, values = {"state_dicts": []}, {}
    for i, mk in enumerate(C.module_makers(ref)):
        torch.manual_seed(1)
        meta, vals = C.state_dict_record(mk().state_dict())
        out["state_dicts"].append(meta)
        values.update({"sd%d|%s" % (i, k): v for k, v in vals.items()})
    ref.Config.NOISY_LAYER_STD = 0.5
    (meta, vals), tail = C.noisy_rainbow_record(ref)
    out["noisy_rainbow"] = {"state_dict": meta, "tail": tail}
    values.update({"noisy|%s" % k: v for k, v in vals.items()})
    out["random_processes"] = {name: C.random_process_record(ref, name) for name in ("OrnsteinUhlenbeckProcess", "GaussianProcess")}
    return out, values


# ------------------------------------------------------------------------------------------------ examples.py
def examples(ref_root):
    import deeprl_amd as d
    from deeprl_amd import launch
    saved = {k: v for k, v in sys.modules.items() if k == "deep_rl" or k.startswith("deep_rl.")}
    for k in list(saved):
        del sys.modules[k]
    d.select_device(-1)
    zoo = {}
    try:
        for name in sorted(C.ZOO_GAMES):
            mod = launch.load_examples(os.path.join(ref_root, "examples.py"), "ref_examples_zoo")
            got = {}
            for a in C.ZOO_AGENTS:
                setattr(mod, a, lambda cfg, _a=a: (_a, cfg))
            mod.run_steps = lambda pair: got.update(agent=pair[0], cfg=pair[1])
            np.random.seed(0)
            getattr(mod, name)(game=C.ZOO_GAMES[name])
            zoo[name] = {"agent": got["agent"], "config": C.describe_config(got["cfg"])}
        # the global names each entry point loads that examples.py does not define itself (they come from `deep_rl`)
        src = open(os.path.join(ref_root, "examples.py")).read()
        import re
        src = re.sub(r"\basync\b", "async_", src)
        empty = types.ModuleType("deep_rl")
        sys.modules["deep_rl"] = empty
        mod = types.ModuleType("ref_examples_names")
        exec(compile(src, "examples.py", "exec"), mod.__dict__)
        own = set(mod.__dict__)
        per_fn, every = {}, set()
        for k, v in mod.__dict__.items():
            if isinstance(v, types.FunctionType) and v.__module__ == mod.__name__:
                names = sorted(g for g in C.global_names(v) if g not in own and not hasattr(builtins, g))
                every |= set(names)
                if k in C.EXAMPLES_IN_SCOPE:
                    per_fn[k] = names
        assert sorted(per_fn) == sorted(C.EXAMPLES_IN_SCOPE)
    finally:
        for k in [k for k in sys.modules if k == "deep_rl" or k.startswith("deep_rl.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    return zoo, {"per_function": per_fn, "whole_file": sorted(every)}


# ------------------------------------------------------------------------------------------------ replay streams
def replay_streams(ref):
    arrays = {}
    for seed in C.REPLAY_SEEDS:
        rs, p = C.replay_params(seed)
        for kind in C.REPLAY_KINDS:
            cls = ref.UniformReplay if kind == "uniform" else ref.PrioritizedReplay
            r = cls(memory_size=p["cap"], batch_size=p["b"], n_step=p["n"], discount=p["gamma"], history_length=p["h"])
            np.random.seed(seed)
            random.seed(seed)
            st = (np.random.get_state(), random.getstate())
            rec = {k: [] for k in ("state", "next_state", "action", "reward", "mask", "sampling_prob", "idx", "np_rng", "py_rng",
                                   "tree", "max_priority")}
            last = None
            for ev, data in C.replay_events(rs, p, kind):
                if ev == "feed":
                    frame, act, rew, msk = data
                    r.feed(dict(state=[frame], action=[act], reward=[rew], mask=[msk]))
                elif ev == "sample":
                    np.random.set_state(st[0])
                    random.setstate(st[1])
                    last = r.sample()
                    st = (np.random.get_state(), random.getstate())
                    rec["state"].append(np.asarray(last.state))
                    rec["next_state"].append(np.asarray(last.next_state))
                    rec["action"].append(np.asarray(last.action).reshape(-1))
                    rec["reward"].append(np.asarray(last.reward, dtype=np.float64))
                    rec["mask"].append(np.asarray(last.mask))
                    rec["np_rng"].append(C.np_rng_digest(st[0]))
                    rec["py_rng"].append(C.py_rng_digest(st[1]))
                    if kind == "prioritized":
                        rec["sampling_prob"].append(np.asarray(last.sampling_prob))
                        rec["idx"].append(np.asarray(last.idx))
                else:
                    info = list(zip(np.asarray(last.idx).tolist(), data.tolist()))
                    r.update_priorities(info)
                    rec["tree"].append(np.asarray(r.tree.tree).copy())
                    rec["max_priority"].append(float(r.max_priority))
            for k, v in rec.items():
                if v:
                    arrays["s%d_%s_%s" % (seed, kind, k)] = np.stack([np.asarray(x) for x in v])
    return arrays


def fixture_digests():
    """Runs tests/golden/make_golden.py into a scratch directory and digests every file it writes."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([sys.executable, os.path.join(HERE, "make_golden.py")], env=dict(os.environ, GOLDEN_OUT=tmp),
                              stdout=subprocess.DEVNULL)
        for f in sorted(glob.glob(os.path.join(tmp, "*.npz"))):
            out[os.path.basename(f)] = C.fixture_file_digest(np.load(f, allow_pickle=True))
    return out


def main():
    ref = ref_shim.load()
    data = {"host_utils": host_utils(ref), "loss_cases": loss_cases(ref)}
    data["modules"], module_values = modules(ref)
    data["zoo"], data["examples_names"] = examples(ref_shim.REFERENCE_ROOT)
    C.dump_json(data, C.CROSSCHECK_JSON)
    np.savez_compressed(C.MODULES_NPZ, **module_values)
    np.savez_compressed(C.REPLAY_STREAMS_NPZ, **replay_streams(ref))
    with open(C.FIXTURE_DIGESTS_JSON, "w") as f:
        json.dump(fixture_digests(), f, indent=0, sort_keys=True)
    for p in (C.CROSSCHECK_JSON, C.MODULES_NPZ, C.REPLAY_STREAMS_NPZ, C.FIXTURE_DIGESTS_JSON):
        print("wrote %s (%.1f KB)" % (p, os.path.getsize(p) / 1024.0))


if __name__ == "__main__":
    main()
