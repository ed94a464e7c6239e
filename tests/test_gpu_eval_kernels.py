"""The evaluation kernels (csrc/eval_act.h; dra_dqn_mlp_eval, dra_dist_mlp_eval, dra_rainbow_mlp_eval over dra_mlp_eval_io)
against the fp64 restatement (tests/eval_restatement.py, pinned by tests/test_eval_host.py): per kind and shape
(tests/eval_cases.py) one episode and five episodes at horizon 12, horizon 1 (every step ends an episode) and a start with a
non-zero counter and junk in the episode words; and the launches the entry points refuse."""
import ctypes

import numpy as np
import pytest
import torch
from feature_kernel_harness import (      # noqa: F401  (dra: the fixture)
    GUARD, dra, _fraction, _bits, _guarded, _tails_intact, _body)
from parity_log import record_parity
from test_gpu_dist_feature import _net_struct as _dist_net
from test_gpu_dqn_feature import _net_struct as _dqn_net
from test_gpu_rainbow_feature import _net_struct as _rainbow_net

import eval_cases as C
import eval_restatement as E

pytestmark = pytest.mark.gpu

EINVAL = -22


def _net_of(dra, case, got):
    """(net struct, the device tensors it points to, the kind's entry point)."""
    from deeprl_amd._lib import lib
    kind, hidden, gate = case[:3]
    dev, padded = dra.Config.DEVICE, hidden == 16
    if kind == "dqn":
        net, flat, tflat, _ = _dqn_net(got["params"], None, dev, hidden, gate, padded)
        return net, (flat, tflat), lib.dra_dqn_mlp_eval
    if kind == "dist":
        net, flat, tflat, _ = _dist_net(got["params"], None, dev, got["spec"], hidden, gate, padded)
        return net, (flat, tflat), lib.dra_dist_mlp_eval
    net, keep, _ = _rainbow_net(got["params"], None, [got["noise"]], None, dev, got["spec"], hidden, gate, padded)
    return net, keep, lib.dra_rainbow_mlp_eval


def _launch(dra, case, got, n_episodes, horizon, junk, null=None, with_q=True):
    """One evaluation launch -> dict of host arrays (guards included), the return code and the spec.  `null`: the io field left
    null."""
    from deeprl_amd import dqn_mlp
    from deeprl_amd._lib import stream_ptr
    dev, nan = dra.Config.DEVICE, float("nan")
    net, keep, fn = _net_of(dra, case, got)
    n, rows = max(n_episodes, 1), max(min(n_episodes * horizon, 70000), 1)
    spec = dict(env_state=((1, 4), torch.float64, nan), env_counter=((1,), torch.int64, -7), ep_steps=((1,), torch.int32, -7),
                ep_return=((1,), torch.float64, nan), env_seed=((1,), torch.int64, -7), out_return=((n,), torch.float64, nan),
                out_length=((n,), torch.int32, -7), out_steps=((1,), torch.int64, -7), out_q=((rows, 2), torch.float32, nan))
    full, view = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], view[k] = _guarded(shape, dt, dev, fill)
    j = C.JUNK
    view["env_state"].copy_(torch.tensor([j["state"]], dtype=torch.float64))       # (a reset at the counter replaces it either way)
    view["env_counter"].fill_(j["counter"] if junk else 0)
    view["ep_steps"].fill_(j["ep_steps"] if junk else 0)
    view["ep_return"].fill_(j["ep_return"] if junk else 0.0)
    view["env_seed"].fill_(C.ENV_SEED)
    io = dqn_mlp.EvalIO()
    for k in spec:
        if k != null and (k != "out_q" or with_q):
            setattr(io, k, view[k].data_ptr())
    io.horizon, io.n_episodes = horizon, n_episodes
    before = [t.cpu().numpy().copy() for t in keep]
    start = {k: v.cpu().numpy().copy() for k, v in full.items()}
    rc = fn.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in full.items()}
    out.update(rc=rc, spec=spec, start=start)
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(b)) for t, b in zip(keep, before))      # parameters and noise untouched
    return out


def _check(out, want, n_episodes):
    """Everything but q to the bit, q's written rows within the bar and the rows behind them untouched, the guards -> q's
    fraction of the bar."""
    assert out["rc"] == 0
    assert np.array_equal(_bits(_body(out, "out_return")), _bits(want["returns"]))
    assert np.array_equal(_body(out, "out_length"), want["lengths"])
    steps = int(_body(out, "out_steps")[0])
    assert steps == want["steps"] == int(want["lengths"].sum())
    assert np.array_equal(_bits(_body(out, "env_state")), _bits(want["state"].reshape(1, 4)))
    assert int(_body(out, "env_counter")[0]) == want["counter"]
    assert int(_body(out, "ep_steps")[0]) == want["ep_steps"] == 0
    assert np.array_equal(_bits(_body(out, "ep_return")), _bits(np.asarray([want["ep_return"]], dtype=np.float64)))
    assert int(_body(out, "env_seed")[0]) == C.ENV_SEED
    q = _body(out, "out_q")
    assert np.isnan(q[steps:]).all()
    _tails_intact(out)
    return _fraction(q[:steps], want["q"], "q")


@pytest.mark.parametrize("label", list(C.LAUNCHES))
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_eval_kernel_matches_restatement(dra, case, label):
    """One evaluation launch against the restatement: returns, lengths, the step count, the environment's words and its counter
    equal to the bit (junk in ep_steps / ep_return and in the state does not survive); q within 1e-5 of scale over the rows
    written, NaN behind them; the guards behind every buffer, the parameter and the noise buffers untouched; a second launch from
    the same start gives the same bits; without out_q the launch leaves the same words.  The restatement's margin is at least 100
    bars, and the five-episode launches end both ways."""
    n_episodes, horizon, junk, both = C.LAUNCHES[label]
    got = C.restated(case)
    want = got["runs"][label]
    print("%s %s: margin %.3e, bar %.3e, lengths %s" % (C.case_id(case), label, want["margin"], E.q_bar(want), list(want["lengths"])))
    assert E.comparable(want, horizon, both) and want["margin"] >= E.MARGIN_BARS * E.q_bar(want)
    if horizon == 1:
        assert want["steps"] == n_episodes
    out = _launch(dra, case, got, n_episodes, horizon, junk)
    eq = _check(out, want, n_episodes)
    record_parity("mlp eval kernel vs restatement %s %s (fraction of the bar)" % (C.case_id(case), label), q=eq)
    assert eq <= 1.0
    again = _launch(dra, case, got, n_episodes, horizon, junk)
    for k in out["spec"]:
        assert np.array_equal(_bits(out[k]), _bits(again[k])), k
    bare = _launch(dra, case, got, n_episodes, horizon, junk, with_q=False)
    assert bare["rc"] == 0 and np.array_equal(_bits(bare["out_q"]), _bits(bare["start"]["out_q"]))
    for k in out["spec"]:
        if k != "out_q":
            assert np.array_equal(_bits(out[k]), _bits(bare[k])), k


REFUSED = (("no_episodes", 0, 12, None), ("too_many_episodes", 257, 12, None), ("too_many_steps", 1, 65537, None),
           ("too_many_steps_in_all", 241, 272, None), ("no_horizon", 5, 0, None), ("null_state", 5, 12, "env_state"),
           ("null_returns", 5, 12, "out_return"), ("null_steps", 5, 12, "out_steps"))


@pytest.mark.parametrize("case", [c for c in C.CASES if c[1] == 64 and c[2] == "relu"], ids=C.case_id)
@pytest.mark.parametrize("what", REFUSED, ids=lambda w: w[0])
def test_refused_launches_write_nothing(dra, case, what):
    """n_episodes 0 and 257, n_episodes * horizon 65537 (as 1 x 65537) and 65552 (as 241 x 272), horizon 0 and a null pointer:
    DRA_EINVAL, every buffer as it was."""
    from deeprl_amd._lib import lib
    _, n_episodes, horizon, null = what
    if null is None:
        assert lib.dra_mlp_eval_supported.raw(n_episodes, horizon) == EINVAL
    out = _launch(dra, case, C.restated(case), n_episodes, horizon, False, null=null)
    assert out["rc"] == EINVAL
    for k in out["spec"]:
        assert np.array_equal(_bits(out[k]), _bits(out["start"][k])), k


def test_supported_table(dra):
    from deeprl_amd._lib import lib
    ok = lib.dra_mlp_eval_supported.raw
    assert ok(1, 1) == 0 and ok(256, 256) == 0 and ok(10, 200) == 0 and ok(1, 65536) == 0
    assert ok(256, 257) == EINVAL and ok(-1, 5) == EINVAL and ok(5, -1) == EINVAL and ok(2, 1 << 40) == EINVAL
