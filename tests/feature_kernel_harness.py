"""What the GPU tests of the cart-pole feature entries share (tests/test_gpu_{a2c,nstep,option_critic,dqn,dist,rainbow}_feature.py):
the device fixture, a logger that records, the error bars, guarded buffers and flat parameter buffers for single kernel launches,
the parsing of the episodic-return lines, and -- for the three entries that act into a replay ring (dqn, dist, rainbow: one
dra_dqn_mlp_act_io) -- the guarded acting launch with its checks.  A plain helper module like parity_log.py: the test files import
what they use by name (the `dra` fixture included)."""
import ctypes

import numpy as np
import pytest
import torch
from parity_log import record_parity

GAME = "classic-CartPole-v0"
GATE = {"relu": 1, "tanh": 2}
GUARD = 8       # elements behind every buffer's stated size, filled with a sentinel that must survive


@pytest.fixture(scope="module")
def dra():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import deeprl_amd as d
    d.select_device(0)
    return d


class _Rec:
    """A logger that keeps the episodic-return lines and the warnings."""

    def __init__(self):
        self.lines, self.warnings = [], []

    def info(self, msg, *a, **k):
        self.lines.append(str(msg))

    def warning(self, msg, *a, **k):
        self.warnings.append(str(msg))

    def add_scalar(self, *a, **k):
        pass
    add_histogram = add_scalar


def _fraction(got, want, what):
    """Largest error as a fraction of 1e-5 of the tensor's largest magnitude, floor 1.0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    bar = 1e-5 * max(float(np.abs(want).max()) if want.size else 0.0, 1.0)
    print("%s: max abs error %.3e (bar %.3e)" % (what, err, bar))
    return err / bar


def _within(got, want, what):
    f = _fraction(got, want, what)
    assert f <= 1.0, (what, f)
    return f


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _as_int(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def _guarded(shape, dtype, dev, fill):
    n = int(np.prod(shape))
    full = torch.full((n + GUARD,), fill, dtype=dtype, device=dev)
    return full, full[:n].view(*shape)


def _flat(keys, params, padded, fill=np.nan):
    """(float32 flat array, offsets per key): the tensors of `keys` back to back, or -- padded -- behind a leading gap with `fill`
    between."""
    offs, chunks, off = {}, [], 0
    if padded:
        chunks.append(np.full(3, fill, dtype=np.float32))
        off = 3
    for k in keys:
        v = np.asarray(params[k], dtype=np.float32).reshape(-1)
        offs[k] = off
        pad = ((-v.size) % 4 + 1) if padded else 0
        chunks += [v, np.full(pad, fill, dtype=np.float32)]
        off += v.size + pad
    return np.concatenate(chunks), offs


def _tails_intact(out):
    for k, (shape, dt, fill) in out["spec"].items():
        tail = out[k][int(np.prod(shape)):]
        assert tail.size == GUARD and (np.isnan(tail).all() if fill != fill else (tail == fill).all()), k


def _body(out, k):
    shape = out["spec"][k][0]
    return out[k][:int(np.prod(shape))].reshape(shape)


# ------------------------------------------------------------------------------------------ the replay entries' acting launch
def _launch_replay_act(dra, fn, net, keep, K, start, k_len, cap, slot0, horizon):
    """One acting launch `fn` (lib.dra_{dqn,dist,rainbow}_mlp_act) of `net` from a case's start -> dict of host arrays (guards
    included) and the return code.  `keep`: the device tensors the net struct points to, which the launch must leave as they are;
    K: the case module (EP_RING_CAP, EP_RING_COUNT0, STEP0)."""
    from deeprl_amd import dqn_mlp
    from deeprl_amd._lib import stream_ptr
    dev = dra.Config.DEVICE
    nan = float("nan")
    kk = max(k_len, 1)
    spec = dict(env_state=((1, 4), torch.float64, nan), env_counter=((1,), torch.int64, -7), ep_steps=((1,), torch.int32, -7),
                ep_return=((1,), torch.float64, nan), env_seed=((1,), torch.int64, -7), step=((1,), torch.int64, -7),
                ep_count=((1,), torch.int64, -7), ep_ring=((K.EP_RING_CAP, 3), torch.float64, nan),
                explore=((kk,), torch.uint8, 9), random_action=((kk,), torch.int64, -7), slot0=((1,), torch.int64, -7),
                frames=((cap, 4), torch.float64, nan), actions=((cap,), torch.int64, -1), rewards=((cap,), torch.float64, nan),
                masks=((cap,), torch.int32, -1), q=((kk, 2), torch.float32, nan), action=((kk,), torch.int64, -7),
                err=((1,), torch.int32, -7))
    full, view = {}, {}
    for k, (shape, dt, fill) in spec.items():
        full[k], view[k] = _guarded(shape, dt, dev, fill)
    view["env_state"].copy_(torch.from_numpy(start["raw"]).view(1, 4))
    view["env_counter"].zero_(); view["ep_steps"].zero_(); view["ep_return"].zero_(); view["err"].zero_()
    view["env_seed"].fill_(start["seed"])
    view["step"].fill_(K.STEP0); view["ep_count"].fill_(K.EP_RING_COUNT0); view["slot0"].fill_(slot0)
    n_draws = min(kk, len(start["explore"]))
    view["explore"].zero_(); view["random_action"].zero_()
    view["explore"][:n_draws].copy_(torch.from_numpy(start["explore"][:n_draws].astype(np.uint8)))
    view["random_action"][:n_draws].copy_(torch.from_numpy(start["random_action"][:n_draws]))
    io = dqn_mlp.ActIO()
    io.env_state, io.env_counter, io.ep_steps = view["env_state"].data_ptr(), view["env_counter"].data_ptr(), view["ep_steps"].data_ptr()
    io.ep_return, io.env_seed, io.step_counter = view["ep_return"].data_ptr(), view["env_seed"].data_ptr(), view["step"].data_ptr()
    io.ep_count, io.ep_ring = view["ep_count"].data_ptr(), view["ep_ring"].data_ptr()
    io.explore, io.random_action, io.slot0 = view["explore"].data_ptr(), view["random_action"].data_ptr(), view["slot0"].data_ptr()
    io.ring_frames, io.ring_actions = view["frames"].data_ptr(), view["actions"].data_ptr()
    io.ring_rewards, io.ring_masks = view["rewards"].data_ptr(), view["masks"].data_ptr()
    io.out_q, io.out_action, io.err = view["q"].data_ptr(), view["action"].data_ptr(), view["err"].data_ptr()
    io.horizon, io.ring_cap, io.capacity, io.reward_coef, io.t_len, io.n_env = horizon, K.EP_RING_CAP, cap, 1.0, k_len, 1
    before = [t.cpu().numpy().copy() for t in keep]
    rc = fn.raw(ctypes.byref(net), ctypes.byref(io), stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in full.items()}
    out["rc"], out["spec"] = rc, spec
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(b)) for t, b in zip(keep, before))
    return out


def _check_act(out, want, env, K, k_len, slot0):
    """A launch's outputs against the restatement's, everything but q to the bit, and the guards -> q's fraction of the bar."""
    assert out["rc"] == 0 and int(_body(out, "err")[0]) == 0
    assert np.array_equal(_body(out, "action"), want["action"])
    ring = want["ring"]
    assert np.array_equal(_bits(_body(out, "frames")), _bits(ring["frames"]))
    assert np.array_equal(_body(out, "actions"), ring["actions"]) and np.array_equal(_body(out, "masks"), ring["masks"])
    assert np.array_equal(_bits(_body(out, "rewards")), _bits(ring["rewards"]))
    assert np.array_equal(_bits(_body(out, "env_state")), _bits(want["raw"].reshape(1, 4)))
    assert int(_body(out, "env_counter")[0]) == env.c and int(_body(out, "ep_steps")[0]) == env.steps
    assert np.array_equal(_bits(_body(out, "ep_return")), _bits(np.asarray([env.ret], dtype=np.float64)))
    assert int(_body(out, "step")[0]) == K.STEP0 + k_len and int(_body(out, "slot0")[0]) == slot0
    assert int(_body(out, "ep_count")[0]) == K.EP_RING_COUNT0 + len(want["events"])
    ep = np.full((K.EP_RING_CAP, 3), np.nan)
    for i, ev in enumerate(want["events"]):
        ep[(K.EP_RING_COUNT0 + i) % K.EP_RING_CAP] = ev
    assert np.array_equal(_bits(_body(out, "ep_ring")), _bits(ep))
    _tails_intact(out)
    return _fraction(_body(out, "q"), want["q"], "q")


def _check_act_case(launch, want, env, K, k_len, slot0, label):
    """test_act_kernel_matches_restatement's body: launch() against the restatement (q within the bar, recorded under `label`), and
    a second launch from the same start with the same bits everywhere."""
    out = launch()
    eq = _check_act(out, want, env, K, k_len, slot0)
    record_parity(label, q=eq)
    assert eq <= 1.0
    again = launch()
    for k in out["spec"]:
        assert np.array_equal(_bits(out[k]), _bits(again[k])), k


def _check_bad_slots(launch, cap):
    """A staged first slot outside [0, capacity) is taken as 0 and counted in the error word: launch(slot0) equals launch(0) bit
    for bit, and nothing outside the ring is written."""
    want = launch(0)
    for bad in (-1, cap, cap + 1000):
        got = launch(bad)
        assert got["rc"] == 0 and int(_body(got, "err")[0]) == 1 and int(_body(want, "err")[0]) == 0
        for k in ("frames", "actions", "rewards", "masks", "q", "action", "env_state", "ep_ring", "step", "ep_count"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        _tails_intact(got)


def _line_events(lines):
    out = []
    for ln in lines:
        if 'episodic_return_train' in ln:
            w = ln.replace(',', '').split()
            out.append((int(w[1]), float(w[3])))
    return out
