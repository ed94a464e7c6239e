"""What the GPU tests of the cart-pole feature entries share (tests/test_gpu_{a2c,nstep,option_critic,dqn,dist}_feature.py): the
device fixture, a logger that records, the error bars, guarded buffers and flat parameter buffers for single kernel launches, and
the parsing of the episodic-return lines.  A plain helper module like parity_log.py: the test files import what they use by
name (the `dra` fixture included)."""
import numpy as np
import pytest
import torch

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


def _line_events(lines):
    out = []
    for ln in lines:
        if 'episodic_return_train' in ln:
            w = ln.replace(',', '').split()
            out.append((int(w[1]), float(w[3])))
    return out
