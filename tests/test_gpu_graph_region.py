"""graphs.Region alone on the device: two elementwise launches over a static 1024-float buffer, eager for the warm-up calls and
replayed from the captured hipGraph afterwards, equal to the eager result bit for bit on every call."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WARMUP = 2


def test_region_replays_what_the_eager_body_computes():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    from types import SimpleNamespace
    from deeprl_amd.graphs import Region
    dev = torch.device("cuda:0")
    x, mid, y = (torch.zeros(1024, dtype=torch.float32, device=dev) for _ in range(3))

    def body():
        torch.mul(x, 1.7, out=mid)
        torch.sin(mid, out=y)
        return y

    def eager(inp):
        return torch.sin(inp * 1.7)

    region = Region("the test body", SimpleNamespace(), WARMUP)
    gen = torch.Generator().manual_seed(5)

    def call(key):
        inp = torch.randn(1024, generator=gen).to(dev)
        x.copy_(inp)        # refilled before each call: a replay that read stale input would show
        if region.due(key) and (region.graph is not None or region.capture(body, key)):
            out = region.replay()
        else:
            out = body()
        assert torch.equal(out, eager(inp)), "call %d differs from the eager result" % region.calls

    for i in range(WARMUP + 3):
        call('a')
        assert (region.graph is not None) == (i >= WARMUP), "the graph exists from call W + 1 on"
    first = region.graph
    assert region.out is y
    call('b')
    assert region.graph is not None and region.graph is not first and region.key == 'b'
    call('b')
    assert region.calls == WARMUP + 5 and not region.failed

