"""support.StagedUpload on real pinned memory: every upload reaches the device tensor intact although the stages are refilled
while earlier copies may still be in flight (the per-stage event is the only thing that orders the two)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("slots", [4, 2])       # 4: the default; 2: ppo_mlp's permutation upload
def test_nine_uploads_through_rotating_pinned_stages(slots):
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    from deeprl_amd.support import StagedUpload
    dev = torch.device("cuda:0")
    up = StagedUpload((3, 5), torch.int64, dev, slots=slots)
    assert len(up.stages) == slots and all(s.is_pinned() for s in up.stages)
    at = up.dev.data_ptr()
    record = torch.zeros((9, 3, 5), dtype=torch.int64, device=dev)
    want = torch.arange(9 * 15, dtype=torch.int64).view(9, 3, 5) * 7919 + 1
    for i in range(9):
        up.stage().copy_(want[i])
        record[i].copy_(up.send())      # same stream: reads .dev behind upload i, ahead of upload i + 1
    torch.cuda.synchronize()
    assert up.dev.data_ptr() == at
    assert torch.equal(record.cpu(), want)
