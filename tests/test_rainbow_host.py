"""Rainbow on pixels, host side (no GPU): the zoo entry against the Config the reference's examples.py::rainbow_pixel builds
(tests/golden/rainbow/rainbow_pixel_config.json, recorded by tests/golden/make_golden_rainbow.py), the staged noise draw of
RainbowNet.reset_noise() against the reference's recorded noise vectors and generator position, and the lazily formed
weight_epsilon / bias_epsilon of the state dict."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fake_envs
import ref_shim
from golden import crosscheck_cases as C
from golden.make_golden_cases import NOISE_BUFFERS, NOISY_LAYERS, RAINBOW_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "rainbow", "rainbow_pixel_config.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rainbow_dueling.npz")

needs_ref = pytest.mark.skipif(not ref_shim.available(), reason="needs the reference checkout")


@pytest.fixture(autouse=True)
def _leave_global_state_alone():
    """These tests seed the generators, switch the package's device and raise Config.NOISY_LAYER_STD; the tests after them see
    what they saw before."""
    import deeprl_amd as d
    np_state, torch_state, device, std = np.random.get_state(), torch.get_rng_state(), d.Config.DEVICE, d.Config.NOISY_LAYER_STD
    yield
    np.random.set_state(np_state)
    torch.set_rng_state(torch_state)
    d.Config.DEVICE, d.Config.NOISY_LAYER_STD = device, std


def test_zoo_rainbow_pixel_equals_reference_example():
    import deeprl_amd as d
    from deeprl_amd import zoo
    rec = json.load(open(RECORD))
    want = rec["config"]
    assert rec["agent"] == zoo.ZOO["rainbow_pixel"]["agent"] == "CategoricalDQNAgent"
    d.select_device(-1)
    d.Config.NOISY_LAYER_STD = 0.1
    np.random.seed(0)
    have = C.describe_config(zoo.config("rainbow_pixel", game=rec["game"]))
    assert d.Config.NOISY_LAYER_STD == rec["noisy_layer_std"] == 0.5
    assert set(want) == set(have), sorted(set(want) ^ set(have))
    for k in sorted(want):
        assert want[k] == have[k], "%s: reference %s, zoo %s" % (k, want[k], have[k])


@needs_ref
def test_rainbow_record_is_the_reference_output(tmp_path):
    """The committed record equals a fresh one made from the reference checkout (in a fresh interpreter: importing the reference
    installs stand-in modules that must not leak into the other tests)."""
    out = str(tmp_path / "rainbow_pixel_config.json")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.check_call([sys.executable] + flags + [os.path.join(ROOT, "tests", "golden", "make_golden_rainbow.py"), out],
                          cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert json.load(open(out)) == json.load(open(RECORD))


def _net(d, fused):
    d.Config.NOISY_LAYER_STD = 0.5
    torch.manual_seed(9)
    net = d.RainbowNet(4, 51, d.NatureConvBody(noisy_linear=True), noisy_linear=True)
    net.set_fused_noisy(fused)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in fake_envs.numpy_params(RAINBOW_SHAPES, 33).items()}, strict=False)
    torch.manual_seed(11)
    net.reset_noise()
    return net


def test_staged_noise_draw_is_the_reference_stream():
    """One normal_ per vector into slices of one staging block, in the reference's order: the block, the modules' buffers and
    the generator's position afterwards equal the per-module draw and the reference's recorded vectors, bit for bit."""
    import deeprl_amd as d
    d.select_device(-1)
    g = np.load(GOLDEN)
    net = _net(d, True)
    blk = net.noise_block()
    assert [name for name, _ in blk.layers] == ["fc_value", "fc_advantage", "body.fc4"]      # the reference's draw order
    assert sorted(blk.slices) == sorted((la, b) for la in NOISY_LAYERS for b in NOISE_BUFFERS)
    ends = 0
    for name, _ in blk.layers:
        for b in d.NoisyLinear.NOISE_NAMES:
            o, n = blk.slices[(name, b)]
            assert o >= ends and o % 4 == 0      # disjoint, 16-byte aligned, in draw order
            ends = o + n
            want = g["rainbow_%s.%s" % (name, b)]
            assert np.array_equal(blk.host[o:o + n].numpy(), want), (name, b)
            buf = getattr(net.get_submodule(name), b)
            assert np.array_equal(buf.numpy(), want), (name, b)
            assert buf.data_ptr() == blk.flat.data_ptr() + 4 * o      # a view of the flat buffer: static address
    tail = torch.randint(0, 1 << 30, (4,)).numpy()
    _net(d, False)                                  # per-module draw from the same seeds
    assert np.array_equal(tail, torch.randint(0, 1 << 30, (4,)).numpy())
    # a second draw lands in the same device buffers
    ptrs = [getattr(m, b).data_ptr() for _, m in blk.layers for b in d.NoisyLinear.NOISE_NAMES]
    net.reset_noise()
    assert ptrs == [getattr(m, b).data_ptr() for _, m in blk.layers for b in d.NoisyLinear.NOISE_NAMES]
    assert net.noise_block() is blk


def test_state_dict_forms_epsilon_on_demand():
    import deeprl_amd as d
    d.select_device(-1)
    net = _net(d, True)
    ref = _net(d, False)
    f = d.NoisyLinear.transform_noise
    for _ in range(2):       # after construction + load, and after a further redraw
        sd = net.state_dict()
        assert set(sd) == set(ref.state_dict())
        for la in NOISY_LAYERS:
            m = net.get_submodule(la)
            assert {la + "." + k for k in ("weight_mu", "weight_sigma", "weight_epsilon", "bias_mu", "bias_sigma", "bias_epsilon",
                                             "noise_in", "noise_out_weight", "noise_out_bias")} <= set(sd)
            assert torch.equal(sd[la + ".weight_epsilon"], torch.outer(f(m.noise_out_weight), f(m.noise_in))), la
            assert torch.equal(sd[la + ".bias_epsilon"], f(m.noise_out_bias)), la
        net.reset_noise()
    # a copy through the state dict carries products that match the copied vectors
    other = _net(d, True)
    other.load_state_dict(net.state_dict())
    other_sd = other.state_dict()
    for k, v in net.state_dict().items():
        assert torch.equal(v, other_sd[k]), k
