"""`gpu`: per-layer (teacher-forced) parity of the float32 extractor plans on the MI355X (tests/f32_layer_cases.py): every layer
of a two- or three-image batch against its float64 restatement from the traced float32 records - the rigorous (K + C) u A and
the tight (4 sqrt(K) + C) u A bound -, the trace run's output bit-identical to the plain forward's, the VGG routes (taps, no
taps, Model.extract_taps_device) bit-identical, guard bands around out, workspace, trace and every tap buffer.

The headline shape (VGG16[:16] at 512 x 256, n = 2) is left out: this check carries two intervals per element through the
epilogue, so its float64 restatement costs more than the 16-bit test's case of that shape."""

import pytest

import f32_layer_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()


@pytest.fixture(scope="module")
def torch_dev():
    from shoeprint_image_retrieval_amd.device import TorchDevice

    return TorchDevice()


@pytest.mark.parametrize("arch,block,hw,n,rgb", [
    ("VGG16", 30, (64, 48), 2, False),            # reaches the 512 -> 512 layers: K = 4608
    ("VGG16", 16, (100, 70), 2, False),           # not a multiple of the 16-pixel tile, odd sizes under the pools
    ("VGG16", 2, (40, 36), 2, True),              # the first convolution alone, RGB
    ("VGG19_BN", 26, (64, 48), 3, False),         # folded BatchNorm weights
    ("ResNet50", 7, (160, 96), 2, False),         # all four (ks, stride) instances, downsample branches
    ("ResNet50", 6, (100, 70), 2, False),         # 50 x 35 -> 25 x 18: layer1's tensor outgrows the stem's
    ("ResNet50", 7, (32, 32), 2, True),           # the minimum size, RGB
    ("EfficientNet_B3", 6, (160, 96), 2, False),  # 5x5 depthwise, squeeze-excitation
    ("EfficientNetV2_S", 7, (96, 64), 2, True),   # fused-MBConv then MBConv, RGB
    ("EfficientNet_B7", 9, (64, 48), 2, False),   # the widest squeeze-excitation, full features
    ("DenseNet_201", 7, (96, 64), 3, False),
    ("DenseNet_201", 9, (128, 96), 2, True),      # crosses two transitions, RGB
])
def test_f32_per_layer_parity(torch_dev, lib, arch, block, hw, n, rgb):
    fc.check_layers(arch, block, hw, n, torch_dev, lib, rgb=rgb)
