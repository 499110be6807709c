"""`gpu`: per-layer (teacher-forced) parity of the 16-bit EfficientNet and ResNet extractors on the MI355X
(tests/layer_cases.py): every layer of a two- or three-image batch against its float64 restatement from the traced inputs,
the trace run's output bit-identical to the plain forward's, guard bands around out, workspace and trace."""

import pytest

import layer_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()


@pytest.fixture(scope="module")
def torch_dev():
    from shoeprint_image_retrieval_amd.device import TorchDevice

    return TorchDevice()


@pytest.mark.parametrize("arch,block,hw,n,compute", [
    # the shapes of test_efficientnet_on_the_16bit_matrix_cores / test_resnet50_on_the_16bit_matrix_cores, two images
    ("EfficientNetV2_M", 6, (512, 256), 2, "bfloat16"), ("EfficientNetV2_S", 7, (192, 128), 2, "float16"),
    ("EfficientNet_B3", 6, (160, 96), 2, "bfloat16"), ("EfficientNetV2_L", 9, (96, 64), 2, "float16"),
    ("ResNet50", 7, (512, 256), 2, "bfloat16"), ("ResNet50", 7, (160, 96), 2, "float16"), ("ResNet50", 6, (100, 70), 2, "bfloat16"),
    ("EfficientNetV2_M", 6, (100, 70), 3, "float16"),
    ("EfficientNet_B7", 9, (64, 48), 2, "bfloat16"),  # the widest squeeze-excitation (sq = 160), full features
    ("ResNet50", 7, (160, 96), 3, "float16"),
])
def test_per_layer_parity_on_the_16bit_matrix_cores(torch_dev, lib, arch, block, hw, n, compute):
    lc.check_layers(arch, block, hw, n, compute, torch_dev, lib)
