"""`gpu`: the 16-bit DenseNet_201 extractor on the MI355X (tests/densenet16_cases.py): every layer of a two- or three-image
batch against its float64 restatement from the traced inputs, the trace run's output bit-identical to the plain forward's,
guard bands around out, workspace and trace, batch invariance, the sanity distance to the float32 network, the surface."""

import pytest

import densenet16_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()


@pytest.fixture(scope="module")
def torch_dev():
    from shoeprint_image_retrieval_amd.device import TorchDevice

    return TorchDevice()


@pytest.mark.parametrize("block,hw,n,compute", [
    (12, (512, 256), 2, "bfloat16"),  # all of `features` at the full print: [1920, 16, 8] out, norm5 in float32
    (9, (160, 96), 3, "float16"),
    (6, (100, 70), 2, "bfloat16"),
    (11, (128, 96), 2, "float16"),
    (10, (96, 64), 2, "bfloat16"),
])
def test_densenet16_per_layer_parity_on_the_matrix_cores(torch_dev, lib, block, hw, n, compute):
    dc.check_layers(block, hw, n, compute, torch_dev, lib)


@pytest.mark.parametrize("block,hw,compute", [(9, (160, 96), "bfloat16"), (12, (128, 96), "float16")])
def test_densenet16_batch_invariance(torch_dev, lib, block, hw, compute):
    dc.check_batch_invariance(block, hw, compute, torch_dev, lib)


def test_densenet16_surface(torch_dev, lib):
    dc.check_surface(torch_dev, lib)


@pytest.mark.parametrize("compute", ["bfloat16", "float16"])
def test_densenet16_get_feature_maps(torch_dev, lib, compute):
    print(dc.check_get_feature_maps(9, (256, 128), compute, torch_dev, lib))
