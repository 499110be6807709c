"""`gpu`: the "bfloat16x3" plain-VGG extractor plans on the MI355X (tests/vgg_x3_cases.py): every convolution's float32 tap
against the float64 restatement of the three-term bfloat16 sum from the record the kernel itself stored, every stored record
against split(maxpool?(tap)) bit for bit, guard bands, the bit-identity of every route to the same features (the registered
torch operators with compute = 3 included), the end-to-end distance to the float32 plan, scores, and the surface."""

import pytest

import vgg_x3_cases as xc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()


@pytest.fixture(scope="module")
def torch_dev():
    from shoeprint_image_retrieval_amd.device import TorchDevice

    return TorchDevice()


@pytest.mark.parametrize("case", list(xc.CASES))
def test_vgg_x3_per_layer(torch_dev, lib, case):
    from shoeprint_image_retrieval_amd import _torch_ops

    xc.check_case(case, torch_dev, lib, ops=_torch_ops.load())


def test_vgg_x3_first_convolution_alone(torch_dev, lib):
    xc.check_first_conv_alone(torch_dev, lib)


def test_vgg_x3_against_float32_and_bfloat16_plans(torch_dev, lib):
    xc.check_end_to_end(torch_dev, lib)


def test_vgg_x3_scores_equal_the_float32_plans(torch_dev, lib):
    from shoeprint_image_retrieval_amd import similarity

    xc.check_scores(torch_dev, lib, similarity.NccScorer(device=torch_dev, library=lib))


def test_vgg_x3_surface(torch_dev, lib):
    xc.check_surface(torch_dev, lib)
