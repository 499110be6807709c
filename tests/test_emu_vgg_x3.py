"""The "bfloat16x3" plain-VGG extractor plans under emulation (tests/vgg_x3_cases.py): per-layer checks of the three-term
bfloat16 sum on partial tiles, odd pooled maps, several images, RGB, the longest reduction and a BatchNorm fold; the end-to-end
distance to the float32 plan against the bfloat16 plan's; scores; the C and Python surface."""

import pytest

import vgg_x3_cases as xc
from emu_util import emu_library, emu_scorer
from host_device import HostDevice


@pytest.mark.parametrize("case", list(xc.CASES))
def test_emu_vgg_x3_per_layer(case):
    # K4608 is the emulator's slowest case (a minute per forward pass): its other routes to the same result are left to the
    # three cases around it here, and run on the MI355X
    xc.check_case(case, HostDevice(), emu_library(), routes=case != "K4608")


def test_emu_vgg_x3_first_convolution_alone():
    xc.check_first_conv_alone(HostDevice(), emu_library())


def test_emu_vgg_x3_against_float32_and_bfloat16_plans():
    xc.check_end_to_end(HostDevice(), emu_library())


def test_emu_vgg_x3_scores_equal_the_float32_plans():
    xc.check_scores(HostDevice(), emu_library(), emu_scorer())


def test_emu_vgg_x3_surface():
    xc.check_surface(HostDevice(), emu_library())
