"""CPU emulation: the pipelined corner-sum gallery preparation (csrc/ncc_prep6.hip) against prep_fft_kernel, on 128 x 64 maps
(124 x 60 after the crop) of the 192 x 96 six-wave plan - channel counts that end the channel pipeline after its first,
second, an odd and a later channel, one and three items, the three storage types, all-zero channels in the middle and at the
end; a smaller map on the same grid; the fall-back for templates smaller than the map; scores against the oracle."""

import pytest

import prep6_cases as pc
from emu_util import emu_scorer


def _make():
    return emu_scorer("fft")


@pytest.mark.parametrize("storage", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("items", [1, 3])
@pytest.mark.parametrize("channels", [1, 2, 3, 5])
def test_prep6_matches_table_kernel(monkeypatch, channels, items, storage):
    pc.check_same_preparation(_make, monkeypatch, items, channels, (128, 64), storage)


def test_prep6_smaller_map_same_grid(monkeypatch):
    # 124 x 60 raw, 120 x 56 after the crop: needs 180 x 84, still the 192 x 96 grid (asserted by two_plans)
    pc.check_same_preparation(_make, monkeypatch, 2, 3, (124, 60), "float32")


def test_prep6_smaller_template_falls_back(monkeypatch):
    pc.check_smaller_template_falls_back(_make, monkeypatch)


def test_prep6_scores_against_oracle(monkeypatch):
    pc.check_scores(_make, monkeypatch)
