"""`not gpu`: the float32 matrix-core method ("mfma_f32", SPR_NCC_MFMA_F32) under the CPU emulation, at small channel counts,
against the oracle on the unrounded float32 inputs."""

import numpy as np
import pytest

import mfma_f32_cases as fc
from emu_util import emu_library, emu_scorer


def test_emu_f32_method_resolution():
    fc.check_resolution(emu_scorer)


@pytest.mark.parametrize("channels,nq,ng", [(3, 5, 2), (2, 18, 2), (2, 70, 2), (5, 3, 3)])
def test_emu_f32_equal_size(channels, nq, ng):
    """Query counts that leave waves (18: three of four) and lanes (70: a second block of six) of the last 64-query block
    idle; odd and even channel counts."""
    fc.check_equal_size(emu_scorer, channels, nq, ng)


def test_emu_f32_general_shapes():
    fc.check_general_shapes(emu_scorer, channels=3, nq=2, ng=3)


def test_emu_f32_conditioning():
    fc.check_conditioning(emu_scorer)


def test_emu_f32_degenerate_channels():
    fc.check_degenerate_channels(emu_scorer)


def test_emu_f32_lo_terms_are_needed():
    fc.check_lo_terms_needed(emu_scorer)


def test_emu_f32_opt_in_flag():
    fc.check_opt_in_flag(emu_scorer)


def test_emu_f32_config_flag():
    from host_device import HostDevice
    from shoeprint_image_retrieval_amd.similarity import scorer_from_config

    dev = HostDevice()
    fc.check_config_flag(lambda cfg: scorer_from_config(cfg, device=dev, library=emu_library()))


def test_emu_f32_table_prep(monkeypatch):
    fc.check_table_prep(emu_scorer, monkeypatch)


def test_emu_f32_mean_term(monkeypatch):
    fc.check_mean_term(emu_scorer, monkeypatch)


def test_f32_torch_op_method_name():
    """torch.ops.shoeprint_mi355x.ncc_scores knows "mfma_f32".  Without a GPU that shows in the order of its checks only: a
    CPU tensor is refused before the method is looked at, and the C header, the ctypes mirror and the op's source agree on
    the code of the method."""
    import os
    import re

    import torch
    from shoeprint_image_retrieval_amd import _lib, _torch_ops, similarity

    ops = _torch_ops.load()
    with pytest.raises(RuntimeError, match="must live in HBM"):
        ops.ncc_scores(torch.zeros(1, 2, 32, 16), torch.zeros(1, 2, 32, 16), 2, "mfma_f32", 0)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "shoeprint_mi355x.h")).read()
    assert int(re.search(r"SPR_NCC_MFMA_F32\s*=\s*(\d+)", header).group(1)) == _lib.NCC_MFMA_F32
    assert _lib.METHOD_NAMES[_lib.NCC_MFMA_F32] == "mfma_f32" and similarity._METHODS["mfma_f32"] == _lib.NCC_MFMA_F32
    src = open(os.path.join(os.path.dirname(_lib.DEFAULT_PATH), "csrc", "torch_ops.cpp")).read()
    assert 'if (m == "mfma_f32") return SPR_NCC_MFMA_F32;' in src
