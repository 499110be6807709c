"""`not gpu`: shortlist retrieval (csrc/topk.hip, NccScorer.topk_device / locate, similarity.retrieve) on the CPU-emulation
build - the checks of shortlist_cases.py, which tests/test_gpu_shortlist.py runs through the real library."""

import os
import subprocess
import sys

import pytest

import shortlist_cases as sc
from emu_util import emu_scorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scorer():
    return emu_scorer("fft")


@pytest.mark.parametrize("k", sc.TOPK_KS)
@pytest.mark.parametrize("size", sc.TOPK_SIZES)
def test_emu_topk_order(scorer, size, k):
    sc.check_topk_order(scorer, size, k)


def test_emu_topk_edges(scorer):
    sc.check_topk_edges(scorer)


def test_emu_topk_merge(scorer):
    sc.check_topk_merge(scorer)


def test_emu_strided_views_are_refused(scorer):
    sc.check_strided_views_are_refused(scorer)


def test_shortlist_config_key():
    from shoeprint_image_retrieval_amd.config import MI355X_DEFAULTS, normalise

    assert MI355X_DEFAULTS["shortlist"] == 0 and normalise({})["mi355x"]["shortlist"] == 0
    assert normalise({"mi355x": {"shortlist": 256}})["mi355x"]["shortlist"] == 256
    for bad in (-1, 257, 300, 2.5, "3", True):
        with pytest.raises(ValueError, match="shortlist"):
            normalise({"mi355x": {"shortlist": bad}})


def test_emu_grid_stride(scorer, monkeypatch):
    sc.check_grid_stride(scorer, monkeypatch)


@pytest.mark.parametrize("shape", sc.PEAK_SHAPES)
def test_emu_maps_peak_exact(scorer, shape):
    sc.check_maps_peak_exact(scorer, shape)


def test_emu_maps_peak_arguments(scorer):
    sc.check_maps_peak_arguments(scorer)


def test_emu_reverse_work_item_order():
    """Both kernels with the work-items of a workgroup run from the last to the first (SPR_EMU_ORDER=reverse, fixed when
    the emulation starts: a process of its own): the same bits."""
    env = dict(os.environ, SPR_EMU_ORDER="reverse")
    sel = "maps_peak_exact or topk_merge or topk_edges or grid_stride or (topk_order and 300)"
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", sel],
                       env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# (method, storage) that cover a planted case: the matrix-core forms take cropped maps up to 28 x 12, the direct form what
# fits LDS; 124 x 60 maps go to the six-wave 192 x 96 grid ("fft") and the four-wave 256 x 128 one ("fft_pow2")
LOCATE = [("fft", "float32", 0), ("fft_pow2", "float32", 0), ("direct", "float32", 0), ("mfma", "bfloat16", 0),
          ("mfma_f32", "float32", 0), ("fft", "float32", 1), ("fft_pow2", "float32", 1), ("direct", "float32", 1),
          ("mfma", "bfloat16", 1), ("mfma_f32", "float32", 1), ("fft", "float32", 2), ("fft_pow2", "float32", 2)]


@pytest.mark.parametrize("method,storage,case", LOCATE)
def test_emu_locate_planted(method, storage, case):
    sc.check_locate_planted(emu_scorer(method, storage=storage), sc.PLANTED_CASES[case])


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_emu_locate_variants(method):
    sc.check_locate_variants(emu_scorer(method))


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_emu_retrieve_surface(method):
    sc.check_retrieve_surface(emu_scorer(method))


def test_topk_op_is_registered_and_refuses_cpu_tensors():
    import torch
    from shoeprint_image_retrieval_amd import _torch_ops

    ops = _torch_ops.load()
    assert str(ops.topk.default._schema) == "shoeprint_mi355x::topk(Tensor scores, int k) -> (Tensor, Tensor)"
    with pytest.raises(RuntimeError, match="must live in HBM"):
        ops.topk(torch.zeros(2, 3), 2)
