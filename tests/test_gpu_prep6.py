"""`gpu`: the pipelined corner-sum gallery preparation (csrc/ncc_prep6.hip) against prep_fft_kernel on an MI355X - byte-identical
spectra and dead flags, 1/sigma within one float32 step, poison guard bands on both sides of the prepared buffer untouched;
3 items x 5 channels (a partial channel group) and 2 items x 256 channels (32 full groups per item)."""

import pytest

import prep6_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    from shoeprint_image_retrieval_amd import _lib
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    lib = _lib.load_library()  # raises if the in-tree .so is missing: no fallback
    return lambda: NccScorer(method="fft", library=lib)


@pytest.mark.parametrize("storage", ["float32", "float16", "bfloat16"])
def test_prep6_matches_table_kernel_3x5(make, monkeypatch, storage):
    pc.check_same_preparation(make, monkeypatch, 3, 5, (128, 64), storage)


def test_prep6_matches_table_kernel_2x256(make, monkeypatch):
    pc.check_same_preparation(make, monkeypatch, 2, 256, (128, 64), "float32")


def test_prep6_smaller_map_same_grid(make, monkeypatch):
    pc.check_same_preparation(make, monkeypatch, 2, 3, (124, 60), "float32")


def test_prep6_smaller_template_falls_back(make, monkeypatch):
    pc.check_smaller_template_falls_back(make, monkeypatch)


def test_prep6_scores_against_oracle(make, monkeypatch):
    pc.check_scores(make, monkeypatch)
