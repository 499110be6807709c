"""`not gpu`: spr_ncc_score_surfaces, spr_surface_peaks, spr_maps_mean, NccScorer.pair_surfaces and
similarity.retrieve(..., surfaces=True) on the CPU-emulation build - the checks of surface_cases.py, which
tests/test_gpu_surfaces.py runs through the real library."""

import pytest

import score_list_cases as lc
import shortlist_cases as sc_cases
import surface_cases as sv
from emu_util import emu_scorer


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_emu_surfaces_equal_list(case):
    sv.check_siblings(emu_scorer, case)


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_emu_surfaces_against_the_oracle(case):
    sv.check_oracle(emu_scorer, case)


def test_emu_surfaces_anticorrelated_pair():
    sv.check_anticorrelated(emu_scorer)


@pytest.mark.parametrize("n_variants", [2, 3])
@pytest.mark.parametrize("case", [lc.SMALL, lc.CASES[11], lc.CASES[14]], ids=lambda c: c.id)
def test_emu_surfaces_accumulate(case, n_variants):
    sv.check_accumulate(emu_scorer, case, n_variants)


@pytest.mark.parametrize("case", [lc.SMALL, lc.CASES[12], lc.CASES[14]], ids=lambda c: c.id)
def test_emu_surfaces_slicing(monkeypatch, case):
    sv.check_slicing(emu_scorer, monkeypatch, case)


def test_emu_surfaces_arguments(monkeypatch):
    sv.check_arguments(emu_scorer, monkeypatch)


@pytest.fixture(scope="module")
def fft_scorer():
    return emu_scorer("fft")


@pytest.mark.parametrize("hw", sv.PEAK_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_emu_surface_peaks(fft_scorer, hw):
    sv.check_surface_peaks(fft_scorer, hw)


def test_emu_surface_peaks_edges(fft_scorer):
    sv.check_surface_peaks_edges(fft_scorer)


@pytest.mark.parametrize("shape", sc_cases.PEAK_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_emu_maps_mean(fft_scorer, shape):
    sv.check_maps_mean(fft_scorer, shape)


def test_emu_maps_mean_arguments(fft_scorer):
    sv.check_maps_mean_arguments(fft_scorer)


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_emu_pair_surfaces_equal_score_pairs(method):
    sv.check_pair_surfaces_list_route(emu_scorer(method))


def test_emu_pair_surfaces_of_feature_sets(fft_scorer):
    from shoeprint_image_retrieval_amd.features import FeatureSet

    q, g = lc.ragged_sets()
    sv.check_pair_surfaces_list_route(fft_scorer, sides=(FeatureSet.from_host(fft_scorer.dev, q), FeatureSet.from_host(fft_scorer.dev, g)))
    sv.check_pair_surfaces_list_route(fft_scorer, sides=(q, FeatureSet.from_host(fft_scorer.dev, g)), rot=None, sc=None)


def test_emu_pair_surfaces_matrix_core_block():
    sv.check_pair_surfaces_matrix_cores(emu_scorer)


def test_emu_pair_surfaces_workspace_instance(monkeypatch):
    monkeypatch.setenv("SPR_NCC_FORCE_BIG", "1")
    sc = emu_scorer("fft")
    pairs, got = sv.check_pair_surfaces(sc, rot=[180], sc=None)
    assert sc._plans and all(not p.has_surfaces for p in sc._plans.values())
    score, variant, yx = sc.locate(*lc.ragged_sets(), pairs, rotations=[180])
    for k in range(len(pairs)):
        if got[0][k] > 0 and got[1][k] == variant[k]:  # (the kernels' float32 arg-max and locate's float64 one may differ)
            sv.assert_same_bits(got[4][k].max(), score[k], f"workspace instance, entry {k}: the fallback's maximum against locate")


@pytest.mark.parametrize("case", sc_cases.PLANTED_CASES, ids=str)
def test_emu_retrieve_surfaces(fft_scorer, case):
    sv.check_retrieve_surfaces(fft_scorer, case)


def test_emu_retrieve_surfaces_variants(fft_scorer):
    sv.check_retrieve_surfaces_variants(fft_scorer)
