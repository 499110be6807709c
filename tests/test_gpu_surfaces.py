"""`gpu`: spr_ncc_score_surfaces, spr_surface_peaks, spr_maps_mean, NccScorer.pair_surfaces,
similarity.retrieve(..., surfaces=True) and torch.ops.shoeprint_mi355x.surface_peaks on the MI355X - the checks of
surface_cases.py through the real library (tests/test_emu_surfaces.py runs them on the emulation)."""

import numpy as np
import pytest

import score_list_cases as lc
import shortlist_cases as sc_cases
import surface_cases as sv

pytestmark = pytest.mark.gpu


def make_scorer(method="auto", **kw):
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    return NccScorer(method=method, **kw)


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_surfaces_equal_list(case):
    sv.check_siblings(make_scorer, case)


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_surfaces_against_the_oracle(case):
    sv.check_oracle(make_scorer, case)


def test_surfaces_anticorrelated_pair():
    sv.check_anticorrelated(make_scorer)


@pytest.mark.parametrize("n_variants", [2, 3])
@pytest.mark.parametrize("case", [lc.SMALL, lc.CASES[11], lc.CASES[14]], ids=lambda c: c.id)
def test_surfaces_accumulate(case, n_variants):
    sv.check_accumulate(make_scorer, case, n_variants)


@pytest.mark.parametrize("case", [lc.SMALL, lc.CASES[12], lc.CASES[14]], ids=lambda c: c.id)
def test_surfaces_slicing(monkeypatch, case):
    sv.check_slicing(make_scorer, monkeypatch, case)


def test_surfaces_arguments(monkeypatch):
    sv.check_arguments(make_scorer, monkeypatch)


@pytest.fixture(scope="module")
def fft_scorer():
    return make_scorer("fft")


@pytest.mark.parametrize("hw", sv.PEAK_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_surface_peaks(fft_scorer, hw):
    sv.check_surface_peaks(fft_scorer, hw)


def test_surface_peaks_edges(fft_scorer):
    sv.check_surface_peaks_edges(fft_scorer)


@pytest.mark.parametrize("hw", [(28, 12), (124, 60)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_surface_peaks_torch_op(fft_scorer, hw):
    """torch.ops.shoeprint_mi355x.surface_peaks against the ctypes route, bit for bit (``surface_peaks_device`` takes the op
    when it is built: here both are called by name)."""
    import torch

    from shoeprint_image_retrieval_amd import _torch_ops

    ops = _torch_ops.load()
    surfaces = sv.peak_surfaces(*hw)
    dev = fft_scorer.dev
    for n_peaks, (ry, rx) in ((1, (0, 0)), (3, (hw[0] // 5, hw[1] // 5)), (8, hw)):
        want = sv.run_surface_peaks(fft_scorer, surfaces, n_peaks, ry, rx)
        got = ops.surface_peaks(dev.to_device(np.array(surfaces)), n_peaks, ry, rx)
        assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.float32]
        sv.assert_same_bits(dev.to_host(got[0]), want[0], "torch op: values")
        np.testing.assert_array_equal(dev.to_host(got[1]), want[1])
        sv.assert_same_bits(dev.to_host(got[2]), want[2], "torch op: psr")
        mirror = fft_scorer.surface_peaks_device(dev.to_device(np.array(surfaces)), n_peaks, ry, rx)
        sv.assert_same_bits(dev.to_host(mirror[0]), want[0], "surface_peaks_device: values")
        np.testing.assert_array_equal(dev.to_host(mirror[1]), want[1])
        sv.assert_same_bits(dev.to_host(mirror[2]), want[2], "surface_peaks_device: psr")
    empty = ops.surface_peaks(dev.to_device(np.zeros((0, 3, 4), np.float32)), 2, 1, 1)
    assert [tuple(t.shape) for t in empty] == [(0, 2), (0, 2), (0,)]
    with pytest.raises(RuntimeError):
        ops.surface_peaks(dev.to_device(np.zeros((1, 3, 4), np.float32)), 9, 1, 1)


@pytest.mark.parametrize("shape", sc_cases.PEAK_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_maps_mean(fft_scorer, shape):
    sv.check_maps_mean(fft_scorer, shape)


def test_maps_mean_arguments(fft_scorer):
    sv.check_maps_mean_arguments(fft_scorer)


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_pair_surfaces_equal_score_pairs(method):
    sv.check_pair_surfaces_list_route(make_scorer(method))


def test_pair_surfaces_of_feature_sets(fft_scorer):
    from shoeprint_image_retrieval_amd.features import FeatureSet

    q, g = lc.ragged_sets()
    sv.check_pair_surfaces_list_route(fft_scorer, sides=(FeatureSet.from_host(fft_scorer.dev, q), FeatureSet.from_host(fft_scorer.dev, g)))
    sv.check_pair_surfaces_list_route(fft_scorer, sides=(q, FeatureSet.from_host(fft_scorer.dev, g)), rot=None, sc=None)


def test_pair_surfaces_matrix_core_block():
    sv.check_pair_surfaces_matrix_cores(make_scorer)


def test_pair_surfaces_workspace_instance(monkeypatch):
    monkeypatch.setenv("SPR_NCC_FORCE_BIG", "1")
    sc = make_scorer("fft")
    pairs, got = sv.check_pair_surfaces(sc, rot=[180], sc=None)
    assert sc._plans and all(not p.has_surfaces for p in sc._plans.values())
    score, variant, yx = sc.locate(*lc.ragged_sets(), pairs, rotations=[180])
    for k in range(len(pairs)):
        if got[0][k] > 0 and got[1][k] == variant[k]:  # (the kernels' float32 arg-max and locate's float64 one may differ)
            sv.assert_same_bits(got[4][k].max(), score[k], f"workspace instance, entry {k}: the fallback's maximum against locate")


@pytest.mark.parametrize("case", sc_cases.PLANTED_CASES, ids=str)
def test_retrieve_surfaces(fft_scorer, case):
    sv.check_retrieve_surfaces(fft_scorer, case)


def test_retrieve_surfaces_variants(fft_scorer):
    sv.check_retrieve_surfaces_variants(fft_scorer)
