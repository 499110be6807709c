"""`gpu`: every pixel of the FFT NCC maps and the planted-peak sweeps (ncc_map_cases.py) on an MI355X through the C ABI -
each of the twelve kernel instances, both variants, the three 1/sigma paths of the gallery prep.  What the emulation cannot
reproduce is checked here: the barrier-free wave exchanges, the buffer loads and the LDS layouts."""

import pytest

import ncc_map_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scorer():
    from shoeprint_image_retrieval_amd import _lib
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    lib = _lib.load_library()  # raises if the in-tree .so is missing: no fallback
    return lambda method: NccScorer(method=method, library=lib, crop=0)


def _ids(cases):
    return [c.id if hasattr(c, "id") else c[1].id for c in cases]


def test_ncc_maps_case_table(scorer, monkeypatch):
    mc.check_case_table(scorer, monkeypatch, mc.ALL_CASES)


@pytest.mark.parametrize("case", mc.BASE_CASES, ids=_ids(mc.BASE_CASES))
def test_ncc_maps(scorer, case, monkeypatch):
    mc.check_maps(scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mc.POW2_CASES, ids=_ids(mc.POW2_CASES))
def test_ncc_maps_pow2(scorer, case, monkeypatch):
    mc.check_maps(scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mc.STORAGE_CASES, ids=_ids(mc.STORAGE_CASES))
def test_ncc_maps_16bit_storage(scorer, case, monkeypatch):
    mc.check_maps(scorer, case, monkeypatch)


@pytest.mark.parametrize("pair", mc.BOUNDARY_PAIRS, ids=_ids(mc.BOUNDARY_PAIRS))
def test_ncc_maps_variant_boundary(scorer, pair, monkeypatch):
    mc.check_boundary_pair(scorer, pair, monkeypatch)


@pytest.mark.parametrize("pair", mc.FORCE_BIG_CASES, ids=_ids(mc.FORCE_BIG_CASES))
def test_ncc_maps_forced_workspace(scorer, pair, monkeypatch):
    mc.check_force_big(scorer, pair, monkeypatch)


_DIRECT = [c for c in mc.BASE_CASES if not c.env]


@pytest.mark.parametrize("case", _DIRECT, ids=_ids(_DIRECT))
def test_ncc_maps_direct(scorer, case, monkeypatch):
    mc.check_direct(scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mc.SWEEP_CASES, ids=_ids(mc.SWEEP_CASES))
def test_ncc_sweep(scorer, case, monkeypatch):
    mc.check_sweep(scorer, case, monkeypatch)
