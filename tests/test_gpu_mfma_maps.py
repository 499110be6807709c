"""`gpu`: every pixel of the matrix-core NCC maps, the planted-peak score matrices at all 336 positions of the frame and the
guard-band / fill-invariance runs of all scorer methods (mfma_map_cases.py) on an MI355X through the C ABI.  What the
emulation cannot reproduce is checked here: the matrix cores' own accumulation order, the buffer loads of the query block,
the LDS image of the Toeplitz gather - and device memory that nobody poisoned."""

import pytest

import mfma_map_cases as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scorer():
    from shoeprint_image_retrieval_amd import _lib
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    lib = _lib.load_library()  # raises if the in-tree .so is missing: no fallback
    return lambda method, crop=0: NccScorer(method=method, library=lib, crop=crop)


def _ids(cases):
    return [c.id for c in cases]


def test_mfma_maps_case_table(scorer, monkeypatch):
    mm.check_case_table(scorer, monkeypatch, mm.ALL_MAP_CASES + [c.map_case() for c in mm.PEAK_CASES])


@pytest.mark.parametrize("case", mm.MAP_CASES, ids=_ids(mm.MAP_CASES))
def test_mfma_maps(scorer, case, monkeypatch):
    mm.check_maps(scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mm.WIDE_CASES, ids=_ids(mm.WIDE_CASES))
def test_mfma_maps_17_channels(scorer, case, monkeypatch):
    mm.check_maps(scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mm.PREP_CASES, ids=_ids(mm.PREP_CASES))
def test_mfma_maps_prep_kernels(scorer, case, monkeypatch):
    mm.check_maps(scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mm.OFFSET_CASES, ids=_ids(mm.OFFSET_CASES))
def test_mfma_maps_on_offsets(scorer, case, monkeypatch):
    mm.check_maps(scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mm.PEAK_CASES, ids=_ids(mm.PEAK_CASES))
def test_mfma_planted_peaks(scorer, case, monkeypatch):
    mm.check_peaks(scorer, case, monkeypatch, every_position=True)


@pytest.mark.parametrize("case", mm.GUARD_CASES, ids=_ids(mm.GUARD_CASES))
def test_scorer_guard_bands(scorer, case, monkeypatch):
    mm.check_guarded(scorer, case, monkeypatch)
