"""`not gpu`: every pixel of the matrix-core NCC maps, the planted-peak score matrices and the guard-band / fill-invariance
runs of all scorer methods (mfma_map_cases.py) on the CPU emulation of the kernels.  The planted peaks take every 7th
position of the frame here (every row and every column); the MI355X runner takes all of them."""

import pytest

import mfma_map_cases as mm
from emu_util import emu_scorer


def _scorer(method, crop=0):
    return emu_scorer(method, crop=crop)


def _ids(cases):
    return [c.id for c in cases]


def test_emu_mfma_maps_case_table(monkeypatch):
    mm.check_case_table(_scorer, monkeypatch, mm.ALL_MAP_CASES + [c.map_case() for c in mm.PEAK_CASES])


@pytest.mark.parametrize("case", mm.MAP_CASES, ids=_ids(mm.MAP_CASES))
def test_emu_mfma_maps(case, monkeypatch):
    mm.check_maps(_scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mm.WIDE_CASES, ids=_ids(mm.WIDE_CASES))
def test_emu_mfma_maps_17_channels(case, monkeypatch):
    mm.check_maps(_scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mm.PREP_CASES, ids=_ids(mm.PREP_CASES))
def test_emu_mfma_maps_prep_kernels(case, monkeypatch):
    mm.check_maps(_scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mm.OFFSET_CASES, ids=_ids(mm.OFFSET_CASES))
def test_emu_mfma_maps_on_offsets(case, monkeypatch):
    mm.check_maps(_scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mm.PEAK_CASES, ids=_ids(mm.PEAK_CASES))
def test_emu_mfma_planted_peaks(case, monkeypatch):
    mm.check_peaks(_scorer, case, monkeypatch, every_position=False)


@pytest.mark.parametrize("case", mm.for_emu(mm.GUARD_CASES), ids=_ids(mm.for_emu(mm.GUARD_CASES)))
def test_emu_scorer_guard_bands(case, monkeypatch):
    mm.check_guarded(_scorer, case, monkeypatch)
