"""`gpu`: the matrix-core pair kernels' peak form (spr_ncc_plan_enable_peaks, NccScorer(matrix_core_peaks=True)) through the
real gfx950 library on an MI355X - the checks of mfma_peak_cases.py (which tests/test_emu_mfma_peaks.py runs on the
CPU-emulation build), with every position of the frame planted."""

import pytest

import mfma_map_cases as mm
import mfma_peak_cases as mp
import peak_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()  # raises if the in-tree .so is missing: no fallback


@pytest.fixture(scope="module")
def scorer(lib):
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    def make(method="auto", **kw):
        s = NccScorer(method=method, library=lib, **kw)
        s._ops_cache = None  # the ctypes route: the entry points are counted on the library object
        return s

    return make


def _ids(cases):
    return [c.id for c in cases]


def test_mfma_peaks_default_refuses(scorer):
    mp.check_default_refuses(scorer)


def test_mfma_peaks_opt_in(scorer):
    mp.check_opt_in(scorer)


@pytest.mark.parametrize("case", mm.PEAK_CASES, ids=_ids(mm.PEAK_CASES))
def test_mfma_peaks_planted(scorer, case, monkeypatch):
    mp.check_planted(scorer, case, monkeypatch, every_position=True)


@pytest.mark.parametrize("form", list(mm.FORMS))
@pytest.mark.parametrize("t,tiling", mp.TIE_CASES)
def test_mfma_peaks_ties(scorer, t, tiling, form, monkeypatch):
    mp.check_ties(scorer, t, tiling, form, monkeypatch)


@pytest.mark.parametrize("case", mp.INSTANCE_CASES, ids=_ids(mp.INSTANCE_CASES))
def test_mfma_peaks_instance(scorer, case, monkeypatch):
    mp.check_instance(scorer, case, monkeypatch)


@pytest.mark.parametrize("method,dtype", mp.RULE_SCORERS)
def test_mfma_peaks_accumulate_rule(scorer, method, dtype):
    mp.check_accumulate_rule(scorer, method, dtype)


@pytest.mark.parametrize("method,dtype", mp.RULE_SCORERS)
def test_mfma_peaks_edges(scorer, method, dtype, monkeypatch):
    mp.check_edges(scorer, monkeypatch, method, dtype)


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_mfma_peaks_planted_matrix(scorer, method, storage):
    mp.check_planted_matrix(scorer(method, storage=storage, matrix_core_peaks=True))


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_mfma_peaks_ragged(scorer, method, storage):
    mp.check_ragged(scorer(method, storage=storage, matrix_core_peaks=True))


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_mfma_peaks_located_variants(scorer, method, storage):
    mp.check_located_variants(scorer(method, storage=storage, matrix_core_peaks=True))


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_mfma_peaks_second_pass_counts(scorer, method, storage, monkeypatch):
    mp.check_second_pass_counts(scorer, method, storage, monkeypatch)


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_mfma_peaks_call_counts(scorer, method, storage, monkeypatch):
    pc.check_call_counts(lambda **kw: scorer(method, storage=storage, matrix_core_peaks=True, **kw), monkeypatch,
                         ("score_matrix_located", "locate"))


def test_mfma_peaks_config_key(lib):
    from shoeprint_image_retrieval_amd.similarity import scorer_from_config

    mp.check_config_key(lambda cfg: scorer_from_config(cfg, library=lib))
