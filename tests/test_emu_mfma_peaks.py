"""`not gpu`: the matrix-core pair kernels' peak form (spr_ncc_plan_enable_peaks, NccScorer(matrix_core_peaks=True)) on the
CPU-emulation build - the checks of mfma_peak_cases.py, which tests/test_gpu_mfma_peaks.py runs through the real library.  The
planted-peak cases plant every emu_stride-th position here (every row and column is still hit), all of them on the MI355X."""

import pytest

import mfma_map_cases as mm
import mfma_peak_cases as mp
import peak_cases as pc
from emu_util import emu_library, emu_scorer


def _ids(cases):
    return [c.id for c in cases]


def _host(method, storage, **kw):
    return emu_scorer(method, storage=storage, matrix_core_peaks=True, **kw)


def test_emu_mfma_peaks_default_refuses():
    mp.check_default_refuses(emu_scorer)


def test_emu_mfma_peaks_opt_in():
    mp.check_opt_in(emu_scorer)


@pytest.mark.parametrize("case", mm.PEAK_CASES, ids=_ids(mm.PEAK_CASES))
def test_emu_mfma_peaks_planted(case, monkeypatch):
    mp.check_planted(emu_scorer, case, monkeypatch, every_position=False)


@pytest.mark.parametrize("form", list(mm.FORMS))
@pytest.mark.parametrize("t,tiling", mp.TIE_CASES)
def test_emu_mfma_peaks_ties(t, tiling, form, monkeypatch):
    mp.check_ties(emu_scorer, t, tiling, form, monkeypatch)


@pytest.mark.parametrize("case", mp.INSTANCE_CASES, ids=_ids(mp.INSTANCE_CASES))
def test_emu_mfma_peaks_instance(case, monkeypatch):
    mp.check_instance(emu_scorer, case, monkeypatch)


@pytest.mark.parametrize("method,dtype", mp.RULE_SCORERS)
def test_emu_mfma_peaks_accumulate_rule(method, dtype):
    mp.check_accumulate_rule(emu_scorer, method, dtype)


@pytest.mark.parametrize("method,dtype", mp.RULE_SCORERS)
def test_emu_mfma_peaks_edges(method, dtype, monkeypatch):
    mp.check_edges(emu_scorer, monkeypatch, method, dtype, n_items=30)


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_emu_mfma_peaks_planted_matrix(method, storage):
    mp.check_planted_matrix(_host(method, storage))


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_emu_mfma_peaks_ragged(method, storage):
    mp.check_ragged(_host(method, storage))


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_emu_mfma_peaks_located_variants(method, storage):
    mp.check_located_variants(_host(method, storage))


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_emu_mfma_peaks_second_pass_counts(method, storage, monkeypatch):
    mp.check_second_pass_counts(emu_scorer, method, storage, monkeypatch)


@pytest.mark.parametrize("method,storage", mp.HOST_SCORERS)
def test_emu_mfma_peaks_call_counts(method, storage, monkeypatch):
    pc.check_call_counts(lambda **kw: _host(method, storage, **kw), monkeypatch, ("score_matrix_located", "locate"))


def test_emu_mfma_peaks_config_key():
    from host_device import HostDevice
    from shoeprint_image_retrieval_amd.similarity import scorer_from_config

    dev = HostDevice()
    mp.check_config_key(lambda cfg: scorer_from_config(cfg, device=dev, library=emu_library()))
