"""`not gpu`: spr_ncc_score_peaks and its host mirror (score_matrix_located, the fused similarity.retrieve) on the
CPU-emulation build - the checks of peak_cases.py, which tests/test_gpu_peaks.py runs through the real library."""

import os
import subprocess
import sys

import pytest

import ncc_map_cases as mc
import peak_cases as pc
import shortlist_cases as sc
from emu_util import emu_scorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scorer(method):
    return emu_scorer(method, crop=0)


def _ids(cases):
    return [c.id for c in cases]


_SWEEPS = mc.for_emu(mc.SWEEP_CASES)


@pytest.mark.parametrize("case", _SWEEPS, ids=_ids(_SWEEPS))
def test_emu_peaks_sweep(case, monkeypatch):
    pc.check_sweep(_scorer, case, monkeypatch)


@pytest.mark.parametrize("t,i", pc.DIRECT_SWEEPS)
def test_emu_peaks_sweep_direct(t, i, monkeypatch):
    pc.check_sweep(_scorer, pc.direct_sweep_case(t, i), monkeypatch, method="direct")


_INSTANCES = mc.for_emu(pc.INSTANCE_CASES)


@pytest.mark.parametrize("case", _INSTANCES, ids=_ids(_INSTANCES))
def test_emu_peaks_instance(case, monkeypatch):
    pc.check_instance(_scorer, case, monkeypatch)


_DIRECT = [c for c in _INSTANCES if c.direct and not c.env and c.method == "fft"]


@pytest.mark.parametrize("case", _DIRECT, ids=_ids(_DIRECT))
def test_emu_peaks_instance_direct(case, monkeypatch):
    pc.check_instance(_scorer, case, monkeypatch, method="direct")


MATRIX = [("fft", 0), ("fft_pow2", 0), ("direct", 0), ("fft", 1), ("fft_pow2", 1), ("direct", 1), ("fft", 2), ("fft_pow2", 2), ("direct", 2)]


@pytest.mark.parametrize("method,case", MATRIX)
def test_emu_peaks_planted_matrix(method, case):
    pc.check_planted_matrix(emu_scorer(method), sc.PLANTED_CASES[case])


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_emu_peaks_accumulate_rule(method):
    pc.check_accumulate_rule(_scorer, method)


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_emu_peaks_located_variants(method):
    pc.check_located_variants(emu_scorer(method))


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_emu_peaks_ragged(method):
    pc.check_ragged(emu_scorer(method))


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_emu_peaks_no_second_pass(method, monkeypatch):
    pc.check_no_second_pass(emu_scorer(method), monkeypatch)


def test_emu_peaks_mfma_keeps_the_second_pass(monkeypatch):
    pc.check_mfma_keeps_the_second_pass(emu_scorer("mfma", storage="bfloat16"), monkeypatch)


@pytest.mark.parametrize("method,storage,counted", pc.CALL_COUNT_SCORERS, ids=[c[0] for c in pc.CALL_COUNT_SCORERS])
def test_emu_peaks_call_counts(method, storage, counted, monkeypatch):
    pc.check_call_counts(lambda **kw: emu_scorer(method, storage=storage, **kw), monkeypatch, counted)


def test_emu_peaks_plan_has_peaks():
    pc.check_has_peaks(_scorer)


@pytest.mark.parametrize("method,t,i,n", pc.EDGE_SHAPES)
def test_emu_peaks_edges(method, t, i, n, monkeypatch):
    pc.check_edges(_scorer, monkeypatch, method, t, i, n)


def test_emu_peaks_reverse_work_item_order():
    """The planted-peak sweeps of three kernels and the accumulate rule with the work-items of a workgroup run from the last
    to the first (SPR_EMU_ORDER=reverse, fixed when the emulation starts: a process of its own): the same planted pixels and
    the same bits as spr_ncc_score."""
    env = dict(os.environ, SPR_EMU_ORDER="reverse")
    sel = "(peaks_sweep and not direct and not TEAM and not FORCE_BIG and (32x16 or 96x48 or 192x96-6)) or accumulate_rule"
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", sel],
                       env=env, capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode == 0 and "5 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]  # three sweeps, two accumulate rules


def test_located_op_is_registered_and_refuses_cpu_tensors():
    import torch
    from shoeprint_image_retrieval_amd import _torch_ops

    ops = _torch_ops.load()
    assert str(ops.ncc_scores_located.default._schema) == pc.SCHEMA
    with pytest.raises(RuntimeError, match="must live in HBM"):
        ops.ncc_scores_located(torch.zeros(2, 3, 8, 6), torch.zeros(2, 3, 16, 8))
