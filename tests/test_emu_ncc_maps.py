"""`not gpu`: every pixel of the FFT NCC maps and the planted-peak sweeps (ncc_map_cases.py) on the CPU emulation of the
kernels - each of the twelve kernel instances, both variants, the three 1/sigma paths of the gallery prep."""

import os

import pytest

import ncc_map_cases as mc
from emu_util import emu_scorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scorer(method):
    return emu_scorer(method, crop=0)


def _ids(cases):
    return [c.id if hasattr(c, "id") else c[1].id for c in cases]


def test_emu_ncc_maps_case_table(monkeypatch):
    mc.check_case_table(_scorer, monkeypatch, mc.ALL_CASES)


@pytest.mark.parametrize("case", mc.for_emu(mc.BASE_CASES), ids=_ids(mc.for_emu(mc.BASE_CASES)))
def test_emu_ncc_maps(case, monkeypatch):
    mc.check_maps(_scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mc.POW2_CASES, ids=_ids(mc.POW2_CASES))
def test_emu_ncc_maps_pow2(case, monkeypatch):
    mc.check_maps(_scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mc.STORAGE_CASES, ids=_ids(mc.STORAGE_CASES))
def test_emu_ncc_maps_16bit_storage(case, monkeypatch):
    mc.check_maps(_scorer, case, monkeypatch)


@pytest.mark.parametrize("pair", mc.BOUNDARY_PAIRS, ids=_ids(mc.BOUNDARY_PAIRS))
def test_emu_ncc_maps_variant_boundary(pair, monkeypatch):
    mc.check_boundary_pair(_scorer, pair, monkeypatch)


@pytest.mark.parametrize("pair", mc.FORCE_BIG_CASES, ids=_ids(mc.FORCE_BIG_CASES))
def test_emu_ncc_maps_forced_workspace(pair, monkeypatch):
    mc.check_force_big(_scorer, pair, monkeypatch)


_DIRECT = [c for c in mc.for_emu(mc.BASE_CASES) if not c.env]


@pytest.mark.parametrize("case", _DIRECT, ids=_ids(_DIRECT))
def test_emu_ncc_maps_direct(case, monkeypatch):
    mc.check_direct(_scorer, case, monkeypatch)


@pytest.mark.parametrize("case", mc.for_emu(mc.SWEEP_CASES), ids=_ids(mc.for_emu(mc.SWEEP_CASES)))
def test_emu_ncc_sweep(case, monkeypatch):
    mc.check_sweep(_scorer, case, monkeypatch)


def test_emu_ncc_maps_reverse_work_item_order():
    """The map and sweep tests of this file once more with the work-items of a workgroup run in descending order
    (SPR_EMU_ORDER=reverse, see test_emu_kernels.test_emu_reverse_work_item_order): a data race between work-items that
    the ascending order happens to resolve the right way must not hide behind it."""
    import subprocess
    import sys

    env = dict(os.environ, SPR_EMU_ORDER="reverse")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "(ncc_maps or ncc_sweep) and not reverse"],
                       env=env, capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
