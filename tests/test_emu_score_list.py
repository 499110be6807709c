"""`not gpu`: spr_ncc_score_list, NccScorer.score_pairs and similarity.retrieve_cascade on the CPU-emulation build - the checks
of score_list_cases.py, which tests/test_gpu_score_list.py runs through the real library - and the two configuration keys."""

import os
import subprocess
import sys

import numpy as np
import pytest

import score_list_cases as lc
import shortlist_cases as sc_cases
from emu_util import emu_scorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_emu_list_equals_dense(case):
    lc.check_instance(emu_scorer, case)


@pytest.mark.parametrize("case", [lc.SMALL, lc.CASES[11], lc.CASES[14]], ids=lambda c: c.id)
def test_emu_list_accumulate(case):
    lc.check_accumulate(emu_scorer, case)


@pytest.mark.parametrize("case", [lc.SMALL, lc.CASES[12], lc.CASES[14]], ids=lambda c: c.id)
def test_emu_list_slicing(monkeypatch, case):
    lc.check_slicing(emu_scorer, monkeypatch, case)


def test_emu_list_arguments(monkeypatch):
    lc.check_arguments(emu_scorer, monkeypatch)


def test_emu_list_reverse_work_item_order():
    """The list cases with the work-items of a workgroup run from the last to the first (SPR_EMU_ORDER=reverse, fixed when the
    emulation starts: a process of its own): the same bits."""
    env = dict(os.environ, SPR_EMU_ORDER="reverse")
    sel = "list_equals_dense or list_accumulate"
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", sel],
                       env=env, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("method,case", [("fft", 0), ("direct", 0), ("fft", 1), ("fft", 2), ("fft_pow2", 2)])
def test_emu_score_pairs_against_the_oracle(method, case):
    lc.check_planted_against_oracle(emu_scorer(method), sc_cases.PLANTED_CASES[case])


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_emu_score_pairs_equals_located_cells(method):
    sc = emu_scorer(method)
    lc.check_score_pairs(sc)
    lc.check_score_pairs_surface(sc)


def test_emu_score_pairs_of_feature_sets():
    from shoeprint_image_retrieval_amd.features import FeatureSet

    sc = emu_scorer("fft")
    q, g = lc.ragged_sets()
    lc.check_score_pairs(sc, sides=(FeatureSet.from_host(sc.dev, q), FeatureSet.from_host(sc.dev, g)))
    lc.check_score_pairs(sc, sides=(q, FeatureSet.from_host(sc.dev, g)), rot=None, sc=None)


def test_emu_score_pairs_gallery_chunks():
    sc = emu_scorer("fft")
    q, g = lc.ragged_sets()
    plan = sc.plan(5, (18, 12), (18, 12))
    sc.max_prepared_bytes = plan.gallery_item_bytes  # one item per chunk: three and two chunks for the two gallery classes
    lc.check_score_pairs(sc)
    assert sc.last_chunk_items == 1


def test_emu_score_pairs_fallbacks(monkeypatch):
    """Blocks whose plans have no list form: the matrix-core method without and with its peak form, the workspace instance."""
    rng = np.random.default_rng(12)
    q = [rng.random((4, 32, 16), dtype=np.float32) for _ in range(3)]
    g = [rng.random((4, 32, 16), dtype=np.float32) for _ in range(4)]
    bf = lambda items: [lc.synth.from_bfloat16_bits(lc.synth.bfloat16_bits(a)) for a in items]
    for kw in ({}, {"matrix_core_peaks": True}):
        sc = emu_scorer("mfma", storage="bfloat16", **kw)
        lc.check_score_pairs(sc, bf(q), bf(g), rot=[180], sc=None)
        assert not sc.plan(4, (32, 16), (32, 16), dtype="bfloat16").has_list
    monkeypatch.setenv("SPR_NCC_FORCE_BIG", "1")
    sc = emu_scorer("fft")
    lc.check_score_pairs(sc, rot=[180], sc=None)
    assert sc._plans and all(p.method == lc._lib.NCC_FFT and not p.has_list for p in sc._plans.values())


@pytest.fixture(scope="module")
def fft_scorer():
    return emu_scorer("fft")


@pytest.mark.parametrize("depth", [12, 256])
def test_emu_cascade_full_depth(fft_scorer, depth):
    lc.check_cascade_full_depth(fft_scorer, depth)


def test_emu_cascade_short_depth(fft_scorer):
    lc.check_cascade_short_depth(fft_scorer)


def test_emu_cascade_located(fft_scorer):
    lc.check_cascade_located(fft_scorer)


def test_emu_cascade_errors(fft_scorer):
    lc.check_cascade_errors(fft_scorer)


def test_cascade_config_keys():
    from shoeprint_image_retrieval_amd.config import MI355X_DEFAULTS, normalise

    assert MI355X_DEFAULTS["cascade_blocks"] == [] and MI355X_DEFAULTS["cascade_depth"] == 100
    got = normalise({})["mi355x"]
    assert got["cascade_blocks"] == [] and got["cascade_depth"] == 100
    model = {"type": "VGG16"}
    got = normalise({"model": dict(model), "mi355x": {"cascade_blocks": [9, 16], "cascade_depth": 256, "shortlist": 256}})["mi355x"]
    assert got["cascade_blocks"] == [9, 16] and got["cascade_depth"] == 256
    assert normalise({"model": dict(model), "mi355x": {"cascade_blocks": [9], "cascade_depth": 1}})["mi355x"]["cascade_depth"] == 1
    assert normalise({"mi355x": {"cascade_depth": 5, "shortlist": 9}})["mi355x"]["shortlist"] == 9  # (no cascade: no bound)
    for bad in (0, 257, -3, 2.5, "3", True, None):
        with pytest.raises(ValueError, match="cascade_depth"):
            normalise({"mi355x": {"cascade_depth": bad}})
    for bad in (9, "9", [9.0], [True], None):
        with pytest.raises(ValueError, match="cascade_blocks"):
            normalise({"model": dict(model), "mi355x": {"cascade_blocks": bad}})
    with pytest.raises(ValueError, match="cascade_blocks.*not feature taps"):
        normalise({"model": dict(model), "mi355x": {"cascade_blocks": [10]}})
    with pytest.raises(ValueError, match="cascade_blocks with fuse_blocks"):
        normalise({"model": dict(model), "mi355x": {"cascade_blocks": [9], "fuse_blocks": [9]}})
    with pytest.raises(ValueError, match="cascade_blocks with gallery_cache"):
        normalise({"model": dict(model), "mi355x": {"cascade_blocks": [9], "gallery_cache": "/tmp/x"}})
    with pytest.raises(ValueError, match="cascade_depth"):
        normalise({"model": dict(model), "mi355x": {"cascade_blocks": [9], "cascade_depth": 5, "shortlist": 6}})
    # fuse_blocks alone is what it was
    assert normalise({"model": dict(model), "mi355x": {"fuse_blocks": [9]}})["mi355x"]["fuse_blocks"] == [9]
    with pytest.raises(ValueError, match="fuse_blocks with shortlist"):
        normalise({"model": dict(model), "mi355x": {"fuse_blocks": [9], "shortlist": 2}})
