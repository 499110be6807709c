"""`gpu`: spr_ncc_score_list, NccScorer.score_pairs, similarity.retrieve_cascade and the run driver's cascade route on the
MI355X - the checks of score_list_cases.py through the real library (tests/test_emu_score_list.py runs them on the emulation)."""

import os
import re

import numpy as np
import pytest

import score_list_cases as lc
import shortlist_cases as sc_cases

pytestmark = pytest.mark.gpu


def make_scorer(method="auto", **kw):
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    return NccScorer(method=method, **kw)


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_list_equals_dense(case):
    lc.check_instance(make_scorer, case)


@pytest.mark.parametrize("case", [lc.SMALL, lc.CASES[11], lc.CASES[14]], ids=lambda c: c.id)
def test_list_accumulate(case):
    lc.check_accumulate(make_scorer, case)


@pytest.mark.parametrize("case", [lc.SMALL, lc.CASES[12], lc.CASES[14]], ids=lambda c: c.id)
def test_list_slicing(monkeypatch, case):
    lc.check_slicing(make_scorer, monkeypatch, case)


def test_list_arguments(monkeypatch):
    lc.check_arguments(make_scorer, monkeypatch)


@pytest.mark.parametrize("method,case", [("fft", 0), ("direct", 0), ("fft", 1), ("fft", 2), ("fft_pow2", 2)])
def test_score_pairs_against_the_oracle(method, case):
    lc.check_planted_against_oracle(make_scorer(method), sc_cases.PLANTED_CASES[case])


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_score_pairs_equals_located_cells(method):
    sc = make_scorer(method)
    lc.check_score_pairs(sc)
    lc.check_score_pairs_surface(sc)


def test_score_pairs_of_feature_sets():
    from shoeprint_image_retrieval_amd.features import FeatureSet

    sc = make_scorer("fft")
    q, g = lc.ragged_sets()
    lc.check_score_pairs(sc, sides=(FeatureSet.from_host(sc.dev, q), FeatureSet.from_host(sc.dev, g)))
    lc.check_score_pairs(sc, sides=(q, FeatureSet.from_host(sc.dev, g)), rot=None, sc=None)


def test_score_pairs_gallery_chunks():
    sc = make_scorer("fft")
    plan = sc.plan(5, (18, 12), (18, 12))
    sc.max_prepared_bytes = plan.gallery_item_bytes  # one item per chunk: three and two chunks for the two gallery classes
    lc.check_score_pairs(sc)
    assert sc.last_chunk_items == 1


def test_score_pairs_fallbacks(monkeypatch):
    """Blocks whose plans have no list form: the matrix-core method without and with its peak form, the workspace instance."""
    rng = np.random.default_rng(12)
    q = [rng.random((4, 32, 16), dtype=np.float32) for _ in range(3)]
    g = [rng.random((4, 32, 16), dtype=np.float32) for _ in range(4)]
    bf = lambda items: [lc.synth.from_bfloat16_bits(lc.synth.bfloat16_bits(a)) for a in items]
    for kw in ({}, {"matrix_core_peaks": True}):
        sc = make_scorer("mfma", storage="bfloat16", **kw)
        lc.check_score_pairs(sc, bf(q), bf(g), rot=[180], sc=None)
        assert not sc.plan(4, (32, 16), (32, 16), dtype="bfloat16").has_list
    monkeypatch.setenv("SPR_NCC_FORCE_BIG", "1")
    sc = make_scorer("fft")
    lc.check_score_pairs(sc, rot=[180], sc=None)
    assert sc._plans and all(p.method == lc._lib.NCC_FFT and not p.has_list for p in sc._plans.values())


@pytest.fixture(scope="module")
def fft_scorer():
    return make_scorer("fft")


@pytest.mark.parametrize("depth", [12, 256])
def test_cascade_full_depth(fft_scorer, depth):
    lc.check_cascade_full_depth(fft_scorer, depth)


def test_cascade_short_depth(fft_scorer):
    lc.check_cascade_short_depth(fft_scorer)


def test_cascade_located(fft_scorer):
    lc.check_cascade_located(fft_scorer)


def test_cascade_errors(fft_scorer):
    lc.check_cascade_errors(fft_scorer)


def _driver_toml(tmp_path, case, extra):
    return (f'[dataset]\ndir = "{tmp_path}"\ntype = "WVU2019"\ncrop = {case["crop"]}\nn_processes = 3\nn_clusters = 2\n'
            f'cluster_minimise_tolerance = 0.05\n[model]\ntype = "EfficientNetV2_M"\nclahe_clip_limit = 2.0\n'
            f'clahe_tile_grid_size = [8, 8]\nstart_block = 6\nend_block = 4\nskip_blocks = []\nminimum_dim = 120\nmaximum_dim = 200\n'
            f'[comparison]\nn_processes = 2\n[mi355x]\n' + extra)


def test_run_driver_cascade_blocks(tmp_path, capsys):
    """run_mi355x.main on wvu_split with the default model: without the keys the output is what cascade_blocks = [] gives, line
    for line; cascade_blocks = [4] at a depth beyond the gallery returns the ranks of fuse_blocks = [4]; with shortlist = 3
    every query is followed by its three best prints, the true match first where the rank is 1."""
    import dataset_util
    import run_mi355x

    case = next(c for c in dataset_util.CASES if c["name"] == "wvu_split")
    dataset_util.write_dataset(str(tmp_path), case)
    toml = tmp_path / "run.toml"

    def run(extra):
        toml.write_text(_driver_toml(tmp_path, case, extra))
        ranks = run_mi355x.main(str(toml))
        return ranks, capsys.readouterr().out

    plain_ranks, plain_out = run("")
    assert run("cascade_blocks = []\ncascade_depth = 7\n") == (plain_ranks, plain_out)
    assert "Cascade" not in plain_out
    fused_ranks, _ = run("fuse_blocks = [4]\n")
    got, out = run("cascade_blocks = [4]\ncascade_depth = 256\n")
    assert got == fused_ranks and len(got) == len(plain_ranks)
    assert out.count("Cascade: ") >= 1 and "feature layers [4, " in out
    got3, out3 = run("cascade_blocks = [4]\ncascade_depth = 256\nshortlist = 3\n")
    assert got3 == got
    lines = out3.splitlines()
    entry = re.compile(r"^    ([123])\. (\S+\.png)  score (\d\.\d{4})  (original|no variant)  offset \((-?\d+), (-?\d+)\)$")
    gallery, queries = sorted(case["gallery"]), sorted(case["query"])
    seen = 0
    for at, line in enumerate(lines):
        m = re.match(r"^Print (\d+) true match ranked (\d+)$", line)
        if not m:
            continue
        entries = [entry.match(lines[at + 1 + p]) for p in range(3)]
        assert all(entries), lines[at:at + 4]
        assert [e.group(1) for e in entries] == ["1", "2", "3"] and sorted(os.path.basename(e.group(2)) for e in entries) == gallery
        scores = [float(e.group(3)) for e in entries]
        assert scores == sorted(scores, reverse=True)
        assert not entry.match(lines[at + 4])
        seen += 1
    assert seen == len(got3) == len(queries)
    # where the rank is 1 the first name is the true match: ranks come cluster by cluster, as the loader orders the queries
    from shoeprint_image_retrieval_amd.config import load_config
    from shoeprint_image_retrieval_amd.dataloader import Dataloader

    firsts = [os.path.basename(entry.match(lines[at + 1]).group(2)) for at, line in enumerate(lines) if line.startswith("Print ")]
    want_first = []
    for marks, prints, match, block in Dataloader(load_config(toml)):
        want_first += [gallery[m] for m in match]
    assert len(want_first) == len(firsts)
    assert any(r == 1 for r in got3)
    for r, first, want in zip(got3, firsts, want_first):
        if r == 1:
            assert first == want
