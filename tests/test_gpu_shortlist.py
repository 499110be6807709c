"""`gpu`: shortlist retrieval through the real gfx950 library on an MI355X - the checks of shortlist_cases.py (which
tests/test_emu_shortlist.py runs on the CPU-emulation build), the torch op against the ctypes route, more rows than one
launch has workgroups, and the run driver's shortlist output."""

import os
import re

import numpy as np
import pytest

import shortlist_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()  # raises if the in-tree .so is missing: no fallback


def _scorer(lib, method="fft", **kw):
    """A scorer on the ctypes route (the torch op is compared with it below)."""
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    s = NccScorer(method=method, library=lib, **kw)
    s._ops_cache = None
    return s


@pytest.fixture(scope="module")
def scorer(lib):
    return _scorer(lib)


@pytest.mark.parametrize("k", sc.TOPK_KS)
@pytest.mark.parametrize("size", sc.TOPK_SIZES)
def test_topk_order(scorer, size, k):
    sc.check_topk_order(scorer, size, k)


def test_topk_edges(scorer):
    sc.check_topk_edges(scorer)


def test_topk_merge(scorer):
    sc.check_topk_merge(scorer)


def test_strided_views_are_refused(lib, scorer):
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    sc.check_strided_views_are_refused(scorer)
    sc.check_strided_views_are_refused(NccScorer(method="fft", library=lib))  # (routed through the torch op by default)


def test_grid_stride(scorer, monkeypatch):
    sc.check_grid_stride(scorer, monkeypatch)


def test_topk_more_rows_than_workgroups_of_a_launch(scorer):
    """n_queries above 65 535: every row still gets its own answer."""
    s = np.random.default_rng(8).standard_normal((70000, 3)).astype(np.float32)
    s[::2, 1] = s[::2, 2]
    got_s, got_i = sc._topk(scorer, s, 2, global_col0=11)
    order = np.lexsort((-np.arange(3)[None].repeat(len(s), 0), -s), axis=1)[:, :2]
    np.testing.assert_array_equal(got_i, order + 11)
    np.testing.assert_array_equal(got_s.view(np.uint32), np.take_along_axis(s, order, axis=1).view(np.uint32))


@pytest.mark.parametrize("shape", sc.PEAK_SHAPES)
def test_maps_peak_exact(scorer, shape):
    sc.check_maps_peak_exact(scorer, shape)


def test_maps_peak_arguments(scorer):
    sc.check_maps_peak_arguments(scorer)


LOCATE = [("fft", "float32", 0), ("fft_pow2", "float32", 0), ("direct", "float32", 0), ("mfma", "bfloat16", 0),
          ("mfma_f32", "float32", 0), ("fft", "float32", 1), ("fft_pow2", "float32", 1), ("direct", "float32", 1),
          ("mfma", "bfloat16", 1), ("mfma_f32", "float32", 1), ("fft", "float32", 2), ("fft_pow2", "float32", 2)]


@pytest.mark.parametrize("method,storage,case", LOCATE)
def test_locate_planted(lib, method, storage, case):
    sc.check_locate_planted(_scorer(lib, method, storage=storage), sc.PLANTED_CASES[case])


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_locate_variants(lib, method):
    sc.check_locate_variants(_scorer(lib, method))


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_retrieve_surface(lib, method):
    sc.check_retrieve_surface(_scorer(lib, method))


def test_topk_op_equals_the_ctypes_route_bit_for_bit(lib, scorer):
    """torch.ops.shoeprint_mi355x.topk on device tensors against spr_topk_rows through ctypes; the host mirror routes
    through the op by default; a CPU tensor is refused."""
    import torch
    from shoeprint_image_retrieval_amd import _torch_ops
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    ops = _torch_ops.load()
    routed = NccScorer(method="fft", library=lib)
    assert routed._torch_ops() is not None and scorer._torch_ops() is None
    for (nq, ng), k in (((5, 300), 5), ((2, 1500), 64), ((3, 7), 10)):
        s = scorer.dev.to_device(np.array(sc.topk_matrix(nq, ng)))
        want_s, want_i = scorer.topk_device(s, k)
        got_s, got_i = ops.topk(s, k)
        assert got_s.dtype == torch.float32 and got_i.dtype == torch.int32 and tuple(got_i.shape) == (nq, k)
        assert torch.equal(got_i, want_i) and torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))
        r_s, r_i = routed.topk_device(s, k)
        assert torch.equal(r_i, want_i) and torch.equal(r_s.view(torch.int32), want_s.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the op takes PyTorch's current stream
        again_s, again_i = ops.topk(s, k)
    side.synchronize()
    assert torch.equal(again_i, want_i)
    with pytest.raises(RuntimeError, match="must live in HBM"):
        ops.topk(torch.zeros(2, 3), 2)
    with pytest.raises(RuntimeError, match="outside"):
        ops.topk(s, 257)


def test_run_driver_prints_the_shortlist(tmp_path, capsys):
    """run_mi355x.main with [mi355x] shortlist = 3: under every query's rank line its three best gallery prints; where the
    true match ranks first, the first name is the true match; shortlist = 0 prints what no shortlist key prints."""
    import dataset_util
    import run_mi355x
    from shoeprint_image_retrieval_amd.dataloader import Dataloader

    case = next(c for c in dataset_util.CASES if c["name"] == "wvu_split")
    cfg = dataset_util.write_dataset(str(tmp_path), case)
    toml = tmp_path / "run.toml"
    base = (f'[dataset]\ndir = "{tmp_path}"\ntype = "WVU2019"\ncrop = {case["crop"]}\nn_processes = 3\nn_clusters = 2\n'
            f'cluster_minimise_tolerance = 0.05\n[model]\ntype = "VGG16"\nclahe_clip_limit = 2.0\nclahe_tile_grid_size = [8, 8]\n'
            f'start_block = 16\nend_block = 9\nskip_blocks = []\nminimum_dim = 120\nmaximum_dim = 200\n'
            f'[comparison]\nn_processes = 2\n')
    toml.write_text(base)
    plain_ranks = run_mi355x.main(str(toml))
    plain_out = capsys.readouterr().out
    toml.write_text(base + "[mi355x]\nshortlist = 0\n")
    assert run_mi355x.main(str(toml)) == plain_ranks
    assert capsys.readouterr().out == plain_out and "offset (" not in plain_out
    toml.write_text(base + "[mi355x]\nshortlist = 3\n")
    assert run_mi355x.main(str(toml)) == plain_ranks
    lines = capsys.readouterr().out.splitlines()
    entry = re.compile(r"    \d+\. \S+  score \d")
    assert [l for l in lines if not entry.match(l)] == plain_out.splitlines()  # today's lines, in today's order
    gallery = sorted(case["gallery"])
    truth = [gallery[m] for _, _, matches, _ in Dataloader(cfg) for m in matches]
    capsys.readouterr()
    at = [i for i, l in enumerate(lines) if l.startswith("Print ") and "true match ranked" in l]
    assert len(at) == len(truth) == len(plain_ranks)
    for q, i in enumerate(at):
        assert int(lines[i].rsplit(" ", 1)[1]) == plain_ranks[q]
        entries = lines[i + 1:i + 4]
        assert [e.split()[0] for e in entries] == ["1.", "2.", "3."], entries
        assert all("score " in e and "original" in e and "offset (" in e for e in entries)
        names = [e.split()[1] for e in entries]
        assert len(set(names)) == 3 and set(names) <= set(gallery)
        if plain_ranks[q] == 1:
            assert names[0] == truth[q]
        else:
            assert names[0] != truth[q]
