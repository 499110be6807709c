"""`gpu`: the device-resident route through the real gfx950 library on an MI355X - the checks of resident_cases.py (which
tests/test_emu_resident.py runs on the CPU-emulation build), the gather's offsets beyond 2^31 bytes, and the run driver with
``[mi355x] device_resident``."""

import numpy as np
import pytest

import resident_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()  # raises if the in-tree .so is missing: no fallback


def make_scorer(method="fft", **kw):
    from shoeprint_image_retrieval_amd import _lib
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    return NccScorer(method=method, library=_lib.load_library(), **kw)


@pytest.fixture(scope="module")
def scorer(lib):
    return make_scorer()


@pytest.mark.parametrize("n", sorted(rc.INDEXES))
@pytest.mark.parametrize("storage", rc.STORAGES)
@pytest.mark.parametrize("item_elems", rc.ITEM_ELEMS)
def test_gather(scorer, item_elems, storage, n):
    rc.check_gather(scorer, item_elems, storage, rc.INDEXES[n])


def test_gather_grid_stride(scorer):
    rc.check_gather_grid_stride(scorer)


def test_gather_arguments(scorer):
    rc.check_gather_arguments(scorer)


def test_gather_beyond_two_gib(scorer):
    """Three items of 2^28 + 4 floats, filled on the device; item 2 (its first byte 2^31 + 32 into the source) to bfloat16:
    the first and the last 1024 elements and every 65537th between, against torch's own conversion of the same elements."""
    import torch

    from shoeprint_image_retrieval_amd import _lib

    lib, dev = scorer.lib, scorer.dev
    n = (1 << 28) + 4
    src = torch.empty(3 * n, dtype=torch.float32, device=dev.device)
    src.normal_(generator=torch.Generator(device=dev.device).manual_seed(3))
    out = torch.full((n + 64,), 0x2525, dtype=torch.int16, device=dev.device)  # 32 guard elements (64 bytes) on either side
    index = dev.to_device(np.array([2], np.int32))
    lib.check(lib.spr_items_gather(dev.ptr(src), n, dev.ptr(index), 1, dev.ptr(out) + 64, _lib.BF16, dev.stream()))
    assert bool((out[:32] == 0x2525).all()) and bool((out[32 + n:] == 0x2525).all())
    sample = torch.cat([torch.arange(1024), torch.arange(1024, n - 1024, 65537), torch.arange(n - 1024, n)]).to(dev.device)
    want = src[2 * n + sample].to(torch.bfloat16).view(torch.int16)
    assert torch.equal(out[32 + sample], want)
    assert not torch.equal(out[32 + sample], src[n + sample].to(torch.bfloat16).view(torch.int16))  # (not item 1)


def test_scatter(scorer):
    rc.check_scatter(scorer)


def test_scatter_arguments(scorer):
    rc.check_scatter_arguments(scorer)


def test_feature_set(scorer):
    rc.check_feature_set(scorer)


@pytest.mark.parametrize("sides", rc.SIDES)
@pytest.mark.parametrize("method,storage", rc.METHODS)
def test_surface(lib, method, storage, sides):
    rc.check_surface(make_scorer, method, storage, sides)


def test_resident_call_counts(lib, monkeypatch):
    rc.check_resident_call_counts(make_scorer, monkeypatch)


@pytest.mark.parametrize("method,storage", [("fft", "float32"), ("mfma", "bfloat16")])
def test_nothing_crosses(lib, monkeypatch, method, storage):
    rc.check_nothing_crosses(make_scorer, monkeypatch, method, storage)


@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_extractor(lib, scorer, rgb):
    rc.check_extractor(scorer.dev, lib, rgb)


def test_extractor_shared_feature_shape(lib, scorer):
    rc.check_extractor_shared_feature_shape(scorer.dev, lib)


def test_run_driver_resident(tmp_path, capsys):
    """run_mi355x.main on wvu_split with [mi355x] device_resident = true - with and without device_resize, with shortlist = 3
    and without - prints what the keys-off run prints and returns its ranks; max_feature_gib = 0 sends every cluster down the
    host route, says so on stderr, and changes nothing else."""
    import dataset_util
    import run_mi355x

    case = next(c for c in dataset_util.CASES if c["name"] == "wvu_split")
    dataset_util.write_dataset(str(tmp_path), case)
    toml = tmp_path / "run.toml"
    base = (f'[dataset]\ndir = "{tmp_path}"\ntype = "WVU2019"\ncrop = {case["crop"]}\nn_processes = 3\nn_clusters = 2\n'
            f'cluster_minimise_tolerance = 0.05\n[model]\ntype = "VGG16"\nclahe_clip_limit = 2.0\nclahe_tile_grid_size = [8, 8]\n'
            f'start_block = 16\nend_block = 9\nskip_blocks = []\nminimum_dim = 120\nmaximum_dim = 200\n'
            f'[comparison]\nn_processes = 2\n')

    def run(extra):
        toml.write_text(base + "[mi355x]\n" + extra)
        ranks = run_mi355x.main(str(toml))
        io = capsys.readouterr()
        return ranks, io.out, io.err

    for shortlist in ("", "shortlist = 3\n"):
        want_ranks, want_out, want_err = run(shortlist)
        assert "host route" not in want_err and ("offset (" in want_out) == bool(shortlist)
        for resize in ("", "device_resize = true\n"):
            ranks, out, err = run(shortlist + resize + "device_resident = true\n")
            assert ranks == want_ranks and out == want_out and "host route" not in err, (shortlist, resize)
        ranks, out, err = run(shortlist + "device_resident = true\nmax_feature_gib = 0\n")
        assert ranks == want_ranks and out == want_out
        lines = [l for l in err.splitlines() if "host route" in l]
        assert len(lines) == 2 and all("max_feature_gib = 0" in l for l in lines), err  # one line per cluster
