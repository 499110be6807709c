"""`gpu`: feature taps of every backbone on the MI355X (tests/taps_cases.py): taps against truncated plans, the stored record
against round16(tap), `out` against the plain and the trace forward, guard bands, batch independence, refusals; then the
routes on top of them: the ragged feature sets (the default model and a plain VGG), torch.ops.shoeprint_mi355x.extract_taps
against the ctypes route, the pipeline, the variant-aware fusion and the run driver with [mi355x] fuse_blocks."""

import os
import subprocess
import sys

import numpy as np
import pytest

import taps_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()


@pytest.fixture(scope="module")
def torch_dev():
    from shoeprint_image_retrieval_amd.device import TorchDevice

    return TorchDevice()


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.id)
def test_tap_equals_truncated_plan(torch_dev, lib, case):
    tc.check_case(case, torch_dev, lib)


def test_taps_with_wide_tiles():
    """The ResNet50 16-bit cases on conv_gemm16_kernel<KIND, 128> (SPR_GEMM16_BN=128 is read once per process: a child)."""
    env = dict(os.environ, SPR_GEMM16_BN="128")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__),
                        "-k", "tap_equals_truncated_plan and ResNet50 and not float32"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(tc.WIDE_CASES)} passed" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("arch,block,tap_lists", tc.REFUSALS, ids=[r[0] for r in tc.REFUSALS])
def test_refused_taps(torch_dev, lib, arch, block, tap_lists):
    tc.check_refusals(arch, block, tap_lists, torch_dev, lib)


@pytest.fixture(scope="module")
def scorer(torch_dev, lib):
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    return NccScorer(device=torch_dev, library=lib)


def test_tapped_feature_sets(torch_dev, lib):
    tc.check_feature_sets("EfficientNetV2_M", 6, (4, 6), torch_dev, lib, sizes=((96, 64), (128, 96)))
    tc.check_feature_sets("VGG16", 16, (9, 14, 16), torch_dev, lib, sizes=((96, 64), (128, 96)))


# (model, block, taps, compute, arch code of torch.ops.shoeprint_mi355x.extract_taps, RGB)
TORCH_OP_CASES = [("VGG16", 16, (9, 14), "float32", 0, False), ("VGG19_BN", 20, (6, 17), "bfloat16", 2, False),
                  ("EfficientNetV2_M", 6, (4, 2), "float32", 16 + 1, False), ("EfficientNetV2_M", 6, (2, 3, 4, 5), "bfloat16", 16 + 1, True),
                  ("EfficientNet_B1", 5, (4,), "float16", 16 + 3, False), ("ResNet50", 7, (5, 6), "float16", 32, False),
                  ("DenseNet_201", 8, (7, 5, 6), "float32", 48, False), ("DenseNet_201", 8, (6,), "bfloat16", 48, False)]


@pytest.mark.parametrize("arch,block,taps,compute,code,rgb", TORCH_OP_CASES, ids=[f"{c[0]}-{c[3]}" for c in TORCH_OP_CASES])
def test_torch_op_extract_taps_equals_the_ctypes_route(torch_dev, lib, arch, block, taps, compute, code, rgb):
    """torch.ops.shoeprint_mi355x.extract_taps against Model.extract_taps_device (ctypes) on the same packed parameters: the
    taps in the order asked, then `out`, bit for bit; a refused tap raises."""
    import torch

    from shoeprint_image_retrieval_amd import _lib, _torch_ops

    ops = _torch_ops.load()
    m = tc.make_model(arch, block, compute, torch_dev, lib)
    try:
        imgs = tc.images(tc.Case(arch, block, taps, compute, (96, 80), 3, rgb))
        dev_imgs = torch_dev.to_device(imgs)
        ch = 3 if rgb else 1
        want = m.extract_taps_device(dev_imgs, list(taps) + [block], in_channels=ch)
        args = (m.packed, code, block, [float(v) for v in m.mean], [float(v) for v in m.std],
                {"float32": _lib.F32, "float16": _lib.F16, "bfloat16": _lib.BF16}[compute])
        got = ops.extract_taps(dev_imgs, *args, list(taps))
        assert len(got) == len(taps) + 1
        for g, w in zip(got, want):
            assert g.dtype == torch.float32 and g.shape == w.shape and torch.equal(g.view(torch.int32), w.view(torch.int32))
        assert torch.equal(ops.extract_taps(dev_imgs, *args, [])[0].view(torch.int32), want[-1].view(torch.int32))
        for bad in ([block], [1], [taps[0], taps[0]]):
            with pytest.raises(RuntimeError):
                ops.extract_taps(dev_imgs, *args, bad)
    finally:
        m.close()


@pytest.mark.parametrize("compute", ["float32", "bfloat16"])
def test_pipeline_on_the_default_model(torch_dev, lib, scorer, compute):
    tc.check_pipeline(torch_dev, lib, scorer, (256, 128), compute)


def test_ragged_variant_aware_fusion(torch_dev, lib, scorer):
    tc.check_ragged_fusion(torch_dev, lib, scorer)
    tc.check_ragged_fusion(torch_dev, lib, scorer, "EfficientNetV2_M", 6, (4, 6), sizes=((256, 128), (288, 160)),
                           query_sizes=((192, 96), (224, 128)))


def _driver_toml(tmp_path, case, extra):
    return (f'[dataset]\ndir = "{tmp_path}"\ntype = "WVU2019"\ncrop = {case["crop"]}\nn_processes = 3\nn_clusters = 2\n'
            f'cluster_minimise_tolerance = 0.05\n[model]\ntype = "EfficientNetV2_M"\nclahe_clip_limit = 2.0\n'
            f'clahe_tile_grid_size = [8, 8]\nstart_block = 6\nend_block = 4\nskip_blocks = []\nminimum_dim = 120\nmaximum_dim = 200\n'
            f'[comparison]\nn_processes = 2\n[mi355x]\n' + extra)


def test_run_driver_fuse_blocks(tmp_path, capsys, scorer):
    """run_mi355x.main on wvu_split with the default model: fuse_blocks = [] prints and returns what a file without the key
    does; fuse_blocks = [4] returns the ranks of the hand-composed computation - per cluster the features of the separately
    truncated models, their score matrices, the spr_scores_fuse mean, the ranker."""
    import dataset_util
    import run_mi355x
    from shoeprint_image_retrieval_amd.config import load_config
    from shoeprint_image_retrieval_amd.dataloader import Dataloader
    from shoeprint_image_retrieval_amd.network import Model

    case = next(c for c in dataset_util.CASES if c["name"] == "wvu_split")
    dataset_util.write_dataset(str(tmp_path), case)
    toml = tmp_path / "run.toml"

    def run(extra):
        toml.write_text(_driver_toml(tmp_path, case, extra))
        ranks = run_mi355x.main(str(toml))
        return ranks, capsys.readouterr().out

    plain_ranks, plain_out = run("")
    assert run("fuse_blocks = []\n") == (plain_ranks, plain_out)
    got, out = run("fuse_blocks = [4]\n")
    config = load_config(toml)
    want, blocks = [], []
    dev, lib = scorer.dev, scorer.lib
    for marks, prints, match, block in Dataloader(config):
        blocks.append(block)
        layers = sorted({t for t in [4] if t < block} | {block})
        fused = dev.zeros((len(marks), len(prints)), np.float32)
        for k, t in enumerate(layers):
            m = Model(config, t)
            s = scorer.score_matrix_device(m.get_multiple_feature_maps_device(marks, progress=False),
                                           m.get_multiple_feature_maps_device(prints, progress=False))
            lib.check(lib.spr_scores_fuse(dev.ptr(fused), dev.ptr(s), len(marks) * len(prints), 0.0 if k == 0 else 1.0,
                                          1.0 / len(layers), dev.stream()))
            m.close()
        want += [int(r) for r in scorer.ranks_of_device(fused, match)]
    assert got == want and len(got) == len(plain_ranks)
    assert any(b > 4 for b in blocks), blocks  # (a cluster fused two layers)
    assert out.count("Scoring the feature layers") == len(blocks)
