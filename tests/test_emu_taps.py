"""Feature taps of every backbone under emulation (tests/taps_cases.py): taps against truncated plans, the stored record
against round16(tap), `out` against the plain and the trace forward, guard bands, batch independence, refusals; then the
multi-layer surface on top of them: the ragged feature sets (an EfficientNet and a plain VGG), the pipeline and the
variant-aware fusion, and the [mi355x] fuse_blocks forms load_config refuses.  The run driver needs a GPU device:
tests/test_gpu_taps.py."""

import os
import subprocess
import sys

import pytest

import taps_cases as tc
from emu_util import emu_library, emu_scorer
from host_device import HostDevice


@pytest.mark.parametrize("case", tc.EMU_CASES, ids=lambda c: c.id)
def test_emu_tap_equals_truncated_plan(case):
    tc.check_case(case, HostDevice(), emu_library())


def test_emu_taps_with_wide_tiles():
    """The ResNet50 16-bit cases on conv_gemm16_kernel<KIND, 128> (SPR_GEMM16_BN=128 is read once per process: a child)."""
    env = dict(os.environ, SPR_GEMM16_BN="128")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "tap_equals_truncated_plan and ResNet50 and not float32"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(tc.WIDE_CASES)} passed" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("arch,block,tap_lists", tc.REFUSALS, ids=[r[0] for r in tc.REFUSALS])
def test_emu_refused_taps(arch, block, tap_lists):
    tc.check_refusals(arch, block, tap_lists, HostDevice(), emu_library())


def test_bad_fuse_blocks_are_refused_at_load_config(tmp_path):
    from shoeprint_image_retrieval_amd.config import load_config

    tc.check_bad_fuse_blocks()
    toml = tmp_path / "run.toml"
    toml.write_text('[model]\ntype = "EfficientNetV2_M"\n[comparison]\nrotations = ""\nscales = ""\n[mi355x]\nfuse_blocks = 4\n')
    with pytest.raises(ValueError, match="fuse_blocks"):
        load_config(toml)
    toml.write_text('[model]\ntype = "EfficientNetV2_M"\n[comparison]\nrotations = ""\nscales = ""\n[mi355x]\nfuse_blocks = [4]\n')
    assert load_config(toml)["mi355x"]["fuse_blocks"] == [4]


@pytest.mark.parametrize("arch,block,taps", [("EfficientNet_B1", 4, (2, 4)), ("VGG16", 9, (7, 9))])
def test_emu_tapped_feature_sets(arch, block, taps):
    """The ragged route on a small EfficientNet (spr_effnet_forward_taps into the class slices) and on a plain VGG (its Python
    route's taps copied in by spr_items_gather); the MI355X test runs the default model."""
    tc.check_feature_sets(arch, block, taps, HostDevice(), emu_library())


def test_emu_pipeline_float32_against_the_oracle():
    """MultiLayerPipeline(EfficientNet_B1[:4], taps = (3, 4)), float32 plan, at 128 x 64: bit for bit the separately truncated
    models, within 1e-4 of the oracle mean, identical ranks.  (The default model's float32 plan - ten times the arithmetic
    per pixel - runs this check on the MI355X.)"""
    tc.check_pipeline(HostDevice(), emu_library(), emu_scorer(), (128, 64), "float32", arch="EfficientNet_B1", taps=(3, 4))


def test_emu_pipeline_on_the_default_model():
    """MultiLayerPipeline(EfficientNetV2_M[:6], taps = (4, 6)) at 128 x 64 with crop 1 (the block-6 map, 8 x 4, survives the
    crop), bfloat16 plan: bit for bit the separately truncated models."""
    tc.check_pipeline(HostDevice(), emu_library(), emu_scorer(crop=1), (128, 64), "bfloat16")


def test_emu_ragged_variant_aware_fusion():
    tc.check_ragged_fusion(HostDevice(), emu_library(), emu_scorer())
