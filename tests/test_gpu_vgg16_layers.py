"""`gpu`: per-layer (teacher-forced) parity of the 16-bit plain-VGG extractors on the MI355X (tests/vgg16_layer_cases.py): every
convolution's float32 tap against its float64 restatement from the record the kernel itself stored, every stored record against
round16(maxpool?(tap)) bit for bit, guard bands around out, workspace, trace and tap buffers, and the bit-identity of every route
to the same features (plain forward, taps forward, trace runs with and without taps, the registered torch operator)."""

import numpy as np
import pytest

import layer_cases as lc
import vgg16_layer_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()


@pytest.fixture(scope="module")
def torch_dev():
    from shoeprint_image_retrieval_amd.device import TorchDevice

    return TorchDevice()


@pytest.mark.parametrize("arch,block,hw,n,compute,rgb", [
    # the shapes of test_vgg_on_the_16bit_matrix_cores, two images
    ("VGG16", 16, (512, 256), 2, "bfloat16", False), ("VGG16", 16, (512, 256), 2, "float16", False),
    ("VGG16", 30, (128, 96), 2, "bfloat16", False), ("VGG19_BN", 27, (96, 64), 2, "float16", False),
    ("VGG16", 7, (50, 38), 2, "bfloat16", False),
    ("VGG19", 37, (64, 64), 2, "bfloat16", False),    # the whole of vgg19().features: eight K = 4608 layers, ends on a 2 x 2 pool
    ("VGG16", 30, (128, 96), 2, "float16", False),    # K = 4608 in the other compute type
    ("VGG16", 24, (149, 91), 3, "float16", False),    # odd x odd, ragged tiles, pooled odd maps (149 x 91, 37 x 22, 18 x 11), three images
    ("VGG16", 17, (96, 80), 2, "bfloat16", True),     # RGB through the 16-bit stem
    ("VGG16", 23, (256, 128), 2, "bfloat16", False),  # BASELINE config 5: taps 16 / 23 (and every other convolution)
])
def test_vgg_per_layer_parity_on_the_16bit_matrix_cores(torch_dev, lib, arch, block, hw, n, compute, rgb):
    vc.check_layers(arch, block, hw, n, compute, torch_dev, lib, rgb=rgb)


def test_vgg16_taps_of_a_16bit_plan_equal_the_trace(torch_dev, lib):
    """Model.extract_taps_device(taps 16, 23) under a bfloat16 plan at the config-5 shape: the very taps the multi-layer
    pipeline scores, bit for bit the traced ones (which the parity case of this shape checks layer by layer)."""
    m = lc.make_model("VGG16", 23, "bfloat16", torch_dev, lib)
    try:
        imgs = vc.images(2, (256, 128))
        tr = vc.run_trace(m, lib, torch_dev, imgs, plain=False)
        t16, t23 = m.extract_taps_device(torch_dev.to_device(imgs), [16, 23])
        assert dict(vc.tap_features(m))[16] == 6
        assert np.array_equal(torch_dev.to_host(t16).view(np.uint32), tr.taps[6].view(np.uint32))
        assert np.array_equal(torch_dev.to_host(t23).view(np.uint32), tr.out.view(np.uint32))
    finally:
        m.close()


def test_vgg16_batch_invariance(torch_dev, lib):
    vc.check_batch_invariance("VGG16", 24, (149, 91), "bfloat16", torch_dev, lib)
    vc.check_batch_invariance("VGG19_BN", 27, (96, 64), "float16", torch_dev, lib)


def test_vgg16_get_feature_maps(torch_dev, lib):
    print(vc.check_get_feature_maps("VGG16", 16, (256, 128), "bfloat16", torch_dev, lib))
    print(vc.check_get_feature_maps("VGG19", 18, (100, 70), "float16", torch_dev, lib))


def test_vgg16_trace_refusals(torch_dev, lib):
    vc.check_refusals(torch_dev, lib)


@pytest.mark.parametrize("compute", ["bfloat16", "float16"])
def test_torch_op_extract_equals_the_ctypes_route_under_16bit_plans(lib, monkeypatch, compute):
    """torch.ops.shoeprint_mi355x.extract(..., compute) - the route Model.extract_device takes by default on the GPU - against
    the ctypes route of the same plan, grey and RGB, bit for bit."""
    import torch
    from shoeprint_image_retrieval_amd import _torch_ops
    from shoeprint_image_retrieval_amd.device import TorchDevice

    ops = _torch_ops.load()
    model = lc.make_model("VGG16", 10, compute, TorchDevice(), lib)
    try:
        gen = torch.Generator(device="cpu").manual_seed(3)
        grey = torch.randint(0, 256, (3, 64, 48), dtype=torch.uint8, generator=gen).cuda()
        rgb = torch.randint(0, 256, (2, 40, 32, 3), dtype=torch.uint8, generator=gen).cuda()
        for imgs, ch in ((grey, 1), (rgb, 3)):
            monkeypatch.setenv("SPR_TORCH_OPS", "0")
            want = model.extract_device(imgs, in_channels=ch)
            monkeypatch.setenv("SPR_TORCH_OPS", "1")
            assert _torch_ops.enabled()
            got = ops.extract(imgs, model.packed, model.arch, 10, list(model.mean), list(model.std), vc.CODE[compute])
            assert got.dtype == torch.float32 and torch.isfinite(got).all()
            assert torch.equal(got, want) and torch.equal(model.extract_device(imgs, in_channels=ch), want)
    finally:
        model.close()
