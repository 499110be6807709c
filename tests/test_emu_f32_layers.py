"""Per-layer (teacher-forced) parity of the float32 extractor plans under emulation (tests/f32_layer_cases.py): every layer of a
two- or three-image batch against its float64 restatement from the traced float32 records, held to the rigorous (K + C) u A and
the tight (4 sqrt(K) + C) u A bound; guard bands around every buffer; and mutation tests - no kernel involved - that prove the
checker reports what the whole-network tolerance of tests/extractor_cases.py cannot see."""

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import densenet16_cases as dc
import f32_layer_cases as fc
from emu_util import emu_library
from host_device import HostDevice
from oracle import vgg_oracle


@pytest.mark.parametrize("arch,block,hw,n,rgb", [
    ("VGG16", 12, (21, 35), 2, False),       # tiles ragged on both axes; pools of 21 x 35 and 10 x 17 maps
    ("VGG16", 2, (20, 18), 2, False),        # the first convolution alone: one NCHW record
    ("VGG16", 5, (20, 24), 3, True),         # three differing input planes
    ("VGG19_BN", 17, (24, 20), 3, False),    # folded BatchNorm weights, cut behind a ReLU
    ("ResNet50", 6, (34, 47), 2, False),     # all four (ks, stride) instances; odd maps: 17 x 24 -> 9 x 12 -> 5 x 6 (layer1's
                                             # tensor outgrows the stem's: the workspace of a float32 plan was too small for it)
    ("ResNet50", 5, (32, 32), 3, True),      # the minimum size, RGB
    ("EfficientNet_B3", 6, (40, 36), 2, False),    # 5x5 depthwise, squeeze-excitation
    ("EfficientNetV2_S", 5, (40, 32), 2, True),    # fused-MBConv then MBConv, RGB
    ("EfficientNet_B7", 4, (32, 32), 2, False),    # the B7 widths (the full features: on the GPU)
    ("DenseNet_201", 7, (32, 32), 2, False),       # two dense blocks, one transition
    ("DenseNet_201", 6, (36, 40), 3, True),        # ends on a transition's average pool (9 x 10 -> 4 x 5), RGB
])
def test_emu_f32_per_layer_parity(arch, block, hw, n, rgb):
    fc.check_layers(arch, block, hw, n, HostDevice(), emu_library(), rgb=rgb)


@pytest.mark.parametrize("name", ["vgg21", "vgg10", "densenet"])
def test_emu_f32_per_layer_parity_of_the_mutation_traces(name):
    _trace(name)


def test_emu_f32_trace_layouts():
    """What used to be refused: a float32 plan's layout is SPR_OK with the expected records and total_bytes."""
    fc.check_f32_layouts(HostDevice(), emu_library(), [
        ("VGG16", 10, 1, (40, 40)), ("VGG19_BN", 9, 2, (37, 51)), ("VGG16", 2, 1, (40, 40)), ("ResNet50", 5, 1, (40, 40)),
        ("ResNet50", 7, 3, (34, 47)), ("EfficientNetV2_S", 3, 1, (40, 40)), ("EfficientNet_B3", 6, 2, (44, 36)),
        ("DenseNet_201", 5, 1, (40, 40)), ("DenseNet_201", 9, 2, (64, 48)), ("DenseNet_201", 3, 1, (40, 40)),
    ])


# ---------------------------------------------------------------------------------------------------- the checker can fail
TRACES = {
    # ends on conv4_2: 512 -> 512, K = 4608, on a 2 x 1 map (the emulator's slowest case - one matrix-core instruction per four
    # products - so the plain forward is left to the cases above)
    "vgg21": ("VGG16", 21, (18, 14), 2),
    "vgg10": ("VGG16", 10, (21, 19), 2),     # ends on conv2_2 + pool of an odd map (21 x 19 -> 10 x 9)
    "densenet": ("DenseNet_201", 5, (32, 32), 2),
}


@functools.lru_cache(maxsize=None)
def _trace(name):
    keep = {}
    fc.check_layers(*TRACES[name], HostDevice(), emu_library(), keep=keep, runs=False, plain=name != "vgg21")
    return keep


def _flagged(keep, raw, taps=None, out=None, ctx=None):
    """The layers the checker reports for the (mutated) records of a kept trace."""
    ctx, tr = ctx or keep["ctx"], keep["trace"]
    out = tr.out if out is None else out
    if ctx["kind"] == "vgg16":
        results = [fc.check_vgg_layer(ctx, raw, tr.taps if taps is None else taps, i, out) for i in range(len(ctx["stages"]))]
    else:
        results = [fc.check_densenet(ctx, raw, key, out) for key in dc.keys_of(ctx)]
    return [r for r in results if not r.ok]


def test_emu_f32_checker_catches_one_dropped_product_at_k4608():
    """One product of 4608 removed from ONE element of conv4_2's tap (and of the record and out behind it).  The product is of
    average size: at least A / K, yet below the rigorous bound (K + C) u A, which alone would have passed it; it is 13 times
    the tight bound."""
    keep = _trace("vgg21")
    ctx, tr = keep["ctx"], keep["trace"]
    i = len(ctx["stages"]) - 1
    assert 9 * ctx["stages"][i]["cin"] == 4608 and not ctx["stages"][i]["pool"]
    x = fc._nchw(tr.raw[i - 1], 512).double()
    w, _ = (t.double() for t in vgg_oracle.fold16(ctx["params"][i], None, False))
    r = vgg_oracle.conv16(x.float(), ctx["params"][i], None, True, False, False, dtype=torch.float64, bound=True)
    xp = F.pad(x, (1, 1, 1, 1))
    found = None
    for n, c, y, xx in np.argwhere(tr.taps[i] > 0)[:500]:
        prod = (w[c] * xp[n, :, y: y + 3, xx: xx + 3]).numpy().ravel()   # the 4608 products of this element
        a = float(r.A[n, c, y, xx])
        ok = (np.abs(prod) >= a / 4608) & (np.abs(prod) <= fc.units_rigorous(4608) * fc.U * a) & (float(r.pre[n, c, y, xx]) - prod > 0)
        if ok.any():
            found = (int(n), int(c), int(y), int(xx), float(prod[np.argmax(ok)]), a)
            break
    assert found, "no element with a product between A / K and the rigorous bound"
    n, c, y, xx, p, a = found
    taps, raw = dict(tr.taps), list(tr.raw)
    taps[i] = tr.taps[i].copy()
    taps[i][n, c, y, xx] = np.float32(float(tr.taps[i][n, c, y, xx]) - p)
    raw[i] = taps[i].copy()
    assert abs(p) >= 8 * fc.units_tight(4608) * fc.U * a
    bad = _flagged(keep, raw, taps, taps[i].copy())
    assert [b.index for b in bad] == [i], [(b.index, b.errors) for b in bad]
    assert "1 of" in bad[0].errors[0] and "outside the tight bound" in bad[0].errors[0], bad[0].errors
    assert f"image {n} channel {c} pixel (y, x) = ({y}, {xx})" in bad[0].errors[0], bad[0].errors


def test_emu_f32_checker_catches_the_border_tap_read_past_the_row():
    """The right-most column's dx = +1 tap read as if padding were absent: in NHWC the next pixel in memory is the first of
    the next row.  Spliced into a VGG tap only (the record stays), so no other layer reads the defect."""
    keep = _trace("vgg10")
    ctx, tr = keep["ctx"], keep["trace"]
    i = 2   # conv2_1 (64 -> 128, 10 x 9 map): the tap alone is mutated, so no other layer reads the defect
    x = fc._nchw(tr.raw[i - 1], ctx["stages"][i]["cin"]).double()
    w, b = (t.double() for t in vgg_oracle.fold16(ctx["params"][i], None, False))
    xp = F.pad(x, (1, 1, 1, 1))
    xp[:, :, 1:-2, -1] = x[:, :, 1:, 0]      # the padding column right of row y holds pixel (y + 1, 0)
    t = F.relu(F.conv2d(xp, w, b)).float().numpy()
    taps = dict(tr.taps)
    taps[i] = tr.taps[i].copy()
    taps[i][..., -1] = t[..., -1]
    assert not np.array_equal(taps[i], tr.taps[i])
    bad = _flagged(keep, list(tr.raw), taps)
    assert [b.index for b in bad] == [i], [(b.index, b.errors) for b in bad]
    assert "bound" in bad[0].errors[0]


def test_emu_f32_checker_catches_a_growth_slice_shifted_by_one_channel():
    keep = _trace("densenet")
    ctx, tr = keep["ctx"], keep["trace"]
    r = next(k for k, rec in enumerate(ctx["recs"]) if rec["type"] == "block")
    op2 = ctx["recs"][r]["layers"][-1]["op2"]   # the block's last slice: no later layer reads it
    c_off = ctx["ops"][op2]["c_off"]
    raw, out = list(tr.raw), tr.out.copy()
    raw[r] = tr.raw[r].copy()
    raw[r][..., c_off: c_off + 32] = np.roll(tr.raw[r][..., c_off: c_off + 32], 1, axis=-1)
    raw[-1] = np.ascontiguousarray(raw[r].transpose(0, 3, 1, 2))   # the output a kernel with that defect would have copied
    out[:] = raw[-1]
    bad = _flagged(keep, raw, out=out)
    assert [b.index for b in bad] == [f"{r} [{c_off}, {c_off + 32})"], [(b.index, b.errors) for b in bad]


def test_emu_f32_checker_catches_a_record_taken_before_the_pool():
    """The last stage's record (and out) holds the window's first element, not its maximum."""
    keep = _trace("vgg10")
    ctx, tr = keep["ctx"], keep["trace"]
    i = len(ctx["stages"]) - 1
    assert ctx["stages"][i]["pool"]
    ho, wo = tr.out.shape[2:]
    raw, out = list(tr.raw), np.ascontiguousarray(tr.taps[i][:, :, 0: 2 * ho: 2, 0: 2 * wo: 2])
    assert not np.array_equal(out, tr.out)
    raw[i] = out.copy()
    bad = _flagged(keep, raw, out=out)
    assert [b.index for b in bad] == [i], [(b.index, b.errors) for b in bad]
    assert "maxpool2x2?(tap)" in bad[0].errors[0]
    # the score-level tolerance's view of it: far more than one element moves, each by less than the largest activation
    assert np.abs(out - tr.out).max() > 0


def test_emu_f32_checker_catches_a_small_channel_the_whole_network_tolerance_cannot_see():
    """One channel of magnitude below 1e-4 of the tensor's maximum, 1.05 x itself.  The channel is made small exactly: the last
    layer's weights and bias of that channel, and its record, scaled by 2^-17 (a power of two commutes with every rounding, so
    the scaled records are what the same kernel stores for the scaled weights - the checker passes them).  The old check of
    the final tensor, atol = 2e-5 * max(1, |ref|.max()), does not notice the 5 % error; the per-layer check names the layer."""
    keep = _trace("vgg21")
    ctx0, tr = keep["ctx"], keep["trace"]
    i = len(ctx0["stages"]) - 1
    c = int(np.argmax(tr.out.max(axis=(0, 2, 3))))   # a lively channel
    scale = np.float32(2.0 ** -17)
    params = list(ctx0["params"])
    w, b = (np.array(t, dtype=np.float32) for t in params[i][:2])
    w[c] *= scale
    b[c] *= scale
    params[i] = (w, b)
    ctx = dict(ctx0, params=params)
    taps, raw = dict(tr.taps), list(tr.raw)
    taps[i] = tr.taps[i].copy()
    taps[i][:, c] *= scale
    raw[i] = taps[i].copy()
    ref = taps[i].copy()
    assert 0 < np.abs(ref[:, c]).max() < 1e-4 * np.abs(ref).max()
    assert not _flagged(keep, raw, taps, ref.copy(), ctx), "the exactly scaled trace must pass"
    taps[i][:, c] *= np.float32(1.05)
    raw[i] = taps[i].copy()
    got = taps[i].copy()
    # tests/extractor_cases.py: np.testing.assert_allclose(got, ref, rtol=0, atol=tol * max(1, |ref|.max())), tol = 2e-5
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, float(np.abs(ref).max())), "the old tolerance was expected to be blind to it"
    bad = _flagged(keep, raw, taps, got, ctx)
    assert [b.index for b in bad] == [i], [(b.index, b.errors) for b in bad]
    assert f"channel {c} " in bad[0].errors[0], bad[0].errors
