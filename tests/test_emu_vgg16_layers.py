"""Per-layer (teacher-forced) parity of the 16-bit plain-VGG extractors under emulation (tests/vgg16_layer_cases.py): batches of
differing images, tiles ragged on both axes, pooled odd maps, every cut of a BatchNorm stage, RGB input, guard bands around every
buffer (tap buffers included), and sensitivity tests that prove the check catches what the end-to-end comparison cannot."""

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_cases as lc
import vgg16_layer_cases as vc
from emu_util import emu_library
from host_device import HostDevice
from oracle import vgg_oracle


@pytest.mark.parametrize("arch,block,hw,n,compute,runs", [
    ("VGG16", 17, (37, 51), 2, "bfloat16", True),    # tiles ragged on both axes; pools of 37 x 51, 18 x 25 and 9 x 12 maps
    # 512 channels (K = 4608) on 4 x 4 and 2 x 2 maps, the last stage pooled to 1 x 1 (the emulator's slowest case: the other
    # routes to the same result are left to the cases around it)
    ("VGG16", 31, (32, 32), 2, "bfloat16", False),
    ("VGG16", 3, (21, 19), 2, "float16", True),      # a plan of two convolutions; ends on a bare convolution
    ("VGG19_BN", 9, (24, 20), 2, "float16", True),   # cut behind a BatchNorm: folded, no ReLU
    ("VGG19_BN", 14, (24, 20), 2, "bfloat16", True),  # cut behind a pool
    ("VGG19", 18, (24, 20), 2, "float16", False),    # the block of four 256-channel convolutions, cut behind its last ReLU
])
def test_emu_vgg16_per_layer_parity(arch, block, hw, n, compute, runs):
    vc.check_layers(arch, block, hw, n, compute, HostDevice(), emu_library(), runs=runs)


# The traces the sensitivity tests splice their mutations into; each is a full parity case of its own (both compute types).
CASES = {
    "vgg16": ("VGG16", 10, (37, 51), 2, False),    # conv1_2 pools a 37 x 51 map (odd x odd, four tiles wide), cut behind a pool
    "bn": ("VGG19_BN", 10, (24, 20), 2, False),    # ImageNet normalisation, BatchNorm folded, cut behind a ReLU
    "rgb": ("VGG16", 5, (20, 24), 3, True),        # three differing input planes
}


@functools.lru_cache(maxsize=None)
def _trace(case, compute):
    arch, block, hw, n, rgb = CASES[case]
    keep = {}
    vc.check_layers(arch, block, hw, n, compute, HostDevice(), emu_library(), rgb=rgb, keep=keep)
    return keep


@pytest.mark.parametrize("compute", ["bfloat16", "float16"])
@pytest.mark.parametrize("case", list(CASES))
def test_emu_vgg16_per_layer_parity_of_the_mutation_traces(case, compute):
    _trace(case, compute)


def test_emu_vgg16_batch_invariance():
    vc.check_batch_invariance("VGG16", 10, (21, 19), "bfloat16", HostDevice(), emu_library())


def test_emu_vgg16_get_feature_maps():
    vc.check_get_feature_maps("VGG16", 10, (48, 32), "float16", HostDevice(), emu_library())


def test_emu_vgg16_trace_refusals():
    vc.check_refusals(HostDevice(), emu_library())


# ---------------------------------------------------------------------------------------------------- sensitivity
MUTATIONS = {  # name -> the trace it is spliced into
    "record rounded toward zero": "vgg16",
    "pool window shifted by one pixel": "vgg16",
    "pool takes the dropped last row and column": "vgg16",
    "left neighbour missing at the tile seam x = 16": "vgg16",
    "last 32-channel chunk skipped": "vgg16",
    "BatchNorm folded after the weights were rounded": "bn",
    "stem padded with pixel value 0 before normalisation": "vgg16",
    "image 1 computed from image 0's operand": "vgg16",
    "one bias off by one 16-bit step": "bn",
    "RGB planes read as BGR": "rgb",
}


def _mutate(keep, what):
    """(layer, records, taps) of one mutation: the layer restated in float64 from its traced inputs under that mutation, spliced
    in as the tap, the record or both - whatever a kernel with that defect would have written."""
    ctx, tr = keep["ctx"], keep["trace"]
    st, params, compute = ctx["stages"], ctx["params"], ctx["compute"]
    raw, taps = list(tr.raw), dict(tr.taps)
    geo = vc.geometry(st, keep["imgs"].shape[1:3])
    inner = range(1, len(st) - 1)  # stages with a tap and a 16-bit record
    _, _, mean, std = vgg_oracle.ARCHS[ctx["arch"]]

    def operand(i):
        return lc._vals16(raw[i - 1], compute, st[i]["cin"])

    def conv(x, w, b, padding=1):
        return F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=padding)

    def splice(i, pre):  # float64 convolution + bias -> the tap and the record a kernel would store from it
        t = (F.relu(pre) if st[i]["relu"] else pre).to(torch.float32).numpy()
        taps[i] = t
        raw[i] = vc.stored(vc.pool2(t) if st[i]["pool"] else t, compute)
        return i, raw, taps

    def stem(x, padding=1):
        w, b = vgg_oracle.fold16(params[0], compute, st[0]["bn"])
        raw[0] = vc.stored(F.relu(conv(x, w, b, padding)).to(torch.float32).numpy(), compute)
        return 0, raw, taps

    if what == "record rounded toward zero":
        i = next(i for i in inner if not st[i]["pool"])
        raw[i] = vc.stored(taps[i], compute, "rtz")
        return i, raw, taps
    if what == "pool window shifted by one pixel":
        i = next(i for i in inner if st[i]["pool"])
        raw[i] = vc.stored(vc.pool2(np.roll(taps[i], -1, axis=3)), compute)
        return i, raw, taps
    if what == "pool takes the dropped last row and column":
        i = next(i for i in inner if st[i]["pool"] and geo[i][0] % 2 and geo[i][1] % 2)
        t = torch.from_numpy(taps[i])
        full = F.max_pool2d(t, 2, 2, ceil_mode=True)   # one more row and column than the floor pool
        p = F.max_pool2d(t, 2, 2).clone()
        p[:, :, -1, :] = torch.maximum(p[:, :, -1, :], full[:, :, -1, :-1])
        p[:, :, :, -1] = torch.maximum(p[:, :, :, -1], full[:, :, :-1, -1])
        p[:, :, -1, -1] = torch.maximum(p[:, :, -1, -1], full[:, :, -1, -1])
        raw[i] = vc.stored(p.numpy(), compute)
        return i, raw, taps
    if what == "left neighbour missing at the tile seam x = 16":
        i = next(i for i in inner if geo[i][1] > 17)
        w, b = vgg_oracle.fold16(params[i], compute, st[i]["bn"])
        left = w.clone()
        left[:, :, :, 1:] = 0  # the dx = 0 taps alone
        pre = conv(operand(i), w, b)
        pre[..., 16] -= conv(operand(i), left, None)[..., 16]
        return splice(i, pre)
    if what == "last 32-channel chunk skipped":
        i = next(i for i in inner if not st[i]["pool"])
        w, b = vgg_oracle.fold16(params[i], compute, st[i]["bn"])
        w = w.clone()
        w[:, -32:] = 0
        return splice(i, conv(operand(i), w, b))
    if what == "BatchNorm folded after the weights were rounded":
        i = next(i for i in inner if st[i]["bn"])
        wr, b0, gamma, beta, mu, var = (np.asarray(t, np.float32) for t in params[i])
        scale = gamma / np.sqrt(var + np.float32(1e-5))
        w = vgg_oracle.round_to(vgg_oracle.round_to(torch.from_numpy(wr), compute) * torch.from_numpy(scale)[:, None, None, None], compute)
        _, b = vgg_oracle.fold16(params[i], compute, True)
        return splice(i, conv(operand(i), w, b))
    if what == "stem padded with pixel value 0 before normalisation":
        padded = np.pad(keep["imgs"], ((0, 0), (1, 1), (1, 1)))  # pixel value 0 around the image, then normalised like any pixel
        return stem(lc._normalised(padded, mean, std, compute)[1], padding=0)
    if what == "image 1 computed from image 0's operand":
        i = next(iter(inner))
        x = operand(i).clone()
        x[1] = x[0]
        w, b = vgg_oracle.fold16(params[i], compute, st[i]["bn"])
        return splice(i, conv(x, w, b))
    if what == "one bias off by one 16-bit step":
        i = 1  # the shortest reduction behind the stem (K = 576): the smallest bound
        w, b = vgg_oracle.fold16(params[i], compute, st[i]["bn"])
        c = int(np.argmax(np.abs(b.numpy())))
        step = float(lc.ulp16(np.float64(b[c]), compute))
        r = vgg_oracle.conv16(operand(i), params[i], compute, st[i]["relu"], False, st[i]["bn"], dtype=torch.float64, bound=True)
        e = (lc.gamma_mfma(r.K) * r.A[:, c]).numpy()
        # the step must exceed the bound where the ReLU lets it through, or this mutation proves nothing
        assert np.any((step > 1.01 * e) & (r.pre[:, c].numpy() > 0)), (step, float(e.min()))
        b = b.clone().double()
        b[c] += step
        return splice(i, conv(operand(i), w, b))
    if what == "RGB planes read as BGR":
        assert keep["imgs"].ndim == 4
        return stem(lc._normalised(np.ascontiguousarray(keep["imgs"][..., ::-1]), mean, std, compute)[1])
    raise KeyError(what)


@pytest.mark.parametrize("compute", ["bfloat16", "float16"])
@pytest.mark.parametrize("what", list(MUTATIONS))
def test_emu_vgg16_per_layer_check_catches(what, compute):
    """Each mutation is spliced into a real emulator trace; the per-layer check must flag THAT layer first (the layer behind it
    reads the mutated record and may be flagged too; the layers in front of it are untouched and must pass)."""
    keep = _trace(MUTATIONS[what], compute)
    ctx, tr = keep["ctx"], keep["trace"]
    layer, raw, taps = _mutate(keep, what)
    changed = not np.array_equal(raw[layer], tr.raw[layer]) or (layer in taps and not np.array_equal(taps[layer], tr.taps[layer]))
    assert changed, "the mutation changed nothing"
    upto = min(layer + 2, len(ctx["stages"]))
    flagged = [i for i in range(upto) if not vc.check_layer(ctx, raw, taps, i).ok]
    assert flagged and flagged[0] == layer, (what, layer, flagged)
