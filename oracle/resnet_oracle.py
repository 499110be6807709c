"""CPU oracle for the build-defined ResNet50 extractor: torch-CPU functional restatement of torchvision's resnet50 (v1.5)
cut after `block` of its top-level children [conv1, bn1, relu, maxpool, layer1, layer2, layer3] (block = 5 / 6 / 7).

TEST INFRASTRUCTURE ONLY (same rules as ncc_oracle.py).  PARITY UNPINNED by the reference: it has no ResNet branch at all
(network.py:121-182) - BASELINE.json config 3 names one - and torchvision is not importable here; the graph below is
torchvision's published resnet50: stem 7x7/2 + BN + ReLU + maxpool 3x3/2, bottlenecks (1x1, 3x3 with the stride, 1x1 x4,
BatchNorm after each, downsample 1x1 + BN on the first block of a layer, ReLU after the sum), [3, 4, 6] blocks.
Pre-processing as the reference's default transforms (network.py:51-71): ToTensor, repeat(3), Normalize(ImageNet mean/std).
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import effnet_oracle

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # network.py:52-53
BLOCKS = (3, 4, 6)


def conv_specs(block: int):
    """(cin, cout, ksize, stride, role) of every convolution in module order; role 0 stem, 1/2/3 bottleneck, 4 downsample."""
    specs = [(3, 64, 7, 2, 0)]
    cin = 64
    for layer in range(block - 4):
        mid = 64 << layer
        for b in range(BLOCKS[layer]):
            stride = 2 if (b == 0 and layer > 0) else 1
            specs += [(cin, mid, 1, 1, 1), (mid, mid, 3, stride, 2), (mid, 4 * mid, 1, 1, 3)]
            if b == 0:
                specs.append((cin, 4 * mid, 1, stride, 4))
            cin = 4 * mid
    return specs


def _round(x: torch.Tensor, compute: str | None) -> torch.Tensor:
    if not compute:
        return x
    return x.to({"float16": torch.float16, "bfloat16": torch.bfloat16}[compute]).to(torch.float32)


def _cbn(x, p, stride, pad):
    w, b, gamma, beta, mu, var = (np.asarray(t, dtype=np.float32) for t in p)
    x = F.conv2d(x, torch.from_numpy(w), torch.from_numpy(b), stride=stride, padding=pad)
    return F.batch_norm(x, torch.from_numpy(mu), torch.from_numpy(var), torch.from_numpy(gamma), torch.from_numpy(beta),
                        training=False, eps=1e-5)


def fold16(p, compute):
    """(weights, bias) of a convolution as a 16-bit plan uses them, float32 tensors: the library folds the BatchNorm into the
    convolution in float32, THEN rounds the weights; the bias stays float32."""
    w, b, gamma, beta, mu, var = (np.asarray(t, dtype=np.float32) for t in p)
    scale = gamma / np.sqrt(var + np.float32(1e-5))
    return (_round(torch.from_numpy(np.ascontiguousarray(w * scale[:, None, None, None])), compute),
            torch.from_numpy(np.ascontiguousarray((b - mu) * scale + beta)))


def conv16(x, p, stride, pad, compute, res=None, relu=False, dtype=torch.float32, bound=False):
    """One convolution of a 16-bit plan (spr_resnet_plan_create_ex) from its stored operand x (values of the compute type,
    NCHW): rounded folded weights, float32 bias, + res (a stored activation), then ReLU - the value BEFORE it is stored,
    evaluated in ``dtype`` (float32: the end-to-end oracle's arithmetic; float64: the exact value of the layer).
    bound=True returns an effnet_oracle.Step: y, A = |W| * |x| + |b| (+ |res|), K = cin x taps (the reduction length), pre (the
    convolution + bias) and res: y = relu(pre + res) here - the ReLU behind the residual sum."""
    w, b = fold16(p, compute)
    with torch.no_grad():
        pre = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=stride, padding=pad)
        y = pre if res is None else pre + res.to(dtype)
        if relu:
            y = F.relu(y)
        if not bound:
            return y
        A = F.conv2d(x.to(torch.float64).abs(), w.to(torch.float64).abs(), b.to(torch.float64).abs(), stride=stride, padding=pad)
        r = None if res is None else res.to(dtype)
        if r is not None:
            A = A + r.abs()
        return effnet_oracle.Step(y, A, w.shape[1] * w.shape[2] * w.shape[3], pre, r)


def blocks(specs):
    """(c1, c2, c3, downsample or None) conv indices of every bottleneck, in order."""
    out, i = [], 1
    while i < len(specs):
        down = i + 3 < len(specs) and specs[i + 3][4] == 4
        out.append((i, i + 1, i + 2, i + 3 if down else None))
        i += 4 if down else 3
    return out


def normalise(img: np.ndarray) -> torch.Tensor:
    """ToTensor, repeat(3), Normalize: uint8 [H,W] -> float32 [1, 3, H, W]."""
    x = torch.from_numpy(img.astype(np.float32) / np.float32(255.0))[None].repeat(3, 1, 1)
    mean = torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
    std = torch.tensor(STD, dtype=torch.float32)[:, None, None]
    return ((x - mean) / std)[None]


def get_feature_maps(img: np.ndarray, block: int, parameters, compute: str | None = None) -> np.ndarray:
    """uint8 [H,W] (already CLAHE'd) -> float32 [C,h,w]; parameters[i] = (w, b, gamma, beta, running_mean, running_var)
    of convolution i of conv_specs(block) and its BatchNorm.  ``compute`` = "float16" | "bfloat16": the 16-bit compute type of
    spr_resnet_plan_create_ex - every convolution, the stem included (its operand is the normalised image), takes rounded
    weights and a rounded operand, the residual operand is a rounded stored activation, everything else float32."""
    x = normalise(img)
    specs = conv_specs(block)
    if compute:  # a loop over conv16: the per-layer reference of tests/layer_cases.py
        x = _round(x, compute)
        x = F.max_pool2d(_round(conv16(x, parameters[0], 2, 3, compute, relu=True), compute), 3, 2, 1)
        bl = blocks(specs)
        for k, (i1, i2, i3, idn) in enumerate(bl):
            t1 = _round(conv16(x, parameters[i1], 1, 0, compute, relu=True), compute)
            t2 = _round(conv16(t1, parameters[i2], specs[i2][3], 1, compute, relu=True), compute)
            r = x if idn is None else _round(conv16(x, parameters[idn], specs[idn][3], 0, compute), compute)
            y = conv16(t2, parameters[i3], 1, 0, compute, res=r, relu=True)
            x = y if k + 1 == len(bl) else _round(y, compute)
        return x.numpy().squeeze(0)
    with torch.no_grad():
        x = F.relu(_cbn(x, parameters[0], 2, 3))
        x = F.max_pool2d(x, 3, 2, 1)
        i = 1
        while i < len(specs):
            down = i + 3 < len(specs) and specs[i + 3][4] == 4
            y = F.relu(_cbn(x, parameters[i], 1, 0))
            y = F.relu(_cbn(y, parameters[i + 1], specs[i + 1][3], 1))
            y = _cbn(y, parameters[i + 2], 1, 0)
            idn = _cbn(x, parameters[i + 3], specs[i + 3][3], 0) if down else x
            x = F.relu(y + idn)
            i += 4 if down else 3
    return x.numpy().squeeze(0)
