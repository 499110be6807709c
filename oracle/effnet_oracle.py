"""CPU oracle for the EfficientNet (B-series and V2) extractors: torch-CPU restatement of the reference's forward path.

TEST INFRASTRUCTURE ONLY (same rules as ncc_oracle.py).  Follows network.py:163-175 (model choice, mean / std), :60-71 /
:74-87 (ToTensor, repeat(3), Normalize), :185-186 (features[:block]) and :228-244 with torch.nn.functional ops in float32,
on torchvision's efficientnet_v2 graph restated from its published definition: stem 3x3/2 + BatchNorm + SiLU; FusedMBConv =
3x3 expansion (BN, SiLU) + 1x1 projection (BN), or one 3x3 (BN, SiLU) when the expansion is 1; MBConv = 1x1 expansion (BN,
SiLU), depthwise 3x3 (BN, SiLU), squeeze-excitation (mean, 1x1, SiLU, 1x1, sigmoid, scale), 1x1 projection (BN); residual sum
where stride 1 and equal widths (stochastic depth is the identity in eval mode); BatchNorm eps 1e-3 (V2, B5, B7) or 1e-5.  The
B-series is MBConv throughout (kernel 3 or 5), without the expansion convolution where the ratio is 1.
PARITY UNPINNED by the reference: network.py needs cv2, torchvision and downloaded weights, none available offline.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3

# ---- the architecture, restated here independently of the library under test -------------------------------------------------
# torchvision.models.efficientnet: (fused, expand ratio, kernel, stride, input width, output width, layers) per stage.
_V2 = {
    "EfficientNetV2_S": [(1, 1, 3, 1, 24, 24, 2), (1, 4, 3, 2, 24, 48, 4), (1, 4, 3, 2, 48, 64, 4), (0, 4, 3, 2, 64, 128, 6),
                         (0, 6, 3, 1, 128, 160, 9), (0, 6, 3, 2, 160, 256, 15)],
    "EfficientNetV2_M": [(1, 1, 3, 1, 24, 24, 3), (1, 4, 3, 2, 24, 48, 5), (1, 4, 3, 2, 48, 80, 5), (0, 4, 3, 2, 80, 160, 7),
                         (0, 6, 3, 1, 160, 176, 14), (0, 6, 3, 2, 176, 304, 18), (0, 6, 3, 1, 304, 512, 5)],
    "EfficientNetV2_L": [(1, 1, 3, 1, 32, 32, 4), (1, 4, 3, 2, 32, 64, 7), (1, 4, 3, 2, 64, 96, 7), (0, 4, 3, 2, 96, 192, 10),
                         (0, 6, 3, 1, 192, 224, 19), (0, 6, 3, 2, 224, 384, 25), (0, 6, 3, 1, 384, 640, 7)],
}
_B0 = [(0, 1, 3, 1, 32, 16, 1), (0, 6, 3, 2, 16, 24, 2), (0, 6, 5, 2, 24, 40, 2), (0, 6, 3, 2, 40, 80, 3),
       (0, 6, 5, 1, 80, 112, 3), (0, 6, 5, 2, 112, 192, 4), (0, 6, 3, 1, 192, 320, 1)]
_B_MULT = {"EfficientNet_B1": (1.0, 1.1), "EfficientNet_B2": (1.1, 1.2), "EfficientNet_B3": (1.2, 1.4),
           "EfficientNet_B4": (1.4, 1.8), "EfficientNet_B5": (1.6, 2.2), "EfficientNet_B6": (1.8, 2.6),
           "EfficientNet_B7": (2.0, 3.1)}
# BatchNorm eps as torchvision builds the models: 1e-3 for efficientnet_v2_* and b5 / b6 / b7, the default 1e-5 otherwise
EPS = {**{k: 1e-3 for k in _V2}, **{k: (1e-3 if k[-1] in "567" else 1e-5) for k in _B_MULT}}


def make_divisible(v: float, divisor: int = 8) -> int:
    """torchvision.models._utils._make_divisible with min_value = divisor."""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def stages(model_str: str):
    if model_str in _V2:
        return list(_V2[model_str])
    wm, dm = _B_MULT[model_str]
    import math
    return [(f, e, k, s, make_divisible(ci * wm), make_divisible(co * wm), int(math.ceil(n * dm))) for f, e, k, s, ci, co, n in _B0]


def arch_ops(model_str: str, block: int) -> list[dict]:
    """features[:block] (network.py:185-186) flattened into convolutions (kind 0), depthwise convolutions (1) and
    squeeze-excitations (2), with the module name of every layer in a torchvision state dict.  act: 2 = SiLU, 0 = none."""
    st = stages(model_str)
    ops = [dict(kind=0, cin=3, cout=st[0][4], ks=3, stride=2, act=2, res=0, sq=0, feature=0, block_end=1,
                names=("features.0.0", "features.0.1"))]
    for si, (fused, expand, ks, stride0, cin0, cout, layers) in enumerate(st[: max(0, block - 1)]):
        for l in range(layers):
            cin, stride = (cin0, stride0) if l == 0 else (cout, 1)
            exp = make_divisible(cin * expand)
            res = int(stride == 1 and cin == cout)
            pre = f"features.{si + 1}.{l}.block"
            k = 0

            def conv(ci, co, kk, s, act, r, end):
                nonlocal k
                ops.append(dict(kind=0, cin=ci, cout=co, ks=kk, stride=s, act=act, res=r, sq=0, feature=si + 1, block_end=end,
                                names=(f"{pre}.{k}.0", f"{pre}.{k}.1")))
                k += 1

            if fused:
                if exp != cin:
                    conv(cin, exp, ks, stride, 2, 0, 0)
                    conv(exp, cout, 1, 1, 0, res, 1)
                else:
                    conv(cin, cout, ks, stride, 2, res, 1)
                continue
            if exp != cin:
                conv(cin, exp, 1, 1, 2, 0, 0)
            ops.append(dict(kind=1, cin=exp, cout=exp, ks=ks, stride=stride, act=2, res=0, sq=0, feature=si + 1, block_end=0,
                            names=(f"{pre}.{k}.0", f"{pre}.{k}.1")))
            k += 1
            ops.append(dict(kind=2, cin=exp, cout=exp, ks=0, stride=0, act=0, res=0, sq=max(1, cin // 4), feature=si + 1,
                            block_end=0, names=(f"{pre}.{k}.fc1", f"{pre}.{k}.fc2")))
            k += 1
            conv(exp, cout, 1, 1, 0, res, 1)
    if block >= len(st) + 2:  # the whole of `features`: the closing 1x1 convolution + BatchNorm + SiLU
        cin, f = st[-1][5], len(st) + 1
        ops.append(dict(kind=0, cin=cin, cout=1280 if model_str in _V2 else 4 * cin, ks=1, stride=1, act=2, res=0, sq=0, feature=f,
                        block_end=1, names=(f"features.{f}.0", f"features.{f}.1")))
    return ops


ARCH_KEYS = ("kind", "cin", "cout", "ks", "stride", "act", "res", "sq", "feature", "block_end")


def _round(x: torch.Tensor, compute) -> torch.Tensor:
    if not compute:
        return x
    return x.to({"float16": torch.float16, "bfloat16": torch.bfloat16}[compute]).to(torch.float32)


def get_feature_maps(img: np.ndarray, ops, parameters, mean, std, bn_eps: float = BN_EPS, compute: str | None = None) -> np.ndarray:
    """uint8 [H,W] or RGB [H,W,3] (already CLAHE'd) -> float32 [C,h,w].  ``ops``: the layer list of Model.effnet_ops (kind,
    widths, kernel, stride, activation, residual flag, block_end); ``parameters[i]``: (w, b, gamma, beta, running mean,
    running variance) or, for a squeeze-excitation, (fc1 w, fc1 b, fc2 w, fc2 b).

    ``compute`` = "float16" | "bfloat16" restates the 16-bit plans of spr_effnet_plan_create_ex (BUILD-DEFINED): every tensor
    between layers is stored rounded to that type (the stem reads the rounded normalised image); a convolution takes its
    BatchNorm-folded weights rounded and, where a squeeze-excitation scales its input, the rounded product x * factor; sums,
    bias, SiLU, the residual sum, the squeeze-excitation mean / factors and the depthwise weights are float32; the last
    layer's output is not rounded."""
    if img.ndim == 3:
        x = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0))
    else:
        x = torch.from_numpy(img.astype(np.float32) / np.float32(255.0))[None].repeat(3, 1, 1)
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    x = ((x - m) / s)[None]
    block_in, scale = x, None
    if compute:  # a loop over step16 / se_step: the per-layer reference of tests/layer_cases.py
        return _forward16(x, ops, parameters, bn_eps, compute)
    with torch.no_grad():
        for op, p in zip(ops, parameters):
            t = [torch.from_numpy(np.asarray(a, dtype=np.float32)) for a in p]
            if op["kind"] == 2:
                z = x.mean(dim=(2, 3), keepdim=True)
                z = F.silu(F.conv2d(z, t[0].reshape(op["sq"], op["cin"], 1, 1), t[1]))
                scale = torch.sigmoid(F.conv2d(z, t[2].reshape(op["cin"], op["sq"], 1, 1), t[3]))
                continue
            if op["kind"] == 0 and scale is not None:
                x = x * scale
                scale = None
            groups = op["cin"] if op["kind"] == 1 else 1
            y = F.conv2d(x, t[0], t[1], stride=op["stride"], padding=op["ks"] // 2, groups=groups)
            y = F.batch_norm(y, t[4], t[5], t[2], t[3], training=False, eps=bn_eps)
            if op["act"] == 2:
                y = F.silu(y)
            if op["kind"] == 0 and op["res"]:
                y = y + block_in
            x = y
            if op["block_end"]:
                block_in = x
    return x.numpy().squeeze(0)


class Step(NamedTuple):
    """One layer restated: y = act(pre) (+ res); A, K: see step16."""
    y: torch.Tensor
    A: torch.Tensor
    K: int
    pre: torch.Tensor
    res: torch.Tensor | None


def fold16(op, p, bn_eps, compute):
    """(weights, bias) of a convolution / depthwise layer as a 16-bit plan uses them, float32 tensors: eval-mode BatchNorm folded
    in float32 as the library folds it; THEN a convolution's weights rounded to the compute type (depthwise weights stay f32)."""
    w, b, gamma, beta, mu, var = (np.asarray(a, dtype=np.float32) for a in p)
    s = gamma / np.sqrt(var + np.float32(bn_eps))
    wf = torch.from_numpy(np.ascontiguousarray(w * s[:, None, None, None]))
    bf = torch.from_numpy(np.ascontiguousarray((b - mu) * s + beta))
    return (_round(wf, compute) if op["kind"] == 0 else wf), bf


def operand16(x, scale, compute):
    """A convolution's operand: the stored input, or round(x * factor) with the product in float32 where a squeeze-excitation
    scales it (scale: [N, C, 1, 1] float32 factors)."""
    return x if scale is None else _round(x * scale, compute)


def se_step(op, p, x, dtype=torch.float32, bound=False, pool_chains=32):
    """Squeeze-excitation factors [N, C, 1, 1] of the stored tensor x: mean, fc1, SiLU, fc2, sigmoid, evaluated in ``dtype``.
    bound=True also returns E: an absolute bound on the float32 evaluation's error (the kernels' f32 chains, worst case:
    enet_pool16_kernel's 32 strided chains + their sum, enet_fc1_kernel's two fma chains + 7 adds, enet_fc2_kernel's four
    chains + 3 adds; SiLU's slope <= 1.1, the sigmoid's <= 1/4, a few units of rounding for each of them).  pool_chains: the
    strided chains the mean is summed in - 32 in enet_pool16_kernel, 4 in the float32 plans' enet_pool_kernel (x is then the
    stored float32 tensor: nothing on this path is rounded to a 16-bit type)."""
    t = [torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype) for a in p]
    x = x.to(dtype)
    with torch.no_grad():
        z = x.mean(dim=(2, 3), keepdim=True)
        z = F.silu(F.conv2d(z, t[0].reshape(op["sq"], op["cin"], 1, 1), t[1]))
        f = torch.sigmoid(F.conv2d(z, t[2].reshape(op["cin"], op["sq"], 1, 1), t[3]))
        if not bound:
            return f
        u, hw, c, sq = 2.0 ** -24, x.shape[2] * x.shape[3], op["cin"], op["sq"]
        a = [v.abs() for v in t]
        pm = x.abs().mean(dim=(2, 3), keepdim=True)
        e_p = (-(-hw // pool_chains) + 34) * u * pm
        mz = F.conv2d(pm, a[0].reshape(sq, c, 1, 1), a[1])
        e_z = (-(-c // 128) + 9) * u * mz + F.conv2d(e_p, a[0].reshape(sq, c, 1, 1))
        e_h = 1.1 * e_z + 4 * u * z.abs()
        mt = F.conv2d(z.abs(), a[2].reshape(c, sq, 1, 1), a[3])
        e_t = (-(-sq // 4) + 4) * u * mt + F.conv2d(e_h, a[2].reshape(c, sq, 1, 1))
        return f, 1.05 * (0.25 * e_t + 4 * u * f)


def step16(op, p, x, block_in, scale, bn_eps, compute, dtype=torch.float32, bound=False):
    """One convolution / depthwise layer of a 16-bit plan from its inputs: x the stored (rounded) input [N, C, H, W], block_in
    the stored block input (the residual operand, used where op["res"]), scale the squeeze-excitation factors on the operand or
    None.  Returns the layer's value BEFORE it is stored (the caller rounds it, or not for the last layer), evaluated in
    ``dtype``: float32 = the end-to-end oracle's arithmetic, float64 = the exact value of the layer.  The operand is always
    prepared in float32 (round(x * factor) is a float32 product).  bound=True returns a Step: y, A = |W| * |a| + |b| (+ |res|)
    (the magnitude sum that scales the kernel's f32 error), K (the reduction length, cin x taps; depthwise: taps), and the parts
    y is made of: pre (convolution + bias, before the activation) and res (the residual operand or None)."""
    wf, bf = fold16(op, p, bn_eps, compute)
    a = operand16(x, scale, compute) if op["kind"] == 0 else x
    groups = op["cin"] if op["kind"] == 1 else 1
    cv = dict(stride=op["stride"], padding=op["ks"] // 2, groups=groups)
    res = block_in.to(dtype) if op["kind"] == 0 and op["res"] else None
    with torch.no_grad():
        pre = F.conv2d(a.to(dtype), wf.to(dtype), bf.to(dtype), **cv)
        y = F.silu(pre) if op["act"] == 2 else pre
        if res is not None:
            y = y + res
        if not bound:
            return y
        A = F.conv2d(a.to(torch.float64).abs(), wf.to(torch.float64).abs(), bf.to(torch.float64).abs(), **cv)
        if res is not None:
            A = A + res.abs()
        return Step(y, A, (op["cin"] if op["kind"] == 0 else 1) * op["ks"] ** 2, pre, res)


def _forward16(x, ops, parameters, bn_eps, compute):
    x = _round(x, compute)  # the stored tensor: what the next layer reads
    block_in, scale = x, None
    for i, (op, p) in enumerate(zip(ops, parameters)):
        if op["kind"] == 2:
            scale = se_step(op, p, x)
            continue
        y = step16(op, p, x, block_in, scale if op["kind"] == 0 else None, bn_eps, compute)
        if op["kind"] == 0:
            scale = None
        x = y if i + 1 == len(ops) else _round(y, compute)
        if op["block_end"]:
            block_in = x
    return x.numpy().squeeze(0)
