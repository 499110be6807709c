"""Feature extractor on MI355X — host mirror of the reference's ``network.py``.

Drop-in for ``src/shoeprint_image_retrieval/network.py``:

* ``Model(config, block)``                                        (network.py:93-97)
* ``Model.get_feature_maps(img) -> float32 [C, h, w]``            (network.py:210-244)
* ``Model.get_multiple_feature_maps(images, *, progress=True)``   (network.py:246-269)

``block`` is the slice end into the backbone's ``features`` (network.py:185).  The forward pass is the HIP
library's ``spr_<family>_forward`` (for the plain VGGs: implicit-GEMM 3x3 convolutions on the fp32 matrix cores with
bias / ReLU / max-pool fused, pre-processing fused into the first layer) and — unlike the reference's one
image per launch (network.py:228) — runs whole batches; ``extract_device`` keeps the features in HBM
for the scorer.  Unknown ``model.type`` raises ``LookupError("Model string not found")`` as the
reference does (network.py:180-182).  ``EfficientNetV2_S / _M / _L`` (network.py:163-175; run.toml's default) and
``EfficientNet_B1 .. B5, B7`` (network.py:139-162) run on ``spr_effnet_forward`` (stem, FusedMBConv and MBConv stages;
BatchNorm folded and parameters packed here) and ``DenseNet_201`` (network.py:176-179) on ``spr_densenet_forward``: every
backbone of the reference's list is built.  ``model.type = "ResNet50"`` is BUILD-DEFINED (BASELINE.json config 3 names a ResNet50
layer3 extractor, the reference has none): torchvision's resnet50 cut after ``block`` of its top-level children
[conv1, bn1, relu, maxpool, layer1, layer2, layer3], block = 5 / 6 / 7, ImageNet mean / std.

Weights: torchvision downloads ``IMAGENET1K_FEATURES`` by name (network.py:126), impossible offline.
``config["mi355x"]["weights"]`` may name a local state dict (``features.N.weight/bias``, loaded with
``torch.load(weights_only=True)``); otherwise seeded He-normal weights from ``synth.vgg16_parameters``
are used (and a warning is printed once).
"""

from __future__ import annotations

import ctypes as C
import sys
from typing import Any

import numpy as np

from . import _lib, synth

VGG16_MEAN = (0.48235, 0.45882, 0.40784)                     # network.py:128
VGG16_STD = (0.00392156862745098,) * 3                       # network.py:129
IMAGENET_MEAN = (0.485, 0.456, 0.406)                        # network.py:52 (the default transforms)
IMAGENET_STD = (0.229, 0.224, 0.225)                         # network.py:53
BN_EPS = 1e-5                                                # torch.nn.BatchNorm2d default
# model.type -> (spr_vgg_arch, mean, std): the plain-VGG branches of network.py:121-139
_VGG_MODELS = {"VGG16": (0, VGG16_MEAN, VGG16_STD), "VGG19": (1, IMAGENET_MEAN, IMAGENET_STD),
               "VGG19_BN": (2, IMAGENET_MEAN, IMAGENET_STD)}
# BUILD-DEFINED (BASELINE.json config 3; the reference has no ResNet branch): torchvision's resnet50 cut after `block` of its
# top-level children [conv1, bn1, relu, maxpool, layer1, layer2, layer3] - block 5 / 6 / 7 - with the default transforms
_RESNET_MODELS = {"ResNet50": (IMAGENET_MEAN, IMAGENET_STD)}
# network.py:139-175: arch id of spr_effnet_plan_create, mean, std (EfficientNetV2_L was trained on 0.5 / 0.5), BatchNorm eps
# (torchvision builds efficientnet_v2_* and efficientnet_b5 / b6 / b7 with eps = 1e-3, the others with the default 1e-5)
_EFFNET_MODELS = {"EfficientNetV2_S": (0, IMAGENET_MEAN, IMAGENET_STD, 1e-3), "EfficientNetV2_M": (1, IMAGENET_MEAN, IMAGENET_STD, 1e-3),
                  "EfficientNetV2_L": (2, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 1e-3),
                  "EfficientNet_B1": (3, IMAGENET_MEAN, IMAGENET_STD, 1e-5), "EfficientNet_B2": (4, IMAGENET_MEAN, IMAGENET_STD, 1e-5),
                  "EfficientNet_B3": (5, IMAGENET_MEAN, IMAGENET_STD, 1e-5), "EfficientNet_B4": (6, IMAGENET_MEAN, IMAGENET_STD, 1e-5),
                  "EfficientNet_B5": (7, IMAGENET_MEAN, IMAGENET_STD, 1e-3), "EfficientNet_B7": (8, IMAGENET_MEAN, IMAGENET_STD, 1e-3)}
_COMPUTE = {"float32": _lib.F32, "float16": _lib.F16, "bfloat16": _lib.BF16, "bfloat16x3": _lib.BF16X3}
_warned = False


_VGG_CONVS_PER_STAGE = {"VGG16": (2, 2, 3, 3, 3), "VGG19": (2, 2, 4, 4, 4), "VGG19_BN": (2, 2, 4, 4, 4)}


def tap_ends(model_type: str) -> list[int]:
    """Every slice end into ``features`` (ResNet50: into its child list) at which ``Model.extract_taps_device`` can hand out
    an activation, whatever the block; a model truncated at ``block`` takes those below it.  Plain VGGs: behind the ReLU of
    every convolution but the first; EfficientNets: every stage end (not the stem alone, not the closing convolution, which
    can only be the output); ResNet50: layer1, layer2; DenseNet_201: behind every dense block and transition."""
    if model_type in _VGG_CONVS_PER_STAGE:
        per_conv = 3 if model_type.endswith("_BN") else 2  # convolution [, BatchNorm], ReLU
        ends, at = [], 0
        for convs in _VGG_CONVS_PER_STAGE[model_type]:
            for _ in range(convs):
                at += per_conv
                ends.append(at)
            at += 1  # the max pool
        return ends[1:]
    if model_type in _RESNET_MODELS:
        return [5, 6]
    if model_type in _EFFNET_MODELS:
        return list(range(2, 8 if model_type == "EfficientNetV2_S" else 9))
    if model_type == "DenseNet_201":
        return list(range(5, 12))
    raise LookupError("Model string not found")


def effnet_state_names(ops) -> list[tuple[str, str]]:
    """Module names of the layers in a torchvision efficientnet_v2 state dict, in ``Model.effnet_ops`` order: (convolution,
    BatchNorm) or, for a squeeze-excitation, (fc1, fc2).  Written from torchvision's module layout - features.0 = stem,
    features.s = stage s, .l = block l of the stage, .block.k = its k-th sub-module - and not checked against a checkpoint:
    none is available offline."""
    names, layer, slot = [], {}, 0
    for i, op in enumerate(ops):
        f = op["feature"]
        if f == 0:
            names.append(("features.0.0", "features.0.1"))
            continue
        # the closing 1x1 convolution of `features` is a Conv2dNormActivation of its own, like the stem: a feature that
        # consists of one plain 1x1 convolution with SiLU (inside a stage a 1x1 + SiLU is an expansion, never a block's end)
        if (op["kind"] == 0 and op["ks"] == 1 and op["act"] == 2 and op["block_end"] and i == len(ops) - 1
                and (i == 0 or ops[i - 1]["feature"] != f)):
            names.append((f"features.{f}.0", f"features.{f}.1"))
            continue
        pre = f"features.{f}.{layer.setdefault(f, 0)}.block.{slot}"
        names.append((f"{pre}.fc1", f"{pre}.fc2") if op["kind"] == 2 else (f"{pre}.0", f"{pre}.1"))
        slot += 1
        if op["block_end"]:
            layer[f] += 1
            slot = 0
    return names


def _plan_ops(lib, handle, prefix: str, width: int, keys) -> list[dict]:
    out = []
    for i in range(getattr(lib, f"spr_{prefix}_num_ops")(handle)):
        info = (C.c_int32 * width)()
        lib.check(getattr(lib, f"spr_{prefix}_op_info")(handle, i, info))
        out.append(dict(zip(keys, list(info))))
    return out


def effnet_plan_ops(lib, handle) -> list[dict]:
    """The op list of an spr_effnet_plan (see Model.effnet_ops)."""
    return _plan_ops(lib, handle, "effnet", 16, ("kind", "cin", "cout", "cin_p", "cout_p", "ks", "stride", "act", "res", "sq",
                                                 "feature", "w_off", "b_off", "w2_off", "b2_off", "block_end"))


def densenet_plan_ops(lib, handle) -> list[dict]:
    """The op list of an spr_densenet_plan (see Model.densenet_ops)."""
    return _plan_ops(lib, handle, "densenet", 12, ("kind", "cin", "cout", "c_off", "ctot", "flags", "feature", "w_off", "b_off",
                                                   "s_off", "t_off"))


def densenet_state_names(ops) -> list[tuple]:
    """Module names of the layers in a torchvision densenet201 state dict, in ``Model.densenet_ops`` order (written from
    torchvision's module layout; not checked against a checkpoint: none is available offline)."""
    names, layer = [], {}
    for op in ops:
        f = op["feature"]
        if op["kind"] == 0:
            names.append(("features.conv0", "features.norm0"))
        elif op["kind"] == 1:
            b = (f - 4) // 2 + 1
            pre = f"features.denseblock{b}.denselayer{layer.setdefault(b, 0) + 1}"
            names.append((f"{pre}.norm1", f"{pre}.conv1", f"{pre}.norm2"))
        elif op["kind"] == 2:
            b = (f - 4) // 2 + 1
            names.append((f"features.denseblock{b}.denselayer{layer[b] + 1}.conv2",))
            layer[b] += 1
        elif op["kind"] == 3:
            b = (f - 5) // 2 + 1
            names.append((f"features.transition{b}.norm", f"features.transition{b}.conv"))
        else:
            names.append(("features.norm5",))
    return names


# ---------------------------------------------------------------------- parameters: reading, folding, layouts
_BN_FIELDS = ("weight", "bias", "running_mean", "running_var")


def _state(state, module: str, *fields) -> tuple:
    return tuple(state[f"{module}.{n}"].float().numpy() for n in fields)


def _conv_state(state, conv: str, bn: str | None = None) -> tuple:
    """(weight, bias[, gamma, beta, running mean, running variance]) of a convolution (zero bias where the module has
    none) and the BatchNorm2d behind it."""
    w, = _state(state, conv, "weight")
    b = _state(state, conv, "bias")[0] if f"{conv}.bias" in state else np.zeros(w.shape[0], np.float32)
    return (w, b) + (_state(state, bn, *_BN_FIELDS) if bn else ())


def _fold_bn(w, b, gamma, beta, mu, var, eps):
    """Eval-mode BatchNorm2d behind a convolution is y = (x - mean) * gamma / sqrt(var + eps) + beta: folded into the
    convolution's (w, b) (float32, as the layer itself computes)."""
    scale = gamma / np.sqrt(var + np.float32(eps))
    return w * scale[:, None, None, None], (b - mu) * scale + beta


def _gemm_layout(w, cout_p: int, cin_p: int, kc: int, bn: int = 64) -> np.ndarray:
    """[cout][cin][k][k] -> [cout_p / bn][K / kc][bn][kc], zero-padded, K index = tap * cin_p + c: kc = 16 is
    conv_gemm_kernel's layout, kc = 64 conv_gemm16_kernel's and (bn = 64 | 32) dnet_gemm16_kernel's."""
    cout, cin, k, _ = w.shape
    wp = np.zeros((cout_p, k * k, cin_p), np.float32)
    wp[:cout, :, :cin] = w.reshape(cout, cin, k * k).transpose(0, 2, 1)
    return np.ascontiguousarray(wp.reshape(cout_p // bn, bn, k * k * cin_p // kc, kc).transpose(0, 2, 1, 3)).ravel()


def _padded(a, n: int) -> np.ndarray:
    out = np.zeros(n, np.float32)
    out[:a.size] = a
    return out


def _require_dense(buf) -> None:
    check = getattr(buf, "is_contiguous", None)
    if not (check() if check is not None else buf.flags["C_CONTIGUOUS"]):
        raise ValueError("out must be contiguous")


# ---------------------------------------------------------------------- backbone families
class _Family:
    """What ``Model`` needs to know about one backbone family: its C entry points (``spr_<prefix>_*``), whether it has a
    16-bit path, how its layers are listed, named in a torchvision state dict, read from one, seeded and packed."""
    prefix = count = ""  # spr_<prefix>_<count>: the number of layers
    lister = ""          # the Model method that lists the layers
    seeder = None        # synth.*_parameters(seed, layers)
    half = True          # float16 / bfloat16 plans exist
    split = False        # bfloat16x3 plans exist (float32 values as hi + lo bfloat16 on the bf16 matrix cores)
    custom_op = False    # also served by the registered torch custom op (keyed by arch)

    def __init__(self, arch, mean, std, bn_eps=BN_EPS):
        self.arch, self.mean, self.std, self.bn_eps = arch, mean, std, bn_eps

    def fn(self, lib, name):
        return getattr(lib, f"spr_{self.prefix}_{name}")

    def layers(self, m):
        return getattr(m, self.lister)()

    def read(self, state, layer, names):
        """One layer's parameters out of a torchvision state dict, given its module names."""
        return _conv_state(state, *names)

    def seeded(self, layers):
        return type(self).seeder(1234, layers)

    def pack_on_device(self, m, folded):
        """Upload every layer's (w, b) and let the library's packer lay them out (VGG, ResNet)."""
        dev = m.dev
        m._w_dev, m._b_dev = [], []
        for w, b in folded:
            m._w_dev.append(dev.to_device(np.ascontiguousarray(w)))
            m._b_dev.append(dev.to_device(np.ascontiguousarray(b)))
        n = len(folded)
        wp = (C.c_void_p * n)(*[dev.ptr(t) for t in m._w_dev])
        bp = (C.c_void_p * n)(*[dev.ptr(t) for t in m._b_dev])
        m.packed = dev.empty_bytes(max(16, self.fn(m.lib, "packed_bytes")(m.handle)))
        m.lib.check(self.fn(m.lib, "pack_weights")(m.handle, wp, bp, dev.ptr(m.packed), dev.stream()))
        dev.synchronize()


class _Vgg(_Family):
    """Layers: (cin, cout, index in model.features, BatchNorm2d inside the truncation)."""
    prefix, count, custom_op, split = "vgg16", "num_convs", True, True

    def create(self, m, handle):
        return m.lib.spr_vgg_plan_create_ex(self.arch, m.block, _COMPUTE[m.compute], handle)

    def layers(self, m):
        return [shape + info for shape, info in zip(m.conv_shapes(), m.conv_info())]

    def names(self, m, layers):  # BatchNorm2d at features.<k + 1>
        return [(f"features.{k}", f"features.{k + 1}" if bn else None) for _, _, k, bn in layers]

    def seeded(self, layers):
        return synth.vgg_parameters(1234, [l[:2] for l in layers], [l[3] for l in layers])

    def pack(self, m, layers, parameters):
        folded = []
        for (cin, cout, _, bn), p in zip(layers, parameters):
            w, b = (np.ascontiguousarray(t, dtype=np.float32) for t in p[:2])
            if bn:
                if len(p) != 6:
                    raise ValueError("a convolution followed by BatchNorm2d needs (w, b, gamma, beta, mean, var)")
                w, b = _fold_bn(w, b, *(np.asarray(t, dtype=np.float32) for t in p[2:]), self.bn_eps)
            if w.shape != (cout, cin, 3, 3) or b.shape != (cout,):
                raise ValueError(f"parameter shape {w.shape}/{b.shape} does not match conv {cin}->{cout}")
            folded.append((w, b))
        self.pack_on_device(m, folded)


class _ResNet(_Family):
    """Layers: ``Model.conv_specs`` - (cin, cout, ksize, stride, role)."""
    prefix, count, lister, seeder = "resnet", "num_convs", "conv_specs", synth.resnet_parameters

    def create(self, m, handle):
        return m.lib.spr_resnet_plan_create_ex(m.block, _COMPUTE[m.compute], handle)

    def names(self, m, layers):
        """(convolution, BatchNorm) module names in a torchvision resnet50 state dict, in conv_specs order."""
        names = [("conv1", "bn1")]
        for layer in range(m.block - 4):
            for b in range((3, 4, 6)[layer]):
                pre = f"layer{layer + 1}.{b}"
                names += [(f"{pre}.conv1", f"{pre}.bn1"), (f"{pre}.conv2", f"{pre}.bn2"), (f"{pre}.conv3", f"{pre}.bn3")]
                if b == 0:
                    names.append((f"{pre}.downsample.0", f"{pre}.downsample.1"))
        return names

    def pack(self, m, layers, parameters):
        folded = []
        for (cin, cout, ks, _stride, _role), p in zip(layers, parameters):
            if len(p) != 6:
                raise ValueError("every ResNet convolution needs (w, b, gamma, beta, running_mean, running_var)")
            w, b, *bn = (np.asarray(t, dtype=np.float32) for t in p)
            if w.shape != (cout, cin, ks, ks) or b.shape != (cout,):
                raise ValueError(f"parameter shape {w.shape}/{b.shape} does not match conv {cin}->{cout} {ks}x{ks}")
            folded.append(_fold_bn(w, b, *bn, self.bn_eps))
        self.pack_on_device(m, folded)


class _EffNet(_Family):
    """Layers: ``Model.effnet_ops``.  BatchNorm folded and parameters packed here, in numpy."""
    prefix, count, lister, seeder = "effnet", "num_ops", "effnet_ops", synth.effnet_parameters

    def create(self, m, handle):
        return m.lib.spr_effnet_plan_create_ex(self.arch, m.block, _COMPUTE[m.compute], handle)

    def names(self, m, layers):
        return effnet_state_names(layers)

    def read(self, state, op, names):
        if op["kind"] == 2:
            return _state(state, names[0], "weight", "bias") + _state(state, names[1], "weight", "bias")
        return _conv_state(state, *names)

    def pack(self, m, ops, parameters):
        packed = np.zeros(m.lib.spr_effnet_packed_bytes(m.handle) // 4, np.float32)
        packed16 = packed.view(np.uint16)  # 16-bit plans: the convolutions' weights as float16 / bfloat16 bit patterns
        half = m.compute != "float32"
        if half and len(ops) < 2:
            raise NotImplementedError("a 16-bit EfficientNet plan needs layers behind the stem (block >= 2)")

        def bits16(a):
            a = np.ascontiguousarray(a, dtype=np.float32)
            return synth.bfloat16_bits(a) if m.compute == "bfloat16" else a.astype(np.float16).view(np.uint16)

        def put(off, a):
            packed[off:off + a.size] = a.ravel()

        for k_op, (op, p) in enumerate(zip(ops, parameters)):
            p = [np.asarray(t, dtype=np.float32) for t in p]
            if op["kind"] == 2:
                w1, b1, w2, b2 = p
                c, cp, sq = op["cin"], op["cin_p"], op["sq"]
                if w1.reshape(-1).size != sq * c or w2.reshape(-1).size != c * sq:
                    raise ValueError(f"squeeze-excitation of width {c}: parameters do not match (hidden width {sq})")
                a = np.zeros((sq, cp), np.float32); a[:, :c] = w1.reshape(sq, c)
                b = np.zeros((cp, sq), np.float32); b[:c] = w2.reshape(c, sq)
                put(op["w_off"], a); put(op["b_off"], b1); put(op["w2_off"], b); put(op["b2_off"], _padded(b2, cp))
                continue
            w, b, gamma, beta, mu, var = p
            w, b = _fold_bn(w, b, gamma, beta, mu, var, self.bn_eps)
            ks, cin, cout, cin_p, cout_p = op["ks"], op["cin"], op["cout"], op["cin_p"], op["cout_p"]
            if op["kind"] == 1:
                if w.shape != (cin, 1, ks, ks):
                    raise ValueError(f"depthwise parameter shape {w.shape} does not match width {cin}, kernel {ks}")
                a = np.zeros((ks * ks, cin_p), np.float32); a[:, :cin] = w.reshape(cin, ks * ks).T
                put(op["w_off"], a); put(op["b_off"], _padded(b, cin_p))
                continue
            if w.shape != (cout, cin, ks, ks):
                raise ValueError(f"parameter shape {w.shape} does not match conv {cin}->{cout} {ks}x{ks}")
            put(op["b_off"], _padded(b, cout_p))
            if half and k_op == 0:
                # the stem of a 16-bit plan: [k / 8][64][8], k = tap * 3 + plane, 27 real values of 32 (stem16_kernel)
                ws = np.zeros((32, 64), np.float32)
                ws[:27, :cout] = w.transpose(2, 3, 1, 0).reshape(27, cout)  # [ky][kx][c][n] -> k = (ky * 3 + kx) * 3 + c
                ws = ws.reshape(4, 8, 64).transpose(0, 2, 1)               # [k / 8][n][k % 8]
                packed16[2 * op["w_off"]:2 * op["w_off"] + ws.size] = bits16(ws).ravel()
            elif half:
                wk = _gemm_layout(w, cout_p, cin_p, 64)
                packed16[2 * op["w_off"]:2 * op["w_off"] + wk.size] = bits16(wk)
            else:
                put(op["w_off"], _gemm_layout(w, cout_p, cin_p, 16))
        m.packed = m.dev.to_device(packed)


class _DenseNet(_Family):
    """Layers: ``Model.densenet_ops``; parameters per layer in torchvision's module order (synth.densenet_parameters)."""
    prefix, count, lister, seeder = "densenet", "num_ops", "densenet_ops", synth.densenet_parameters

    def create(self, m, handle):
        if m.compute != "float32" and m.block < 5:
            raise NotImplementedError("a 16-bit DenseNet plan needs a dense block behind the stem (block >= 5); "
                                      "use [mi355x].extractor_dtype = \"float32\"")
        return m.lib.spr_densenet_plan_create_ex(m.block, _COMPUTE[m.compute], handle)

    def names(self, m, layers):
        return densenet_state_names(layers)

    def read(self, state, op, names):
        bn = lambda k: _state(state, names[k], *_BN_FIELDS)
        wt = lambda k: _state(state, names[k], "weight")
        if op["kind"] == 0:
            return wt(0) + bn(1)
        if op["kind"] == 1:
            return bn(0) + wt(1) + bn(2)
        if op["kind"] == 2:
            return wt(0)
        return bn(0) + wt(1) if op["kind"] == 3 else bn(0)

    def pack(self, m, ops, parameters):
        eps = np.float32(self.bn_eps)
        packed = np.zeros(m.lib.spr_densenet_packed_bytes(m.handle) // 4, np.float32)
        packed16 = packed.view(np.uint16)  # 16-bit plans: the convolutions' weights as float16 / bfloat16 bit patterns
        half = m.compute != "float32"
        if half and m.block < 5:
            raise NotImplementedError("a 16-bit DenseNet plan needs a dense block behind the stem (block >= 5)")

        def bits16(a):
            a = np.ascontiguousarray(a, dtype=np.float32)
            return synth.bfloat16_bits(a) if m.compute == "bfloat16" else a.astype(np.float16).view(np.uint16)

        def put_w(op, w, cout_p, bn=64):
            """A GEMM convolution's weights: conv_gemm_kernel's f32 layout, or dnet_gemm16_kernel's rounded to 16 bits."""
            if half:
                wk = _gemm_layout(w, cout_p, -(-w.shape[1] // 64) * 64, 64, bn)
                packed16[2 * op["w_off"]:2 * op["w_off"] + wk.size] = bits16(wk)
            else:
                put(op["w_off"], _gemm_layout(w, cout_p, w.shape[1], 16))

        def affine(gamma, beta, mu, var):  # eval-mode BatchNorm as x * s + t (in FRONT of a convolution: not folded)
            s = gamma / np.sqrt(var + eps)
            return s, beta - mu * s

        def put(off, a):
            a = np.asarray(a, np.float32).ravel()
            packed[off:off + a.size] = a

        for op, p in zip(ops, parameters):
            p = [np.asarray(t, dtype=np.float32) for t in p]
            if op["kind"] == 0:
                w, b = p[0], np.zeros(64, np.float32)
                if w.shape != (64, 3, 7, 7):
                    raise ValueError(f"conv0 parameter shape {w.shape}")
                if op["flags"] & 1:
                    s, t = affine(*p[1:5])
                    w, b = w * s[:, None, None, None], t
                if half:  # [k / 8][64][8], k = tap * 3 + plane, 147 real values of 160 (stem16_kernel)
                    ws = np.zeros((160, 64), np.float32)
                    ws[:147] = w.transpose(2, 3, 1, 0).reshape(147, 64)
                    ws = ws.reshape(20, 8, 64).transpose(0, 2, 1)
                    packed16[2 * op["w_off"]:2 * op["w_off"] + ws.size] = bits16(ws).ravel()
                else:
                    put(op["w_off"], w.reshape(64, 3, 49).transpose(2, 1, 0))  # [tap][c][n]
                put(op["b_off"], b)
            elif op["kind"] == 1:
                s1, t1 = affine(*p[0:4])
                s2, t2 = affine(*p[5:9])
                w = p[4]
                if w.shape != (128, op["cin"], 1, 1):
                    raise ValueError(f"dense 1x1 parameter shape {w.shape} for {op['cin']} input channels")
                put(op["s_off"], s1); put(op["t_off"], t1)
                put_w(op, w * s2[:, None, None, None], 128); put(op["b_off"], t2)
            elif op["kind"] == 2:
                if p[0].shape != (32, 128, 3, 3):
                    raise ValueError(f"dense 3x3 parameter shape {p[0].shape}")
                put_w(op, p[0], 32 if half else 64, 32 if half else 64)
            elif op["kind"] == 3:
                s, t = affine(*p[0:4])
                if p[4].shape != (op["cout"], op["cin"], 1, 1):
                    raise ValueError(f"transition parameter shape {p[4].shape}")
                put(op["s_off"], s); put(op["t_off"], t)
                put_w(op, p[4], op["cout"])
            else:
                s, t = affine(*p[0:4])
                put(op["s_off"], s); put(op["t_off"], t)
        m.packed = m.dev.to_device(packed)


# model.type -> family.  arch: spr_vgg_arch / the arch id of spr_effnet_plan_create (what the C plans and the torch custom
# op are keyed by); -1 / -2: ResNet / DenseNet take none
_FAMILIES: dict[str, _Family] = {
    **{k: _Vgg(*v) for k, v in _VGG_MODELS.items()},
    **{k: _ResNet(-1, *v) for k, v in _RESNET_MODELS.items()},
    **{k: _EffNet(*v) for k, v in _EFFNET_MODELS.items()},
    "DenseNet_201": _DenseNet(-2, IMAGENET_MEAN, IMAGENET_STD, 1e-5),
}


class Model:
    """Operate on one truncated backbone (a ``_Family``) and its pre-processing (reference network.py:90-269)."""

    def __init__(self, config: dict, block: int, *, device=None, library: _lib.Library | None = None,
                 parameters: list[tuple[np.ndarray, ...]] | None = None, batch_size: int = 16):
        self.config = config
        model_cfg = config["model"]
        self.clahe_clip_limit = float(model_cfg.get("clahe_clip_limit", 2.0))
        self.clahe_tile_grid_size = tuple(model_cfg.get("clahe_tile_grid_size", (8, 8)))
        self.model_str = model_cfg["type"]
        if self.model_str not in _FAMILIES:
            raise LookupError("Model string not found")  # network.py:180-182
        fam = self.family = _FAMILIES[self.model_str]
        self.arch, self.mean, self.std, self.bn_eps = fam.arch, fam.mean, fam.std, fam.bn_eps
        self.block = int(block)
        self.batch_size = int(batch_size)
        self.lib = library or _lib.load_library()
        if device is None:
            from .device import TorchDevice

            device = TorchDevice()
        self.dev = device
        # [mi355x].extractor_dtype: compute type of the convolutions behind the first layer ("float32": the f32 matrix cores,
        # exact, the reference's arithmetic; "bfloat16" / "float16": 16-bit operands, f32 accumulation - BASELINE configs 3 / 5)
        # "bfloat16x3" (plain VGGs): float32 weights and activations split into hi + lo bfloat16, three bf16 matrix-core
        # products per float32 product - the float32 plan's accuracy class and data flow (SPR_COMPUTE_BF16X3)
        self.compute = str((config.get("mi355x") or {}).get("extractor_dtype", "float32") or "float32")
        if self.compute not in _COMPUTE:
            raise ValueError(f"[mi355x].extractor_dtype = {self.compute!r}: expected one of {sorted(_COMPUTE)}")
        if self.compute == "bfloat16x3" and not fam.split:
            raise NotImplementedError(f"{self.model_str}: extractor_dtype = \"bfloat16x3\" is built for VGG16 / VGG19 / VGG19_BN; "
                                      "use \"float32\" (or a 16-bit type)")
        if self.compute != "float32" and not fam.half:
            raise NotImplementedError(f"{self.model_str}: this backbone has no 16-bit matrix-core path; "
                                      "use [mi355x].extractor_dtype = \"float32\"")
        handle = C.c_void_p()
        self.lib.check(fam.create(self, C.byref(handle)))
        self.handle = handle
        self.n_convs = fam.fn(self.lib, fam.count)(handle)
        layers = fam.layers(self)
        if parameters is None:
            parameters = self._load_parameters(config, layers)
        if len(parameters) < len(layers):
            raise ValueError(f"{len(layers)} layers need parameters, got {len(parameters)}")
        fam.pack(self, layers, parameters)

    resnet = property(lambda self: isinstance(self.family, _ResNet))
    effnet = property(lambda self: isinstance(self.family, _EffNet))
    densenet = property(lambda self: isinstance(self.family, _DenseNet))

    def _load_parameters(self, config, layers):
        """The state dict [mi355x].weights names (torchvision's module names), else seeded stand-ins."""
        global _warned
        path = config.get("mi355x", {}).get("weights", "")
        fam = self.family
        if path:
            import torch

            state = torch.load(path, map_location="cpu", weights_only=True)
            return [fam.read(state, layer, names) for layer, names in zip(layers, fam.names(self, layers))]
        if not _warned:
            print(f"shoeprint_image_retrieval_amd: no [mi355x].weights given — using seeded synthetic {self.model_str} "
                  "weights (pretrained ImageNet weights cannot be downloaded offline)", file=sys.stderr)
            _warned = True
        return fam.seeded(layers)

    # ------------------------------------------------------------------ layers
    def _ints(self, fn, n: int, *args) -> tuple:
        """The n int32 results of fn(plan, *args, &out_0, ..)."""
        v = [C.c_int32() for _ in range(n)]
        self.lib.check(fn(self.handle, *args, *[C.byref(t) for t in v]))
        return tuple(t.value for t in v)

    def conv_shapes(self) -> list[tuple[int, int]]:
        """Plain VGG: (cin, cout) of every convolution."""
        return [self._ints(self.lib.spr_vgg16_conv_shape, 2, i) for i in range(self.n_convs)]

    def conv_info(self) -> list[tuple[int, bool]]:
        """Plain VGG: (index in model.features, BatchNorm2d inside the truncation) of every convolution."""
        return [(k, bool(bn)) for k, bn in (self._ints(self.lib.spr_vgg_conv_info, 2, i) for i in range(self.n_convs))]

    def conv_specs(self) -> list[tuple[int, int, int, int, int]]:
        """ResNet50: (cin, cout, ksize, stride, role) of every convolution in torchvision's module order."""
        return [self._ints(self.lib.spr_resnet_conv_shape, 5, i) for i in range(self.n_convs)]

    def effnet_ops(self) -> list[dict]:
        """EfficientNet: the flattened layers of features[:block]: kind (0 convolution, 1 depthwise 3x3, 2 squeeze-excitation),
        real and padded widths, kernel size, stride, activation, residual flag, hidden width, index into ``features`` and the
        offsets (floats) of the layer's parameters in the packed buffer."""
        return effnet_plan_ops(self.lib, self.handle)

    def densenet_ops(self) -> list[dict]:
        """DenseNet: the layers of features[:block]: kind (0 stem, 1 dense 1x1, 2 dense 3x3, 3 transition, 4 closing BatchNorm),
        widths, channel offset / width of the block tensor, stem flags, index into ``features`` and packed offsets (floats)."""
        return densenet_plan_ops(self.lib, self.handle)

    # ------------------------------------------------------------------ shapes
    def output_shape(self, in_h: int, in_w: int) -> tuple[int, int, int]:
        return self._ints(self.family.fn(self.lib, "output_shape"), 3, in_h, in_w)

    # ------------------------------------------------------------------ forward
    def extract_device(self, images_dev, in_channels: int = 1, out=None):
        """uint8 device batch [N,H,W] (or [N,H,W,3]) -> float32 device features [N,C,h,w] (stays in HBM).  ``out``: a dense
        device float32 [N,C,h,w] buffer to write them into (a slice of a shape class, features.FeatureSet) - the C-ABI
        route, whose entry points take the output pointer."""
        dev, fam = self.dev, self.family
        shape = dev.shape(images_dev)
        n, h, w = shape[0], shape[1], shape[2]
        if out is None and fam.custom_op and dev.name == "hip" and self.lib is _lib.load_library():
            from . import _torch_ops

            if _torch_ops.enabled() and images_dev.is_contiguous() and len(shape) == (4 if in_channels == 3 else 3):
                # the registered PyTorch-ROCm custom op (csrc/torch_ops.cpp): same plan, same kernels, current stream
                return _torch_ops.load().extract(images_dev, self.packed, self.arch, self.block, [float(m) for m in self.mean],
                                                 [float(s) for s in self.std], _COMPUTE[self.compute])
        c, oh, ow = self.output_shape(h, w)
        if out is None:
            out = dev.empty((n, c, oh, ow), np.float32)
        elif tuple(dev.shape(out)) != (n, c, oh, ow):
            raise ValueError(f"out is {tuple(dev.shape(out))}, the features are {(n, c, oh, ow)}")
        else:
            _require_dense(out)
        ws = dev.empty_bytes(max(16, fam.fn(self.lib, "workspace_bytes")(self.handle, n, h, w)))
        mean = (C.c_float * 3)(*self.mean)
        inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in self.std])
        self.lib.check(fam.fn(self.lib, "forward")(self.handle, dev.ptr(images_dev), n, h, w, in_channels, mean, inv_std,
                                                   dev.ptr(self.packed), dev.ptr(ws), dev.ptr(out), dev.stream()))
        return out

    def extract_taps_device(self, images_dev, tap_features, in_channels: int = 1):
        """One pass of the extractor that also returns the activations at ``tap_features`` - slice ends into
        ``model.features`` like ``block`` (ResNet50: into [conv1, bn1, relu, maxpool, layer1, layer2, layer3]) - as float32
        device arrays [N, C_l, h_l, w_l], in that order; a tap equal to ``block`` is the network's output.  Plain VGGs: each
        tap just behind a ReLU (16 = conv3_3, 23 = conv4_3, 30 = conv5_3 for VGG16); EfficientNets: every stage end 2 ..
        block - 1; ResNet50: 5, 6; DenseNet_201: 5 .. block - 1 (``accepted_taps``).  A tap is bit for bit the output of
        the same model truncated there.  Multi-layer scoring (BASELINE config 5) feeds on this: the reference would run the
        extractor once per block."""
        if not isinstance(self.family, _Vgg):
            return self._extract_taps_c(images_dev, tap_features, in_channels)
        dev = self.dev
        n, h, w = dev.shape(images_dev)[:3]
        info = self.conv_info()          # (index in model.features, BatchNorm inside) per convolution
        shapes = self.conv_shapes()
        c, oh, ow = self.output_shape(h, w)
        out = dev.empty((n, c, oh, ow), np.float32)
        taps, tap_convs, tap_bufs = [], [], []
        for t in tap_features:
            if t == self.block:
                taps.append(out)
                continue
            # the convolution whose ReLU ends the slice features[:t]
            ordinal = [i for i, (k, bn) in enumerate(info) if k + (2 if bn else 1) == t - 1]
            if not ordinal or ordinal[0] == 0:
                raise ValueError(f"tap {t}: not the ReLU behind one of the convolutions 1.. of features[:{self.block}]")
            i = ordinal[0]
            # spatial size of convolution i's output = image size halved once per max-pool in front of it
            pools = sum(1 for j in range(i) if self._stage_pool(j))
            hh, ww = h >> pools, w >> pools
            buf = dev.empty((n, shapes[i][1], hh, ww), np.float32)
            taps.append(buf)
            tap_convs.append(i)
            tap_bufs.append(buf)
        ws = dev.empty_bytes(max(16, self.lib.spr_vgg16_workspace_bytes(self.handle, n, h, w)))
        mean = (C.c_float * 3)(*self.mean)
        inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in self.std])
        nt = len(tap_convs)
        self.lib.check(self.lib.spr_vgg16_forward_taps(
            self.handle, dev.ptr(images_dev), n, h, w, in_channels, mean, inv_std, dev.ptr(self.packed), dev.ptr(ws),
            dev.ptr(out), nt, (C.c_int32 * max(1, nt))(*tap_convs), (C.c_void_p * max(1, nt))(*[dev.ptr(b) for b in tap_bufs]),
            dev.stream()))
        return taps

    def accepted_taps(self) -> list[int]:
        """The slice ends below ``block`` that ``extract_taps_device`` hands out (``block`` itself is always accepted)."""
        return [t for t in tap_ends(self.model_str) if t < self.block]

    def tap_shape(self, tap: int, in_h: int, in_w: int) -> tuple[int, int, int]:
        """(C, h, w) of the activation at slice end ``tap`` (ResNet50, EfficientNet, DenseNet_201): spr_*_tap_shape."""
        if tap == self.block:
            return self.output_shape(in_h, in_w)
        return self._ints(self.family.fn(self.lib, "tap_shape"), 3, tap, in_h, in_w)

    def _extract_taps_c(self, images_dev, tap_features, in_channels: int, out=None, tap_out=None):
        """``extract_taps_device`` of the families whose C entry point takes slice ends (spr_*_forward_taps).  ``out`` /
        ``tap_out`` (a dict tap -> buffer): dense device float32 buffers to write into, as ``extract_device``'s ``out``."""
        dev, fam = self.dev, self.family
        n, h, w = dev.shape(images_dev)[:3]
        want = [int(t) for t in tap_features]
        inner = [t for t in want if t != self.block]
        bad = [t for t in inner if t not in self.accepted_taps()]
        if bad or len(set(inner)) != len(inner):
            raise ValueError(f"taps {want}: {self.model_str}[:{self.block}] hands out the slice ends {self.accepted_taps()} "
                             f"(each once) and its output ({self.block})")

        def buffer(shape, given):
            if given is None:
                return dev.empty(shape, np.float32)
            if tuple(dev.shape(given)) != shape:
                raise ValueError(f"a buffer is {tuple(dev.shape(given))}, the features are {shape}")
            _require_dense(given)
            return given

        out = buffer((n,) + tuple(self.output_shape(h, w)), out)
        bufs = {t: buffer((n,) + tuple(self.tap_shape(t, h, w)), (tap_out or {}).get(t)) for t in inner}
        ws = dev.empty_bytes(max(16, fam.fn(self.lib, "workspace_bytes")(self.handle, n, h, w)))
        mean = (C.c_float * 3)(*self.mean)
        inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in self.std])
        nt = len(inner)
        self.lib.check(fam.fn(self.lib, "forward_taps")(
            self.handle, dev.ptr(images_dev), n, h, w, in_channels, mean, inv_std, dev.ptr(self.packed), dev.ptr(ws),
            dev.ptr(out), nt, (C.c_int32 * max(1, nt))(*inner), (C.c_void_p * max(1, nt))(*[dev.ptr(bufs[t]) for t in inner]),
            dev.stream()))
        return [out if t == self.block else bufs[t] for t in want]

    def _stage_pool(self, i: int) -> bool:
        """Does a max-pool follow convolution i (and its BatchNorm / ReLU) inside features[:block]?"""
        info = self.conv_info()
        k, bn = info[i]
        pool_at = k + (3 if bn else 2)  # where a pool would sit: behind the ReLU
        if i + 1 < len(info):
            return info[i + 1][0] == pool_at + 1  # the next convolution starts right behind a pool, not behind the ReLU
        return pool_at < self.block

    def clahe_device(self, images_dev):
        """CLAHE of a uint8 device batch (network.py:108-111, 197-208) - HIP kernels, stays in HBM.  [N,H,W]: on the
        image; [N,H,W,3] (RGB): on the L channel of its 8-bit L*a*b* form and back (network.py:199-204)."""
        dev = self.dev
        shape = dev.shape(images_dev)
        if len(shape) == 4:
            if shape[3] != 3:
                raise ValueError("colour images must be [N, H, W, 3] (RGB)")
            n, h, w = shape[:3]
            if getattr(self, "_color_tables", None) is None:
                from . import color

                self._color_tables = dev.to_device(color.tables())
            lab = dev.empty((n, h, w, 3), np.uint8)
            self.lib.check(self.lib.spr_rgb_to_lab_u8(dev.ptr(images_dev), dev.ptr(lab), n * h * w, dev.ptr(self._color_tables),
                                                      dev.stream()))
            dev.set_channel(lab, 0, self.clahe_device(dev.channel(lab, 0)))
            rgb = dev.empty((n, h, w, 3), np.uint8)
            self.lib.check(self.lib.spr_lab_to_rgb_u8(dev.ptr(lab), dev.ptr(rgb), n * h * w, dev.ptr(self._color_tables),
                                                      dev.stream()))
            return rgb
        n, h, w = shape
        tx, ty = int(self.clahe_tile_grid_size[0]), int(self.clahe_tile_grid_size[1])
        out = dev.empty((n, h, w), np.uint8)
        ws = dev.empty_bytes(max(16, self.lib.spr_clahe_workspace_bytes(n, tx, ty)))
        self.lib.check(self.lib.spr_clahe_u8(dev.ptr(images_dev), dev.ptr(out), n, h, w, self.clahe_clip_limit, tx, ty,
                                             dev.ptr(ws), dev.stream()))
        return out

    def _clahe(self, img: np.ndarray) -> np.ndarray:
        """CLAHE before the network (network.py:197-208): grey [H,W] or RGB [H,W,3]."""
        batch = self.dev.to_device(np.ascontiguousarray(img, dtype=np.uint8)[None])
        return self.dev.to_host(self.clahe_device(batch))[0]

    def get_feature_maps(self, img: np.ndarray) -> np.ndarray:
        """One image (uint8 [H,W]) -> float32 [C,h,w], a fresh C-contiguous array (network.py:210-244)."""
        return self.get_multiple_feature_maps([img], progress=False)[0]

    def get_multiple_feature_maps(self, images: list[np.ndarray], *, progress: bool = True) -> list[np.ndarray]:
        """List of images -> list of feature stacks (network.py:246-269).  Images of equal size are
        batched through one launch sequence; sizes may differ between images."""
        results: list[Any] = [None] * len(images)
        groups: dict[tuple, list[int]] = {}
        for i, im in enumerate(images):
            groups.setdefault(tuple(im.shape), []).append(i)
        done = 0
        for shape, idx in groups.items():
            for start in range(0, len(idx), self.batch_size):
                part = idx[start:start + self.batch_size]
                if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
                    raise ValueError("images must be grey [H,W] or RGB [H,W,3] uint8 arrays")
                # grey: transform (repeat to three planes); RGB: transform_rgb (network.py:236-241, 60-87)
                batch = self.dev.to_device(np.stack([np.ascontiguousarray(images[i], dtype=np.uint8) for i in part]))
                feats = self.dev.to_host(self.extract_device(self.clahe_device(batch), in_channels=3 if len(shape) == 3 else 1))
                for k, i in enumerate(part):
                    results[i] = np.ascontiguousarray(feats[k])
                done += len(part)
                if progress:
                    print(f"\rfeatures {done}/{len(images)}", end="" if done < len(images) else "\n", file=sys.stderr)
        return results

    def get_multiple_feature_maps_device(self, images, progress: bool = True, taps=None):
        """``get_multiple_feature_maps`` that leaves the features in HBM: a ``features.FeatureSet`` whose ``to_host_list()``
        is that function's result, bit for bit.  ``images``: a host list as there, or ``features.DeviceImages`` (the loader's
        device-resident output: nothing is uploaded).  CLAHE and extraction run per image shape class in ``batch_size``
        pieces, each piece written straight into its slice of the feature class; image classes whose features share a shape
        lie one behind the other in one feature class.  Nothing is copied to the host.
        ``taps``: slice ends as ``extract_taps_device`` takes them - then the result is a list of one ``FeatureSet`` per
        tap, in that order, all out of ONE extractor pass per image batch; item order and shape classes of each set are
        those of the single set (which the set of a tap equal to ``block`` is, bit for bit)."""
        from .features import DeviceImages, FeatureSet

        dev = self.dev
        if not isinstance(images, DeviceImages):
            images = DeviceImages.from_host(dev, images)
        if taps is not None:
            return self._tapped_feature_sets(images, [int(t) for t in taps], progress)
        total, done = len(images), 0
        # feature shape -> [(image class, first row in the feature class)], in order of first appearance
        layout: dict[tuple, list] = {}
        rows: dict[tuple, int] = {}
        for k, (shape, idx, _) in enumerate(images.classes):
            fshape = tuple(self.output_shape(shape[0], shape[1]))
            layout.setdefault(fshape, []).append((k, rows.get(fshape, 0)))
            rows[fshape] = rows.get(fshape, 0) + len(idx)
        classes = []
        for fshape, parts in layout.items():
            feats = dev.empty((rows[fshape],) + fshape, np.float32)
            for k, row0 in parts:
                shape, idx, batch = images.classes[k]
                for start in range(0, len(idx), self.batch_size):
                    n = min(self.batch_size, len(idx) - start)
                    self.extract_device(self.clahe_device(dev.narrow0(batch, start, n)), in_channels=3 if len(shape) == 3 else 1,
                                        out=dev.narrow0(feats, row0 + start, n))
                    done += n
                    if progress:
                        print(f"\rfeatures {done}/{total}", end="" if done < total else "\n", file=sys.stderr)
            classes.append((fshape, np.concatenate([images.classes[k][1] for k, _ in parts]), feats))
        return FeatureSet(dev, total, classes)

    def _tapped_feature_sets(self, images, taps: list[int], progress: bool):
        """``get_multiple_feature_maps_device`` with taps: per tap the layout of the single set (feature classes keyed by
        that tap's shape, image classes of one feature shape one behind the other), filled by one tapped pass per batch."""
        from .features import FeatureSet

        dev = self.dev
        vgg = isinstance(self.family, _Vgg)
        total, done = len(images), 0
        layouts, feats, where = [], [], []
        for t in taps:
            layout: dict[tuple, list] = {}
            rows: dict[tuple, int] = {}
            for k, (shape, idx, _) in enumerate(images.classes):
                fshape = tuple(self._vgg_tap_shape(t, shape[0], shape[1]) if vgg else self.tap_shape(t, shape[0], shape[1]))
                layout.setdefault(fshape, []).append((k, rows.get(fshape, 0)))
                rows[fshape] = rows.get(fshape, 0) + len(idx)
            layouts.append(layout)
            feats.append({fshape: dev.empty((rows[fshape],) + fshape, np.float32) for fshape in layout})
            where.append({k: (fshape, row0) for fshape, parts in layout.items() for k, row0 in parts})
        for k, (shape, idx, batch) in enumerate(images.classes):
            for start in range(0, len(idx), self.batch_size):
                n = min(self.batch_size, len(idx) - start)
                x = self.clahe_device(dev.narrow0(batch, start, n))
                dst = [dev.narrow0(feats[j][where[j][k][0]], where[j][k][1] + start, n) for j in range(len(taps))]
                in_channels = 3 if len(shape) == 3 else 1
                if vgg:  # spr_vgg16_forward_taps names convolutions: its Python route allocates, the pieces are copied in
                    index = dev.to_device(np.arange(n, dtype=np.int32))
                    for src, d in zip(self.extract_taps_device(x, taps, in_channels), dst):
                        self.lib.check(self.lib.spr_items_gather(dev.ptr(src), int(np.prod(dev.shape(src)[1:])), dev.ptr(index), n,
                                                                 dev.ptr(d), _lib.F32, dev.stream()))
                else:
                    out = [d for t, d in zip(taps, dst) if t == self.block]
                    self._extract_taps_c(x, taps, in_channels, out=out[0] if out else None,
                                         tap_out={t: d for t, d in zip(taps, dst) if t != self.block})
                done += n
                if progress:
                    print(f"\rfeatures {done}/{total}", end="" if done < total else "\n", file=sys.stderr)
        return [FeatureSet(dev, total, [(fshape, np.concatenate([images.classes[k][1] for k, _ in parts]), feats[j][fshape])
                                        for fshape, parts in layouts[j].items()]) for j in range(len(taps))]

    def _vgg_tap_shape(self, tap: int, in_h: int, in_w: int) -> tuple[int, int, int]:
        """Plain VGG: (C, h, w) of the activation at slice end ``tap`` (as ``extract_taps_device`` sizes its buffers)."""
        if tap == self.block:
            return self.output_shape(in_h, in_w)
        info = self.conv_info()
        ordinal = [i for i, (k, bn) in enumerate(info) if k + (2 if bn else 1) == tap - 1]
        if not ordinal or ordinal[0] == 0:
            raise ValueError(f"tap {tap}: not the ReLU behind one of the convolutions 1.. of features[:{self.block}]")
        pools = sum(1 for j in range(ordinal[0]) if self._stage_pool(j))
        return self.conv_shapes()[ordinal[0]][1], in_h >> pools, in_w >> pools

    def close(self):
        if getattr(self, "handle", None):
            self.family.fn(self.lib, "plan_destroy")(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
