"""Per-layer (teacher-forced) and end-to-end checks of the "bfloat16x3" plain-VGG extractor plans (SPR_COMPUTE_BF16X3: float32
weights and activations split into hi + lo bfloat16, three bf16 matrix-core products per float32 product; conv_x3_kernel),
shared by the emulated (not gpu) and MI355X (gpu) tests.  The machinery is tests/layer_cases.py's and tests/vgg16_layer_cases.py's:
guard bands around every buffer, float64 restatement of every layer from what the kernel itself stored, derived bounds.

The arithmetic contract and the record layout are restated HERE from include/shoeprint_mi355x.h (spr_vgg_plan_create_ex), not
imported from the library:

    split(v):  hi = round_bf16(v) (nearest even), lo = round_bf16(v - float(hi))
    record:    NHWC, per pixel and chunk of 32 channels 64 uint16 words: 32 hi patterns, then the 32 lo patterns
    sum:       y3 = sum(a_hi w_hi + a_hi w_lo + a_lo w_hi) + b;  a_lo w_lo is dropped

Per layer i >= 1, every convolution tapped (u = 2^-24, K = 9 cin, C_ACC = layer_cases.C_ACC):

1. |tap_i - relu?(y3)| <= (3 K / 32 + C_ACC) u A3 in every element, y3 and A3 (the same sum over absolute values, + |b|) in
   float64 from record i - 1 as stored and the split weights: products of bfloat16 values are exact in float32 and the
   accumulator takes one float32 rounding per MFMA step, 3 K / 32 steps.  The report prints the worst |tap - y3| / (u A3) next
   to 3 K / 32 + C_ACC (56, 110, 218 and 434 for K = 576, 1152, 2304 and 4608).
2. The same check against the restatement that lacks a_lo w_hi, and against the one that lacks a_hi w_lo, must FAIL in at least
   one element of every layer (on the CPU, from the same inputs): the bound finds a missing term.
3. Record i == split(maxpool2x2?(tap_i)) in every word; for the last stage out == the last record == maxpool2x2?(tap_i) bit for
   bit.  Odd H or W: the pool drops the last row and column.
4. Record 0 == split(output of the float32 plan cut behind conv1_1's ReLU) on the same images, bit for bit (grey and RGB).  That
   plan is block 2; with BatchNorm (VGG19_BN) block 3, since features[:2] there ends in front of the ReLU.
5. |tap_i - relu?(y64)| <= (2^-15 + (3 K / 32 + C_ACC) u) A in every element: y64 the float64 convolution of v^ = hi + lo of
   record i - 1 with the UNSPLIT float32 weights, A = |W| |v^| + |b|  (|w - w^| <= 2^-16 |w|, |a_lo w_lo| <= 2^-16 |a||w|).
6. Nothing is NaN or Inf; guard bands (layer_cases.run_guarded) around out, the workspace (exactly spr_vgg16_workspace_bytes),
   the trace and every tap buffer; the trace run with taps, the one without, the plain forward and Model.extract_taps_device
   agree bit for bit (the GPU test adds torch.ops.shoeprint_mi355x.extract / extract_taps with compute = 3).

A plan that is conv1_1 alone runs in float32 (the 16-bit plans' rule): its output is the float32 plan's bit for bit and both
trace entry points refuse it with SPR_ERR_UNSUPPORTED, as they refuse such a 16-bit plan.

End to end (check_end_to_end), VGG16 block 16 on three grey 64 x 32 images, the same seeded weights in a bfloat16x3, a float32
and a bfloat16 plan: rms(x3 - f32) must be at least 64 x smaller than rms(bf16 - f32) (unit roundoffs 2^-16 against 2^-8 = 256 x,
a factor 4 left for the float32 accumulation floor both share).  Measured, normalised by the rms of the float32 features:

    emulation:  rms(x3 - f32) 1.065e-05, max|x3 - f32| 7.568e-05, rms(bf16 - f32) 6.258e-03: ratio 587
    MI355X:     rms(x3 - f32) 1.052e-05, max|x3 - f32| 8.275e-05, rms(bf16 - f32) 6.244e-03: ratio 593

(the images are the first three prints of check_scores, through Model.get_multiple_feature_maps).  No ceiling on max|x3 - f32| is
asserted.  Per layer, the worst |tap - y3| / (u A3) measured on the MI355X is 4.2 at K = 576, 3.3 at 1152, 3.4 at 2304 and 4.2 at
4608 (bounds 56, 110, 218, 434); under the emulation, one rounding per product, 8.4, 6.8, 6.5 and 8.8
(profiles/vgg_x3_per_layer_report.txt).  The emulated K4608 case leaves check 6's other routes (four more forward passes at a
minute each) to the three cases around it; on the MI355X every case runs them.

Scores (check_scores): 3 marks (crops of three of the prints) against 6 prints of 64 x 32, block 16; the score matrices from the
bfloat16x3 features and from the float32 features agree to 1e-4 in every cell (the project's score contract) and give the same
true-match ranks.  Measured max |score(x3) - score(f32)|: 2.5e-05 under the emulation, 3.3e-05 on the MI355X.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

import layer_cases as lc
import vgg16_layer_cases as vc
from layer_cases import LayerResult, U
from oracle import effnet_oracle, vgg_oracle
from shoeprint_image_retrieval_amd import network, similarity, synth

CODE = 3          # SPR_COMPUTE_BF16X3
COMPUTE = "bfloat16x3"
UNSUPPORTED = -3
# (arch, block, (h, w), images, RGB)
CASES = {
    "conv3_3": ("VGG16", 16, (40, 24), 2, False),     # the headline block; partial tiles, two chunk counts of the shallow layers
    "K4608": ("VGG16", 30, (38, 22), 3, True),        # the longest reduction; three RGB images; pools of 19 x 11 and 9 x 5 maps
    "ends_on_pool": ("VGG16", 17, (38, 22), 2, False),  # the last stage stores pooled float32 NCHW; 19 x 11 pooled to 9 x 5
    "batchnorm": ("VGG19_BN", 27, (40, 24), 2, False),  # BatchNorm folded in float32, then split
}


# ---------------------------------------------------------------------------------------------------- the contract, restated
def _bf16(v: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split(v: np.ndarray):
    """float32 -> (hi bits, lo bits): hi = round_bf16(v), lo = round_bf16(v - float(hi)), the subtraction in float32."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    hi = _bf16(v)
    return hi, _bf16(v - _f32(hi))


def encode(t: np.ndarray) -> np.ndarray:
    """float32 NCHW -> the record's words: uint16 [n][h][w][c / 32][hi, lo][32]."""
    n, c, h, w = t.shape
    hi, lo = split(t.transpose(0, 2, 3, 1))
    return np.ascontiguousarray(np.stack([hi.reshape(n, h, w, c // 32, 32), lo.reshape(n, h, w, c // 32, 32)], axis=4))


def decode(words: np.ndarray):
    """The record's words -> (hi, lo) as float32 NCHW."""
    n, h, w, k = words.shape[:4]
    part = lambda j: np.ascontiguousarray(_f32(words[:, :, :, :, j, :]).reshape(n, h, w, k * 32).transpose(0, 3, 1, 2))
    return part(0), part(1)


# ---------------------------------------------------------------------------------------------------- running a trace
def raw_records(tr: np.ndarray, records, n: int) -> list:
    raw = []
    for off, rh, rw, rc, dt, nchw in records:
        if dt == 0:
            raw.append(tr[off: off + 4 * n * rh * rw * rc].view(np.float32).reshape(n, rc, rh, rw).copy())
        else:
            assert dt == CODE and not nchw and rc % 32 == 0, (dt, nchw, rc)
            raw.append(tr[off: off + 4 * n * rh * rw * rc].view(np.uint16).reshape(n, rh, rw, rc // 32, 2, 32).copy())
    return raw


def run_trace(m, lib, dev, imgs: np.ndarray, taps=None) -> lc.Trace:
    """vgg16_layer_cases.run_trace for records of 4 bytes per channel (no plain forward)."""
    n, h, w = imgs.shape[:3]
    in_channels = 3 if imgs.ndim == 4 else 1
    st = vgg_oracle.stages(m.block, m.model_str)
    geo = vc.geometry(st, (h, w))
    taps = list(range(1, len(st))) if taps is None else list(taps)
    records, total = lc.trace_records(lib.spr_vgg16_trace_layout, m.handle, n, h, w)
    c, oh, ow = m.output_shape(h, w)
    sizes = [n * c * oh * ow * 4, lib.spr_vgg16_workspace_bytes(m.handle, n, h, w), total]
    sizes += [n * st[i]["cout"] * geo[i][0] * geo[i][1] * 4 for i in taps]
    img_dev = dev.to_device(imgs)
    mean = (C.c_float * 3)(*m.mean)
    inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in m.std])
    nt = len(taps)

    def launch(sl):
        lib.check(lib.spr_vgg16_forward_trace(
            m.handle, dev.ptr(img_dev), n, h, w, in_channels, mean, inv_std, dev.ptr(m.packed), dev.ptr(sl[1]), dev.ptr(sl[0]),
            nt, (C.c_int32 * max(1, nt))(*taps), (C.c_void_p * max(1, nt))(*[dev.ptr(b) for b in sl[3:]]), dev.ptr(sl[2]),
            dev.stream()))

    back = lc.run_guarded(dev, sizes, launch)
    out = back[0].view(np.float32).reshape(n, c, oh, ow).copy()
    tap_arrays = {i: back[3 + k].view(np.float32).reshape(n, st[i]["cout"], *geo[i]).copy() for k, i in enumerate(taps)}
    return lc.Trace(records, raw_records(back[2], records, n), out, None, tap_arrays)


def forward_guarded(m, lib, dev, imgs: np.ndarray) -> np.ndarray:
    """spr_vgg16_forward with out and the workspace between guard bands."""
    n, h, w = imgs.shape[:3]
    c, oh, ow = m.output_shape(h, w)
    sizes = [n * c * oh * ow * 4, max(16, lib.spr_vgg16_workspace_bytes(m.handle, n, h, w))]
    img_dev = dev.to_device(imgs)
    mean = (C.c_float * 3)(*m.mean)
    inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in m.std])
    back = lc.run_guarded(dev, sizes, lambda sl: lib.check(lib.spr_vgg16_forward(
        m.handle, dev.ptr(img_dev), n, h, w, 3 if imgs.ndim == 4 else 1, mean, inv_std, dev.ptr(m.packed), dev.ptr(sl[1]),
        dev.ptr(sl[0]), dev.stream())))
    return back[0].view(np.float32).reshape(n, c, oh, ow).copy()


# ---------------------------------------------------------------------------------------------------- the checks
def gamma_units(k: int) -> float:
    """Float32 roundings of one accumulator: three MFMA steps per 32 products, + layer_cases.C_ACC."""
    return 3 * k / 32 + lc.C_ACC


def layer_terms(ctx, raw, i: int) -> dict:
    """Stage i >= 1 restated in float64 from record i - 1 as stored: the three products apart, the bias, A3, and the unsplit form."""
    s, p = ctx["stages"][i], ctx["params"][i]
    w, b = vgg_oracle.fold16(p, None, s["bn"])  # float32, BatchNorm folded as the library folds it; not rounded
    w_hi, w_lo = (torch.from_numpy(_f32(t)).double() for t in split(w.numpy()))
    a_hi, a_lo = (torch.from_numpy(t).double() for t in decode(raw[i - 1]))
    conv = lambda x, k: F.conv2d(x, k, None, padding=1)
    b64 = b.double()[None, :, None, None]
    hh, hl, lh = conv(a_hi, w_hi), conv(a_hi, w_lo), conv(a_lo, w_hi)
    A3 = conv(a_hi.abs(), w_hi.abs() + w_lo.abs()) + conv(a_lo.abs(), w_hi.abs()) + b64.abs()
    v = a_hi + a_lo  # exact: |lo| <= ulp_bf16(hi) / 2 and both carry 8 bits
    y64 = conv(v, w.double()) + b64
    A = conv(v.abs(), w.double().abs()) + b64.abs()
    return dict(hh=hh, hl=hl, lh=lh, b=b64, A3=A3, y64=y64, A=A, K=9 * s["cin"])


def _step(pre, A, K, relu):
    return effnet_oracle.Step(F.relu(pre) if relu else pre, A, K, pre, None)


def check_layer(ctx, raw, taps, i: int, out: np.ndarray | None = None, terms: dict | None = None) -> LayerResult:
    """Checks 1, 3 and 5 of stage i >= 1; `terms`: layer_terms(ctx, raw, i) where the caller has it already."""
    st = ctx["stages"]
    s, last = st[i], i + 1 == len(st)
    res = LayerResult(i, vc.layer_type(st, i))
    act = "relu" if s["relu"] else ""
    tap = taps.get(i)
    if tap is None:
        res.errors.append("no feature tap for this convolution")
        return res
    t = terms or layer_terms(ctx, raw, i)
    pre3 = t["hh"] + t["hl"] + t["lh"] + t["b"]
    if tuple(tap.shape) != tuple(pre3.shape):
        res.errors.append(f"tap shape {tap.shape}, expected {tuple(pre3.shape)}")
        return res
    g = gamma_units(t["K"]) * U
    r3 = _step(pre3, t["A3"], t["K"], s["relu"])
    lo, hi = lc.interval(r3, g * t["A3"], act)
    lc._check_f32(res, tap, r3.y, lo, hi, t["A3"], g / U)                      # 1: the kernel's own sum
    if not np.all(np.isfinite(tap)):
        return res
    r64 = _step(t["y64"], t["A"], t["K"], s["relu"])
    lo, hi = lc.interval(r64, (2.0 ** -15 + g) * t["A"], act)
    worst, count = res.worst, res.n
    lc._check_f32(res, tap, r64.y, lo, hi)                                      # 5: against the unsplit weights
    res.worst, res.n = worst, count  # the report's columns are check 1's
    want = vc.pool2(tap) if s["pool"] else tap                                  # 3: exact behind the tap
    rec = raw[i]
    if last:
        if not (rec.dtype == np.float32 and rec.shape == want.shape and np.array_equal(rec.view(np.uint32), want.view(np.uint32))):
            res.errors.append("the last record is not maxpool?(tap) bit for bit")
        if out is not None and not (out.shape == want.shape and np.array_equal(out.view(np.uint32), want.view(np.uint32))):
            res.errors.append("out is not maxpool?(tap) bit for bit")
    else:
        words = encode(want)
        if rec.dtype != np.uint16 or rec.shape != words.shape:
            res.errors.append(f"record {rec.dtype} {rec.shape}, expected uint16 {words.shape}")
        elif not np.array_equal(rec, words):
            bad = np.argwhere(rec != words)
            j = tuple(bad[0])
            res.errors.append(f"{len(bad)} of {rec.size} stored words are not split(maxpool?(tap)), first at "
                              f"[n,h,w,chunk,part,c]={list(map(int, j))}: stored {int(rec[j]):#06x}, expected {int(words[j]):#06x}")
    res.n += rec.size
    return res


def mutations_caught(ctx, tap: np.ndarray, i: int, t: dict) -> dict:
    """Check 2: elements of stage i's tap outside the bound of check 1 when the restatement lacks one cross term."""
    s = ctx["stages"][i]
    act = "relu" if s["relu"] else ""
    e = gamma_units(t["K"]) * U * t["A3"]
    out = {}
    for name, pre in (("a_lo w_hi missing", t["hh"] + t["hl"] + t["b"]), ("a_hi w_lo missing", t["hh"] + t["lh"] + t["b"])):
        lo, hi = lc.interval(_step(pre, t["A3"], t["K"], s["relu"]), e, act)
        out[name] = int(np.count_nonzero((tap < lo.numpy()) | (tap > hi.numpy())))
    return out


def f32_stem(arch: str, imgs: np.ndarray, device, lib) -> np.ndarray:
    """The float32 plan cut behind conv1_1's ReLU on imgs: float32 NCHW."""
    block = 3 if vgg_oracle.ARCHS[arch][1] else 2
    m = lc.make_model(arch, block, "float32", device, lib)
    try:
        assert [(s["relu"], s["pool"]) for s in vgg_oracle.stages(block, arch)] == [(True, False)]
        return forward_guarded(m, lib, device, imgs)
    finally:
        m.close()


def context(m, imgs: np.ndarray) -> dict:
    arch = m.model_str
    st = vgg_oracle.stages(m.block, arch)
    assert m.conv_shapes() == [(s["cin"], s["cout"]) for s in st] == vgg_oracle.conv_shapes(m.block, arch)
    assert [bn for _, bn in m.conv_info()] == [s["bn"] for s in st]
    params = synth.vgg_parameters(1234, m.conv_shapes(), [s["bn"] for s in st])
    return dict(arch=arch, block=m.block, stages=st, params=params)


def check_case(case: str, device, lib, ops=None, routes=True, keep=None) -> str:
    """One case of CASES through checks 1 .. 6; ops: the loaded torch operator module (GPU), or None; routes=False leaves the
    other routes to the same result (four more forward passes) to the other cases.  Returns the report."""
    arch, block, hw, n, rgb = CASES[case]
    m = lc.make_model(arch, block, COMPUTE, device, lib)
    try:
        assert m.compute == COMPUTE and lib.spr_vgg_plan_compute(m.handle) == CODE
        imgs = vc.images(n, hw, rgb)
        ctx = context(m, imgs)
        st = ctx["stages"]
        tr = run_trace(m, lib, device, imgs)
        same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert same(tr.raw[-1], tr.out), "the last record is not the output"
        geo = vc.geometry(st, hw)
        want = []
        for i, (s, (h, w)) in enumerate(zip(st, geo)):
            h, w = (h // 2, w // 2) if s["pool"] else (h, w)
            want.append((h, w, s["cout"], 0, 1) if i + 1 == len(st) else (h, w, s["cout"], CODE, 0))
        assert [r[1:] for r in tr.records] == want, (tr.records, want)
        assert all(r[0] % 256 == 0 for r in tr.records)
        # 4: the stem's record is split(the float32 plan's conv1_1)
        stem = f32_stem(arch, imgs, device, lib)
        assert np.all(np.isfinite(stem))
        assert tr.raw[0].shape == encode(stem).shape and np.array_equal(tr.raw[0], encode(stem)), \
            "record 0 is not split(conv1_1 of the float32 plan)"
        results, missed = [], []
        for i in range(1, len(st)):
            t = layer_terms(ctx, tr.raw, i)
            results.append(check_layer(ctx, tr.raw, tr.taps, i, tr.out, t))
            if results[-1].ok:
                caught = mutations_caught(ctx, tr.taps[i], i, t)
                missed += [f"layer {i} ({results[-1].type}): the bound does not show '{k}'" for k, v in caught.items() if v == 0]
        text = lc.report(results, f"{arch}[:{block}] {COMPUTE} {hw[0]}x{hw[1]} n={n}" + (" RGB" if rgb else ""))
        print(text)
        bad = vc.failures(results)
        assert not bad, "\n".join(bad) + "\n" + text
        assert not missed, "\n".join(missed)
        if not routes:
            return text
        # 6: the other routes to the same result
        in_channels = 3 if rgb else 1
        assert same(forward_guarded(m, lib, device, imgs), tr.out), "the plain forward differs from the trace run"
        bare = run_trace(m, lib, device, imgs, taps=[])
        assert same(bare.out, tr.out), "out differs between the trace runs with and without taps"
        for i, (a, b) in enumerate(zip(bare.raw, tr.raw)):
            assert a.dtype == b.dtype and np.array_equal(a, b), f"record {i} differs between the trace runs with and without taps"
        feats = vc.tap_features(m)
        img_dev = device.to_device(imgs)
        got = m.extract_taps_device(img_dev, [t for t, _ in feats] + [block], in_channels=in_channels)
        device.synchronize()
        for (t, i), a in zip(feats, got):
            assert same(np.asarray(device.to_host(a)), tr.taps[i]), f"extract_taps_device: tap {t} (convolution {i}) differs"
        assert same(np.asarray(device.to_host(got[-1])), tr.out), "extract_taps_device: out differs from the trace run's"
        if ops is not None:
            assert same(np.asarray(device.to_host(m.extract_device(img_dev, in_channels=in_channels))), tr.out)
            mean, std = [float(v) for v in m.mean], [float(v) for v in m.std]
            o = ops.extract(img_dev, m.packed, m.arch, block, mean, std, CODE)
            assert same(o.cpu().numpy(), tr.out), "torch.ops extract differs"
            want_taps = [t for t, _ in feats][-2:]
            o = ops.extract_taps(img_dev, m.packed, m.arch, block, mean, std, CODE, want_taps)
            assert len(o) == len(want_taps) + 1 and same(o[-1].cpu().numpy(), tr.out), "torch.ops extract_taps: out differs"
            for t, a in zip(want_taps, o):
                assert same(a.cpu().numpy(), tr.taps[dict(feats)[t]]), f"torch.ops extract_taps: tap {t} differs"
        if keep is not None:
            keep.update(trace=tr, ctx=ctx, results=results, imgs=imgs)
        return text
    finally:
        m.close()


def check_first_conv_alone(device, lib):
    """VGG16 block 2 on 40 x 24: the plan reports the split type, runs conv1_1 in float32 - the float32 plan's output bit for
    bit - and is refused by both trace entry points like a 16-bit plan of that block."""
    imgs = vc.images(2, (40, 24))
    m = lc.make_model("VGG16", 2, COMPUTE, device, lib)
    f = lc.make_model("VGG16", 2, "float32", device, lib)
    try:
        assert lib.spr_vgg_plan_compute(m.handle) == CODE
        assert lib.spr_vgg16_packed_bytes(m.handle) == lib.spr_vgg16_packed_bytes(f.handle)
        got, want = forward_guarded(m, lib, device, imgs), forward_guarded(f, lib, device, imgs)
        assert np.all(np.isfinite(got)) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        total = C.c_size_t(77)
        assert lib.spr_vgg16_trace_layout(m.handle, 2, 40, 24, None, C.byref(total)) == UNSUPPORTED and total.value == 77
        dummy = device.to_device(np.zeros(4096, np.uint8))
        p, f3 = device.ptr(dummy), (C.c_float * 3)()
        assert lib.spr_vgg16_forward_trace(m.handle, p, 1, 8, 8, 1, f3, f3, p, p, p, 0, None, None, p, device.stream()) == UNSUPPORTED
        device.synchronize()
        assert not np.asarray(device.to_host(dummy)).any()
    finally:
        m.close()
        f.close()


# ---------------------------------------------------------------------------------------------------- end to end
HW = (64, 32)
MARKS = ((1, (8, 4)), (3, (0, 8)), (4, (16, 0)))  # (print, top-left corner) of every 48 x 24 mark
_features = {}


def features(compute: str, device, lib):
    """(features of the six 64 x 32 prints, features of the three marks) under one plan of VGG16[:16], Model.get_multiple_feature_maps
    (CLAHE included); computed once per library and plan, shared by the two checks below and never changed."""
    key = (id(lib), device.name, compute)
    if key not in _features:
        prints = [synth.shoeprint_image(41, g, *HW) for g in range(6)]
        marks = [np.ascontiguousarray(prints[g][y: y + 48, x: x + 24]) for g, (y, x) in MARKS]
        m = lc.make_model("VGG16", 16, compute, device, lib)
        try:
            # the bfloat16 plan is only the yardstick of check_end_to_end: three prints
            gf = m.get_multiple_feature_maps(prints[:3] if compute == "bfloat16" else prints, progress=False)
            qf = [] if compute == "bfloat16" else m.get_multiple_feature_maps(marks, progress=False)
        finally:
            m.close()
        _features[key] = (gf, qf)
    return _features[key]


def check_end_to_end(device, lib) -> str:
    feats = {c: np.stack(features(c, device, lib)[0][:3]).astype(np.float64) for c in (COMPUTE, "float32", "bfloat16")}
    ref = feats["float32"]
    assert ref.shape == (3, 256, 16, 8) and all(np.all(np.isfinite(v)) for v in feats.values())
    scale = float(np.sqrt(np.mean(ref ** 2)))
    rms = lambda d: float(np.sqrt(np.mean(d ** 2))) / scale
    d3, d16 = feats[COMPUTE] - ref, feats["bfloat16"] - ref
    text = (f"VGG16[:16] on 3 x 64 x 32, normalised by rms(float32 features) = {scale:.4e}: rms(x3 - f32) {rms(d3):.3e}, "
            f"max|x3 - f32| {float(np.abs(d3).max()) / scale:.3e}, rms(bf16 - f32) {rms(d16):.3e}, "
            f"ratio {rms(d16) / max(rms(d3), 1e-300):.0f} (at least 64 asked)")
    print(text)
    assert rms(d16) > 0 and 64 * rms(d3) <= rms(d16), text
    return text


def check_scores(device, lib, scorer) -> str:
    matches = [g for g, _ in MARKS]
    cfg = {"comparison": {"n_processes": 1, "rotations": None, "scales": None}}
    mats, ranks = {}, {}
    for compute in (COMPUTE, "float32"):
        gf, qf = features(compute, device, lib)
        mats[compute] = np.asarray(scorer.score_matrix(qf, gf), dtype=np.float64)
        ranks[compute] = np.asarray(similarity.compare_maps(qf, gf, matches, cfg, scorer=scorer))
    d = float(np.abs(mats[COMPUTE] - mats["float32"]).max())
    text = f"scores 3 x 6, VGG16[:16]: max |score(x3) - score(f32)| {d:.3e} (1e-4 asked), ranks {ranks[COMPUTE].tolist()}"
    print(text)
    assert mats[COMPUTE].shape == (3, 6) and np.all(np.isfinite(mats[COMPUTE])) and d <= 1e-4, text
    assert np.array_equal(ranks[COMPUTE], ranks["float32"]), (ranks, text)
    return text


# ---------------------------------------------------------------------------------------------------- surface
def check_surface(device, lib):
    """The new compute type at the C ABI and in Model: accepted by the three plain VGGs, refused (a null handle, a message
    naming the mode) by the other backbones, still no storage type of the scorer, and unknown strings still rejected."""
    from shoeprint_image_retrieval_amd import _lib
    from extractor_cases import CFG

    for arch, block in ((0, 16), (1, 18), (2, 27)):
        h = C.c_void_p()
        assert lib.spr_vgg_plan_create_ex(arch, block, CODE, C.byref(h)) == 0 and h.value
        assert lib.spr_vgg_plan_compute(h) == CODE == _lib.BF16X3
        f = C.c_void_p()
        assert lib.spr_vgg_plan_create_ex(arch, block, 0, C.byref(f)) == 0
        assert lib.spr_vgg16_packed_bytes(h) == lib.spr_vgg16_packed_bytes(f)                    # 4 bytes per weight
        assert lib.spr_vgg16_workspace_bytes(h, 3, 40, 24) == lib.spr_vgg16_workspace_bytes(f, 3, 40, 24) > 0
        lib.spr_vgg16_plan_destroy(h)
        lib.spr_vgg16_plan_destroy(f)
    h = C.c_void_p(1)
    assert lib.spr_vgg_plan_create_ex(0, 16, 4, C.byref(h)) == -1 and not h.value
    for create, args in ((lib.spr_resnet_plan_create_ex, (6,)), (lib.spr_effnet_plan_create_ex, (1, 4)),
                         (lib.spr_densenet_plan_create_ex, (6,))):
        h = C.c_void_p(1)
        assert create(*args, CODE, C.byref(h)) == UNSUPPORTED and not h.value
        assert b"BF16X3" in lib.spr_last_error()
    shape = _lib.NccShape(8, 6, 4, 8, 4, 0, CODE, 0)
    h = C.c_void_p()
    assert lib.spr_ncc_plan_create(C.byref(shape), C.byref(h)) == -1 and not h.value
    assert network._COMPUTE[COMPUTE] == CODE
    for model, block in (("ResNet50", 6), ("EfficientNetV2_M", 4), ("DenseNet_201", 6)):
        cfg = {"model": dict(CFG["model"], type=model), "mi355x": {"extractor_dtype": COMPUTE}}
        try:
            network.Model(cfg, block, device=device, library=lib)
        except NotImplementedError as e:
            assert model in str(e) and COMPUTE in str(e)
        else:
            raise AssertionError(f"{model} accepted {COMPUTE}")
    try:
        network.Model({"model": CFG["model"], "mi355x": {"extractor_dtype": "bfloat16x2"}}, 5, device=device, library=lib)
    except ValueError as e:
        assert all(name in str(e) for name in network._COMPUTE)
    else:
        raise AssertionError("an unknown extractor_dtype was accepted")
