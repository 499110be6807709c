"""Per-layer (teacher-forced) parity of the 16-bit plain-VGG extractors (VGG16, VGG19, VGG19_BN under spr_vgg_plan_create_ex),
shared by the emulated (not gpu) and MI355X (gpu) tests.  The machinery is tests/layer_cases.py's: guard bands around every
buffer, float64 restatement of every layer from the inputs the kernel itself stored, derived bounds.

spr_vgg16_forward_trace records what every stage stored, and the run taps EVERY convolution that may carry a tap (1 .. last):
the VGG kernels emit the float32 activation of a convolution (bias / ReLU applied, in front of the fused pool) next to the
16-bit record.  That splits the check in two, and makes it tighter than its siblings':

- the tap carries the only inexact step.  tap_i (float32 NCHW) must lie within interval(step, gamma_mfma(cin * 9) * A, ReLU)
  of the float64 value of oracle/vgg_oracle.conv16 on record i - 1 AS STORED, for every element (A = |W| * |x| + |b|);
- everything behind the tap is exact: record i == round16(maxpool2x2?(tap_i)) in EVERY element - no ambiguity class at all -
  and for the last stage record i == out == maxpool2x2?(tap_i) bit for bit.  Odd H or W: the pool drops the last row / column.

The stem (record 0, stem16_kernel<KIND, 3, 1>, K = 27 padded to 32: one matrix-core step) has no tap: it is held by
layer_cases._check_stored16 with e = gamma_mfma(27) * A, against the restatement from both forms of the normalised image (the
oracle divides by std, the kernel multiplies by 1 / std), padded pixels being zero AFTER normalisation.

Besides: nothing is NaN or Inf; the guard bands around out, workspace, trace and every tap buffer stay untouched (interiors
pre-filled with 0xFF bytes); the trace run's out, the plain forward's out, a trace run WITHOUT taps (records and out) and
Model.extract_taps_device (out and taps) agree bit for bit.

gamma.  layer_cases' argument for v_mfma_f32_16x16x32: products of 16-bit values are exact in float32 and the accumulator takes
one float32 rounding per 32-product step, so gamma = (ceil(K / 32) + C_ACC) * 2^-24.  A VGG reduction is 9 taps x cin / 32 chunks
of exactly 32 products each (cin is a multiple of 32 behind the stem), K = cin * 9 up to 4608: gamma / 2^-24 = 20 (K = 576),
38, 74 and 146 (K = 4608).  ResNet layer3 had measured it up to K = 2304 only.  The report prints, per layer type, the worst
|tap - y64| / (A * 2^-24) next to that figure.  Measured ratio on the MI355X at K = 4608: NOT MEASURED YET in either compute
type (no run of tests/test_gpu_vgg16_layers.py could be made when this was written; its report belongs in
profiles/vgg16_per_layer_report.txt and its summary in DESIGN.md).  The emulator (a k-ordered float32 chain, one rounding per
product, worst case K * 2^-24) stays far inside the bound because its roundings have random signs.  gamma changes only with a
written argument about the instruction, here, next to the measured ratio - and every mutation of
tests/test_emu_vgg16_layers.py must still be caught with the new value.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

import layer_cases as lc
from layer_cases import LayerResult, U
from oracle import clahe_oracle, vgg_oracle
from shoeprint_image_retrieval_amd import synth

CODE = {"float16": 1, "bfloat16": 2}
UNSUPPORTED = -3


def images(n: int, hw, rgb: bool = False) -> np.ndarray:
    """layer_cases._images, or its RGB twin [n, H, W, 3]: three decorrelated planes per print, a constant image whose planes differ."""
    if not rgb:
        return lc._images(n, hw)
    h, w = hw
    planes = lambda f: np.stack([f(c) for c in range(3)], axis=-1)
    base = planes(lambda c: synth.shoeprint_image(8 + c, 0, h, w))
    low = planes(lambda c: (112 + synth.shoeprint_image(8 + c, 1, h, w) // 8).astype(np.uint8))
    const = np.broadcast_to(np.uint8([131, 90, 200]), (h, w, 3)).copy()
    pool = [base, low, const] if n >= 3 else [base, const]
    return np.stack([pool[i % len(pool)] for i in range(n)])


def geometry(stages, hw) -> list:
    """(h, w) of every convolution's own resolution: its input's, its tap's; a pool halves (floor) what the next one sees."""
    out, (h, w) = [], hw
    for s in stages:
        out.append((h, w))
        if s["pool"]:
            h, w = h // 2, w // 2
    return out


def pool2(t: np.ndarray) -> np.ndarray:
    """2x2 / stride 2 max pool (floor) of a float32 NCHW array."""
    n, c, h, w = t.shape
    return t[:, :, : h // 2 * 2, : w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))


def stored(t: np.ndarray, compute: str, mode: str = "rne") -> np.ndarray:
    """float32 NCHW -> the 16-bit NHWC record of it."""
    return lc.f32_to_bits(np.ascontiguousarray(t.transpose(0, 2, 3, 1)), compute, mode)


# ---------------------------------------------------------------------------------------------------- running a trace
def run_trace(m, lib, dev, imgs: np.ndarray, taps=None, plain: bool = True) -> lc.Trace:
    """One spr_vgg16_forward_trace of `m` (a 16-bit plain-VGG network.Model) on imgs ([n, H, W] grey or [n, H, W, 3] RGB) with
    feature taps on the convolutions `taps` (default: every one that may carry a tap, 1 .. last); out, the workspace (exactly
    spr_vgg16_workspace_bytes), the trace and every tap buffer between poisoned bands (layer_cases.run_guarded)."""
    n, h, w = imgs.shape[:3]
    in_channels = 3 if imgs.ndim == 4 else 1
    st = vgg_oracle.stages(m.block, m.model_str)
    geo = geometry(st, (h, w))
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
    pl = np.asarray(dev.to_host(m.extract_device(img_dev, in_channels=in_channels))) if plain else None
    return lc.Trace(records, lc.raw_records(back[2], records, n), out, pl, tap_arrays)


# ---------------------------------------------------------------------------------------------------- the checks
def context(m, compute: str, imgs: np.ndarray) -> dict:
    """The oracle's own stage list of the truncation (not the library's), the seeded parameters, both forms of the stem's operand."""
    arch = m.model_str
    st = vgg_oracle.stages(m.block, arch)
    assert m.conv_shapes() == [(s["cin"], s["cout"]) for s in st] == vgg_oracle.conv_shapes(m.block, arch)
    assert [bn for _, bn in m.conv_info()] == [s["bn"] for s in st]
    params = synth.vgg_parameters(1234, m.conv_shapes(), [s["bn"] for s in st])
    _, _, mean, std = vgg_oracle.ARCHS[arch]
    assert tuple(m.mean) == tuple(mean) and tuple(m.std) == tuple(std)
    return dict(arch=arch, block=m.block, stages=st, params=params, compute=compute,
                stem_inputs=lc._normalised(imgs, mean, std, compute))


def layer_type(st, i: int) -> str:
    if i == 0:
        return "stem 3x3, K = 27"
    s = st[i]
    return (f"conv 3x3, K = {9 * s['cin']}" + ("" if s["relu"] else ", no ReLU") + (", pool" if s["pool"] else "")
            + (" -> out (f32)" if i + 1 == len(st) else ""))


def check_layer(ctx, raw, taps, i: int, out: np.ndarray | None = None) -> LayerResult:
    """Stage i of one traced batch: raw = the records, taps = {conv index: float32 NCHW tap}; out: the forward's output, checked
    with the last stage."""
    st, params, compute = ctx["stages"], ctx["params"], ctx["compute"]
    s, last = st[i], i + 1 == len(st)
    res = LayerResult(i, layer_type(st, i))
    act = "relu" if s["relu"] else ""
    if i == 0:
        cands = []
        for x in ctx["stem_inputs"]:
            r = vgg_oracle.conv16(x, params[0], compute, s["relu"], False, s["bn"], dtype=torch.float64, bound=True)
            cands.append((r.y, *lc.interval(r, lc.gamma_mfma(27) * r.A, act)))
        lc._check_stored16(res, raw[0], s["cout"], compute, cands)
        lc._check_padded(res, raw[0], s["cout"], compute)
        return res
    tap = taps.get(i)
    if tap is None:
        res.errors.append("no feature tap for this convolution")
        return res
    x = lc._vals16(raw[i - 1], compute, s["cin"])
    r = vgg_oracle.conv16(x, params[i], compute, s["relu"], False, s["bn"], dtype=torch.float64, bound=True)
    g = lc.gamma_mfma(r.K)
    lo, hi = lc.interval(r, g * r.A, act)
    if tuple(tap.shape) != tuple(r.y.shape):
        res.errors.append(f"tap shape {tap.shape}, expected {tuple(r.y.shape)}")
        return res
    lc._check_f32(res, tap, r.y, lo, hi, r.A, g / U)
    if not np.all(np.isfinite(tap)):
        return res
    want = pool2(tap) if s["pool"] else tap
    rec = raw[i]
    if last:
        ok = rec.dtype == np.float32 and rec.shape == want.shape and np.array_equal(rec.view(np.uint32), want.view(np.uint32))
        if not ok:
            res.errors.append("the last record is not maxpool?(tap) bit for bit")
        if out is not None and not (out.shape == want.shape and np.array_equal(out.view(np.uint32), want.view(np.uint32))):
            res.errors.append("out is not maxpool?(tap) bit for bit")
    else:
        bits = stored(want, compute)
        if rec.dtype != np.uint16 or rec.shape != bits.shape:
            res.errors.append(f"record {rec.dtype} {rec.shape}, expected uint16 {bits.shape}")
        elif not np.array_equal(rec, bits):
            bad = np.argwhere(rec != bits)
            j = tuple(bad[0])
            res.errors.append(f"{len(bad)} of {rec.size} stored values are not round16(maxpool?(tap)), first at [n,h,w,c]="
                              f"{list(map(int, j))}: stored {int(rec[j]):#06x}, expected {int(bits[j]):#06x}")
    res.n += rec.size
    return res


def check_trace(ctx, tr: lc.Trace) -> list:
    return [check_layer(ctx, tr.raw, tr.taps, i, tr.out) for i in range(len(ctx["stages"]))]


def failures(results) -> list:
    return [f"layer {r.index} ({r.type}): {'; '.join(r.errors)}" for r in results if not r.ok]


def tap_features(m) -> list:
    """(slice end into model.features, convolution) of every tap Model.extract_taps_device accepts besides `block` itself:
    just behind the ReLU of a convolution 1 .. of the truncation."""
    st = vgg_oracle.stages(m.block, m.model_str)
    out = []
    for i, ((k, bn), s) in enumerate(zip(m.conv_info(), st)):
        t = k + (2 if bn else 1) + 1
        if i >= 1 and s["relu"] and t < m.block:
            out.append((t, i))
    return out


# ---------------------------------------------------------------------------------------------------- end to end
def restate16(img: np.ndarray, ctx) -> np.ndarray:
    """The whole 16-bit network in float64 with the build's rounding points, on its OWN stored values (one image, already
    CLAHE'd).  Not the parity claim: the yardstick of the sanity check against the float32 network."""
    st, params, compute = ctx["stages"], ctx["params"], ctx["compute"]
    _, _, mean, std = vgg_oracle.ARCHS[ctx["arch"]]
    x = lc._normalised(img[None], mean, std, compute)[1]
    for i, (s, p) in enumerate(zip(st, params)):
        y = vgg_oracle.conv16(x, p, compute, s["relu"], s["pool"], s["bn"], dtype=torch.float64)
        x = y.to(torch.float32) if i + 1 == len(st) else vgg_oracle.round_to(y.to(torch.float32), compute)
    return x.numpy()[0]


def sanity_against_f32(ctx, imgs: np.ndarray, got: np.ndarray) -> str:
    """rms distance of the kernel's output to the float32 network, held to twice the restatement's own distance d (computed
    here, on the CPU, from the restatement alone)."""
    lines = []
    for i, img in enumerate(imgs):
        ref = vgg_oracle.get_feature_maps(img, ctx["block"], ctx["params"], ctx["arch"]).astype(np.float64)
        d = float(np.sqrt(np.mean((restate16(img, ctx).astype(np.float64) - ref) ** 2)))
        k = float(np.sqrt(np.mean((got[i].astype(np.float64) - ref) ** 2)))
        rel = float(np.abs(got[i] - ref).max() / max(np.abs(ref).max(), 1e-30))
        lines.append(f"  image {i}: rms |kernel - f32 network| {k:.3e} against 2 d = {2 * d:.3e}; largest deviation relative to "
                     f"max |f32| {rel:.3e}")
        assert k <= 2 * d, lines[-1]
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------- cases
def check_layers(arch, block, hw, n, compute, device, lib, rgb=False, keep=None, sanity=True, runs=True) -> str:
    """Trace one batch with a tap on every convolution; check every layer, the guard bands, the records' geometry, the
    bit-identity of the other routes to the same result (runs: the plain forward, a trace run without taps,
    Model.extract_taps_device) and the distance to the float32 network (sanity); returns the report."""
    m = lc.make_model(arch, block, compute, device, lib)
    try:
        assert m.compute == compute and lib.spr_vgg_plan_compute(m.handle) == CODE[compute]
        imgs = images(n, hw, rgb)
        ctx = context(m, compute, imgs)
        st = ctx["stages"]
        tr = run_trace(m, lib, device, imgs, plain=runs)
        same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert not runs or same(tr.out, tr.plain), "trace run's out differs from the plain forward"
        assert same(tr.raw[-1], tr.out), "the last record is not the output"
        # the records' geometry, from the oracle's own stage list
        geo = geometry(st, hw)
        want = []
        for i, (s, (h, w)) in enumerate(zip(st, geo)):
            h, w = (h // 2, w // 2) if s["pool"] else (h, w)
            want.append((h, w, s["cout"], 0, 1) if i + 1 == len(st) else (h, w, s["cout"], CODE[compute], 0))
        assert [r[1:] for r in tr.records] == want, (tr.records, want)
        assert all(r[0] % 256 == 0 for r in tr.records)
        results = check_trace(ctx, tr)
        text = lc.report(results, f"{arch}[:{block}] {compute} {hw[0]}x{hw[1]} n={n}" + (" RGB" if rgb else ""))
        print(text)
        bad = failures(results)
        assert not bad, "\n".join(bad) + "\n" + text
        if runs:
            # a trace run without taps: the `if (tap)` branch changes no stored value
            bare = run_trace(m, lib, device, imgs, taps=[], plain=False)
            assert same(bare.out, tr.out), "out differs between the trace runs with and without taps"
            for i, (a, b) in enumerate(zip(bare.raw, tr.raw)):
                assert a.dtype == b.dtype and np.array_equal(a, b), f"record {i} differs between the trace runs with and without taps"
            # Model.extract_taps_device: out and every tap it accepts
            feats = tap_features(m)
            in_channels = 3 if rgb else 1
            got = m.extract_taps_device(device.to_device(imgs), [t for t, _ in feats] + [block], in_channels=in_channels)
            device.synchronize()
            for (t, i), a in zip(feats, got):
                assert same(np.asarray(device.to_host(a)), tr.taps[i]), f"extract_taps_device: tap {t} (convolution {i}) differs"
            assert same(np.asarray(device.to_host(got[-1])), tr.out), "extract_taps_device: out differs from the trace run's"
        if sanity:
            s = sanity_against_f32(ctx, imgs, tr.out)
            print(s)
            text += "\n" + s
        if keep is not None:
            keep.update(trace=tr, ctx=ctx, results=results, imgs=imgs)
        return text
    finally:
        m.close()


def check_batch_invariance(arch, block, hw, compute, device, lib):
    """Image i's features in a batch of 3 equal its features extracted alone, bit for bit."""
    m = lc.make_model(arch, block, compute, device, lib)
    try:
        imgs = images(3, hw)
        batch = np.asarray(device.to_host(m.extract_device(device.to_device(imgs))))
        assert np.all(np.isfinite(batch))
        for i in range(3):
            alone = np.asarray(device.to_host(m.extract_device(device.to_device(imgs[i: i + 1]))))
            assert np.array_equal(alone[0].view(np.uint32), batch[i].view(np.uint32)), f"image {i} differs from its batch of one"
    finally:
        m.close()


def check_get_feature_maps(arch, block, hw, compute, device, lib) -> str:
    """Model.get_feature_maps (CLAHE included) of one print: bit-identical to the traced forward of the CLAHE'd image (the CPU
    oracle's CLAHE), whose every layer passes the per-layer check."""
    m = lc.make_model(arch, block, compute, device, lib)
    try:
        img = synth.shoeprint_image(7, 0, *hw)
        feats = m.get_feature_maps(img)
        pre = clahe_oracle.clahe(img, m.clahe_clip_limit, m.clahe_tile_grid_size)
        tr = run_trace(m, lib, device, pre[None], plain=False)
        ctx = context(m, compute, pre[None])
        results = check_trace(ctx, tr)
        bad = failures(results)
        assert not bad, "\n".join(bad)
        assert feats.dtype == np.float32 and feats.shape == tr.out.shape[1:]
        assert np.array_equal(feats.view(np.uint32), tr.out[0].view(np.uint32)), "get_feature_maps differs from the traced forward"
        return lc.report(results, f"get_feature_maps {arch}[:{block}] {compute}")
    finally:
        m.close()


def check_refusals(device, lib):
    """A 16-bit plan that is its first convolution alone (it runs conv_first_kernel in float32 and stores no 16-bit record): both
    trace entry points answer SPR_ERR_UNSUPPORTED and write nothing.  Float32 plans trace (tests/f32_layer_cases.py): the layout
    is SPR_OK with the expected record count, every record's (h, w, c, dtype, nchw) and total_bytes = the sum of the 256-aligned
    records - a plan that is its first convolution alone included: one float32 NCHW record.  An image that vanishes under the
    pools: SPR_ERR_SHAPE, in either compute type."""
    import f32_layer_cases as fc

    dummy = device.to_device(np.zeros(4096, np.uint8))
    p, f3 = device.ptr(dummy), (C.c_float * 3)()
    for arch, block, compute in (("VGG16", 2, "bfloat16"), ("VGG19_BN", 3, "float16")):
        m = lc.make_model(arch, block, compute, device, lib)
        try:
            total = C.c_size_t(77)
            assert lib.spr_vgg16_trace_layout(m.handle, 1, 40, 40, None, C.byref(total)) == UNSUPPORTED, (arch, block, compute)
            assert total.value == 77
            assert lib.spr_vgg16_forward_trace(m.handle, p, 1, 8, 8, 1, f3, f3, p, p, p, 0, None, None, p,
                                               device.stream()) == UNSUPPORTED, (arch, block, compute)
            device.synchronize()
            assert not np.asarray(device.to_host(dummy)).any()
        finally:
            m.close()
    for arch, block, count in (("VGG16", 10, 4), ("VGG19_BN", 9, 3), ("VGG16", 2, 1), ("VGG19_BN", 3, 1)):
        m = lc.make_model(arch, block, "float32", device, lib)
        try:
            for n, hw in ((1, (40, 40)), (3, (37, 51))):
                assert len(fc.check_layout(m, lib, n, hw)) == count, (arch, block)
            total = C.c_size_t(0)
            if count > 2:
                assert lib.spr_vgg16_trace_layout(m.handle, 1, 1, 40, None, C.byref(total)) == -2   # SPR_ERR_SHAPE
            assert lib.spr_vgg16_trace_layout(m.handle, 1, 0, 40, None, C.byref(total)) == -1       # SPR_ERR_ARG
            assert lib.spr_vgg16_forward_trace(m.handle, p, 1, 8, 8, 1, f3, f3, p, p, p, 0, None, None, None, device.stream()) == -1
        finally:
            m.close()
    m = lc.make_model("VGG16", 10, "bfloat16", device, lib)
    try:
        total = C.c_size_t(0)
        assert lib.spr_vgg16_trace_layout(m.handle, 1, 40, 40, None, C.byref(total)) == 4 and total.value > 0
        assert lib.spr_vgg16_trace_layout(m.handle, 1, 3, 40, None, C.byref(total)) == -2   # SPR_ERR_SHAPE
        assert lib.spr_vgg16_trace_layout(m.handle, 1, 0, 40, None, C.byref(total)) == -1   # SPR_ERR_ARG
        assert lib.spr_vgg16_trace_layout(None, 1, 40, 40, None, C.byref(total)) == -1
        assert lib.spr_vgg16_forward_trace(m.handle, p, 1, 8, 8, 1, f3, f3, p, p, p, 0, None, None, None, device.stream()) == -1
    finally:
        m.close()
