"""Per-layer (teacher-forced) parity of the FLOAT32 extractor plans (plain VGG, ResNet50, EfficientNet, DenseNet_201), shared by
the emulated (not gpu) and MI355X (gpu) tests.  The machinery is tests/layer_cases.py's and its siblings': spr_*_forward_trace
records what every layer stored, guard bands lie around every buffer, and every layer is recomputed in float64 from the float32
records of ITS inputs as stored and the same float32 weights.  Nothing on this path is rounded to a 16-bit type, so a record
holds the kernel's own float32 arithmetic and every element is held to that layer's own rounding.

Bounds (u = 2^-24, A = |W| * |a| + |b| (+ |res|), K = the padded reduction length, C_EPI = 2 as layer_cases.C_ACC: the bias
add and one of margin; SiLU (slope <= 1.1, four roundings), the residual sum (two) and ReLU are carried through
layer_cases.interval exactly as for the 16-bit plans):

- RIGOROUS, always: |k - y64| <= (K + C_EPI) * u * A.  v_mfma_f32_16x16x4_f32 is exact float32 fused arithmetic (the kernel
  headers: bit for bit a k-ordered fmaf chain), so a reduction of K products takes at most K roundings, each of at most u times
  a partial sum that A bounds.
- TIGHT, the one that finds defects: |k - y64| <= (C_TIGHT * sqrt(K) + C_EPI) * u * A with C_TIGHT = 4.  At K = 4608 the rigorous
  bound (4608 u A) is as large as one average product of the sum (A / K ~ 3641 u A): a dropped operand hides under it.  K
  independent roundings add up like a random walk; a float32 chain simulated on a CPU over 2 * 10^5 elements per K, ReLU-type
  and signed operands, gave a worst |err| / (A u) of 4.2 (K = 27), 4.7 (576), 5.4 (2304), 5.5 (4608): at most 0.82 sqrt(K) at
  K = 27 and 0.2 sqrt(K) from K = 576 on, so 4 sqrt(K) has at least 5x margin and still lies 13x below the mean product at
  K = 4608.  The check itself asserts, for every layer, that the bound it uses is at most 1/8 of A / K (in units of A).
  Used for every convolution on the matrix cores (conv_mfma_kernel, conv_gemm_kernel's four (ks, stride) instances).
- Where the rigorous bound is already tight it is used alone: the depthwise 3x3 / 5x5 (an fmaf chain of `taps` products from
  the bias) and the stems (conv_first_kernel K = 27, stem_kernel K = 147: plain fmaf chains; the EfficientNet stem is an
  ordinary conv_gemm_kernel<3, 2> over 16 padded channels, K = 144).
- Normalisation in the stems: the oracle's operand is computed IN THE KERNEL'S FORM, float32 operation by operation -
  (u8 / 255 - mean) * (1 / std) for conv_first_kernel / stem_kernel, (u8 * (1 / 255) - mean) * (1 / std) for enet_input_kernel
  - so there is one candidate per element and no "ambiguous input" class.
- Squeeze-excitation factors (float32 [n][c] records): effnet_oracle.se_step's bound, with the mean summed in
  enet_pool_kernel's 4 strided chains.  The scaled operand x * factor is one float32 product in the kernel and in the oracle.
- Max pools (ResNet / DenseNet 3x3 / stride 2, the VGG kernels' fused 2x2): bit-exact.  DenseNet's transition average pool:
  bit-exact against ((a + b) + c) + d in float32, times 0.25 (the kernel's expression; a, b the upper row).
- DenseNet pre_s / pre_t (BatchNorm + ReLU on the operand, max(fmaf(x, s, t), 0) in float32): the oracle applies them in float64
  to the stored record, and the operand's own rounding |W| * 2u (|x s| + |t|) is added to both bounds.
- DenseNet growth slices: spr_densenet_trace_layout records a block's tensor once, complete (and the pooled tensor that starts
  it).  Every 32-channel slice is checked against the 3x3 convolution of ITS layer's 128-channel record, and the prefix the
  pool wrote must be bit-identical in the complete record - a slice written at the wrong offset shows in both.
- VGG feature taps: every tappable convolution is tapped.  The tap (float32 NCHW, before the pool) is held to the bounds; the
  record, and the last stage's `out`, equal maxpool2x2?(tap) bit for bit (odd H or W drops the last row / column).  The trace
  run with taps, the run without, the plain forward and Model.extract_taps_device agree bit for bit.
- Every run: nothing is NaN or Inf, padded channels hold 0, 4096-byte poisoned guard bands around out, the workspace (sized
  exactly by spr_*_workspace_bytes), the trace and every tap buffer stay untouched, interiors pre-filled with 0xFF bytes.

Measured worst |k - y64| / (A u) on the MI355X (tests/test_gpu_f32_layers.py, all twelve cases, one run; the report prints the
figure per layer next to both bounds, in units of u A; DESIGN.md section 7 has the table):
  matrix-core convolutions     K <= 256      K <= 1152     K <= 2304     K > 2304      largest ratio / sqrt(K)
    plain VGG                  -             5.39 (576)    4.53 (2304)   4.74 (4608)   0.23
    ResNet50                   5.05 (128)    5.77 (1024)   3.92 (2304)   -             0.62
    EfficientNet (SiLU)        8.84 (192)    8.77 (960)    7.37 (1536)   3.05 (3840)   0.71
    DenseNet_201               5.20 (256)    5.89 (608)    4.29 (1440)   -             0.64
  rigorous bound alone: stems 4.46 (K = 27, of 29), 4.45 (144, of 146), 4.02 (147, of 149); depthwise 5.11 (K = 9, of 11) and
  5.01 (K = 25, of 27).
The tight bound at those K is 34 .. 273 u A: the hardware stays below 0.71 sqrt(K) everywhere and below 0.1 sqrt(K) from K = 2304
on, as the CPU simulation did.  The emulator (a k-ordered fmaf chain) gives 2.6 .. 5.3 on its smaller shapes.
C_TIGHT changes only with a measurement recorded here: twice the worst measured ratio over sqrt(K), the 1/8 condition kept.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import densenet16_cases as dc
import layer_cases as lc
import vgg16_layer_cases as vc
from layer_cases import LayerResult, U
from oracle import effnet_oracle, resnet_oracle, vgg_oracle
from oracle.effnet_oracle import Step
from shoeprint_image_retrieval_amd import synth

F32 = "float32"
C_EPI = lc.C_ACC   # float32 roundings of an accumulation besides the reduction's own: the bias add, one of margin
C_TIGHT = 4.0      # tight bound: (C_TIGHT * sqrt(K) + C_EPI) * 2^-24 * A
FAMILY = {"VGG16": "vgg16", "VGG19": "vgg16", "VGG19_BN": "vgg16", "ResNet50": "resnet", "DenseNet_201": "densenet"}


def family(arch: str) -> str:
    return FAMILY.get(arch, "effnet")


def units_rigorous(k: int) -> float:
    return k + C_EPI


def units_tight(k: int) -> float:
    return C_TIGHT * math.sqrt(k) + C_EPI


@dataclass
class F32Result(LayerResult):
    kernel: str = ""
    k: int = 0
    tight: float = 0.0     # the bounds in units of u A (tight: 0 where the rigorous bound is used alone)
    rigorous: float = 0.0


# ---------------------------------------------------------------------------------------------------- running a trace
def raw_records(tr: np.ndarray, records, n: int) -> list:
    """The trace buffer's bytes as one float32 array per record: [n][c][h][w] (the last layer) or [n][h][w][c]."""
    raw = []
    for off, rh, rw, rc, dt, nchw in records:
        assert dt == 0, "a float32 plan stores float32 records"
        a = tr[off: off + 4 * n * rh * rw * rc].view(np.float32)
        raw.append(a.reshape(n, rc, rh, rw).copy() if nchw else a.reshape(n, rh, rw, rc).copy())
    return raw


def run_trace(m, lib, dev, imgs: np.ndarray, taps=None, plain: bool = True) -> lc.Trace:
    """One spr_*_forward_trace of the float32 network.Model `m` on imgs ([n, H, W] grey or [n, H, W, 3] RGB); `out`, the workspace
    (exactly spr_*_workspace_bytes), the trace and - plain VGG - a tap buffer per convolution in `taps` (default: every one that
    may carry a tap) between poisoned bands (layer_cases.run_guarded).  Also runs the plain forward on the same images."""
    kind = family(m.model_str)
    n, h, w = imgs.shape[:3]
    in_channels = 3 if imgs.ndim == 4 else 1
    records, total = lc.trace_records(getattr(lib, f"spr_{kind}_trace_layout"), m.handle, n, h, w)
    c, oh, ow = m.output_shape(h, w)
    sizes = [n * c * oh * ow * 4, getattr(lib, f"spr_{kind}_workspace_bytes")(m.handle, n, h, w), total]
    tap_shapes = {}
    if kind == "vgg16":
        st = vgg_oracle.stages(m.block, m.model_str)
        geo = vc.geometry(st, (h, w))
        taps = list(range(1, len(st))) if taps is None else list(taps)
        tap_shapes = {i: (n, st[i]["cout"], *geo[i]) for i in taps}
        sizes += [4 * int(np.prod(tap_shapes[i])) for i in taps]
    img_dev = dev.to_device(imgs)
    mean = (C.c_float * 3)(*m.mean)
    inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in m.std])
    fwd = getattr(lib, f"spr_{kind}_forward_trace")

    def launch(sl):
        head = (m.handle, dev.ptr(img_dev), n, h, w, in_channels, mean, inv_std, dev.ptr(m.packed), dev.ptr(sl[1]), dev.ptr(sl[0]))
        if kind == "vgg16":
            nt = len(taps)
            lib.check(fwd(*head, nt, (C.c_int32 * max(1, nt))(*taps), (C.c_void_p * max(1, nt))(*[dev.ptr(b) for b in sl[3:]]),
                          dev.ptr(sl[2]), dev.stream()))
        else:
            lib.check(fwd(*head, dev.ptr(sl[2]), dev.stream()))

    back = lc.run_guarded(dev, sizes, launch)
    out = back[0].view(np.float32).reshape(n, c, oh, ow).copy()
    tap_arrays = {i: back[3 + k].view(np.float32).reshape(tap_shapes[i]).copy() for k, i in enumerate(tap_shapes)}
    pl = np.asarray(dev.to_host(m.extract_device(img_dev, in_channels=in_channels))) if plain else None
    return lc.Trace(records, raw_records(back[2], records, n), out, pl, tap_arrays)


# ---------------------------------------------------------------------------------------------------- the records expected
def expected_records(m, hw) -> list:
    """(h, w, c, dtype, nchw) of every record of a float32 plan, restated from the oracles' own layer lists."""
    kind = family(m.model_str)
    h, w = hw
    if kind == "vgg16":
        st = vgg_oracle.stages(m.block, m.model_str)
        out = []
        for i, (s, (gh, gw)) in enumerate(zip(st, vc.geometry(st, hw))):
            gh, gw = (gh // 2, gw // 2) if s["pool"] else (gh, gw)
            out.append((gh, gw, s["cout"], 0, 1 if i + 1 == len(st) else 0))
        return out
    if kind == "resnet":
        specs = resnet_oracle.conv_specs(m.block)
        h, w = (h + 1) // 2, (w + 1) // 2
        out = [(h, w, 64, 0, 0)]
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w, 64, 0, 0))
        bl = resnet_oracle.blocks(specs)
        for kb, (i1, i2, i3, idn) in enumerate(bl):
            s2 = specs[i2][3]
            ho, wo = ((h + 1) // 2, (w + 1) // 2) if s2 == 2 else (h, w)
            out += [(h, w, specs[i1][1], 0, 0), (ho, wo, specs[i2][1], 0, 0), (ho, wo, specs[i3][1], 0, 1 if kb + 1 == len(bl) else 0)]
            if idn is not None:
                out.append((ho, wo, specs[idn][1], 0, 0))
            h, w = ho, wo
        return out
    if kind == "effnet":
        ops = m.effnet_ops()
        pad64 = lambda c: -(-c // 64) * 64
        out = []
        for i, op in enumerate(ops):
            if op["kind"] == 2:
                out.append((1, 1, pad64(op["cin"]), 0, 0))
                continue
            if op["stride"] == 2:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            out.append((h, w, op["cout"], 0, 1) if i + 1 == len(ops) else (h, w, pad64(op["cout"]), 0, 0))
        return out
    ops = m.densenet_ops()
    widths = {i: op["ctot"] for i, op in enumerate(ops) if op["kind"] == 1}
    nxt = lambda i, fallback: widths.get(i + 1, fallback)
    h, w, c = (h + 1) // 2, (w + 1) // 2, 64
    out = [(h, w, 64, 0, 0)]
    if ops[0]["flags"] & 4:
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w, nxt(0, 64), 0, 0))
    for i, op in enumerate(ops):
        if op["kind"] == 1:
            out.append((h, w, 128, 0, 0))
        elif op["kind"] == 2:
            c = op["c_off"] + 32
            if c == op["ctot"]:
                out.append((h, w, c, 0, 0))
        elif op["kind"] == 3:
            out.append((h, w, op["cout"], 0, 0))
            h, w, c = h // 2, w // 2, op["cout"]
            out.append((h, w, nxt(i, c), 0, 0))
    out.append((h, w, c, 0, 1))
    return out


def check_layout(m, lib, n: int, hw) -> list:
    """spr_*_trace_layout of a float32 plan: SPR_OK with the expected record count, every record's (h, w, c, dtype, nchw), the
    records 256-byte aligned in order and total_bytes the sum of the aligned records."""
    kind = family(m.model_str)
    records, total = lc.trace_records(getattr(lib, f"spr_{kind}_trace_layout"), m.handle, n, *hw)
    want = expected_records(m, hw)
    assert [r[1:] for r in records] == want, (records, want)
    at = 0
    for off, rh, rw, rc, _dt, _nchw in records:
        assert off == at, (records, at)
        at += (4 * n * rh * rw * rc + 255) // 256 * 256
    assert total == at, (total, at)
    return records


# ---------------------------------------------------------------------------------------------------- the element check
def _nchw(raw: np.ndarray, c_real: int) -> torch.Tensor:
    """float32 NHWC (padded) record -> float32 NCHW tensor of the real channels."""
    return torch.from_numpy(np.ascontiguousarray(raw[..., :c_real].transpose(0, 3, 1, 2)))


def check_padded(res: F32Result, raw: np.ndarray, c_real: int):
    if raw.shape[-1] > c_real and np.any(raw[..., c_real:] != 0):
        bad = np.argwhere(raw[..., c_real:] != 0)
        res.errors.append(f"{len(bad)} nonzero (or NaN) padded-channel elements, first at [n,h,w,c]="
                          f"{[int(v) for v in bad[0][:3]] + [int(bad[0][3]) + c_real]}")


def check_values(res: F32Result, got: np.ndarray, st: Step, k: int, act: str, tight: bool = True, extra=None):
    """got (float32 NCHW, real channels) against the layer restated as st: the accumulation error units * u * A_conv (+ extra,
    an absolute term: the operand's own rounding) carried through the epilogue by layer_cases.interval, for the tight bound
    (where the layer has one) and the rigorous one; an element outside either is reported against both."""
    res.k, res.rigorous, res.tight = k, units_rigorous(k), units_tight(k) if tight else 0.0
    used = res.tight or res.rigorous
    # the bound that finds defects must stay well below one average product A / K of the sum
    assert used * U <= 1.0 / (8 * k), f"layer {res.index} ({res.type}): the bound {used:.1f} u A exceeds 1/8 of A / K at K = {k}"
    if tuple(got.shape) != tuple(st.y.shape):
        res.errors.append(f"shape {tuple(got.shape)}, expected {tuple(st.y.shape)}")
        return
    res.n += got.size
    if not np.all(np.isfinite(got)):
        bad = np.argwhere(~np.isfinite(got))
        res.errors.append(f"{len(bad)} NaN / Inf, first at [n,c,y,x]={[int(v) for v in bad[0]]}")
        return
    g64, y = got.astype(np.float64), st.y.numpy()
    a_conv = st.A if st.res is None else st.A - st.res.abs()
    dev = np.abs(g64 - y)
    res.worst_acc = max(res.worst_acc, float((dev / np.maximum(st.A.numpy() * U, 1e-300)).max()))
    ratios = {}
    for name, units in (("tight", res.tight), ("rigorous", res.rigorous)):
        if not units:
            continue
        e_acc = units * U * a_conv
        if extra is not None:
            e_acc = e_acc + extra
        lo, hi = (t.numpy() for t in lc.interval(st, e_acc, act))
        e = np.maximum(np.maximum(hi - y, y - lo), 1e-300)
        ratios[name] = (dev / e, (g64 < lo) | (g64 > hi), lo, hi)
    first = "tight" if res.tight else "rigorous"
    res.worst = max(res.worst, float(ratios[first][0].max()))
    for name, (ratio, bad, lo, hi) in ratios.items():
        if not np.any(bad):
            continue
        i = np.unravel_index(int(np.argmax(np.where(bad, ratio, 0))), ratio.shape)
        units = {"tight": res.tight, "rigorous": res.rigorous}
        both = ", ".join(f"{rt[0][i]:.3f} x the {nm} bound ({units[nm]:.1f} u A)" for nm, rt in ratios.items())
        res.errors.append(f"{res.kernel}: {int(np.count_nonzero(bad))} of {got.size} values outside the {name} bound, worst at image "
                          f"{int(i[0])} channel {int(i[1])} pixel (y, x) = ({int(i[2])}, {int(i[3])}): got {g64[i]!r}, want {y[i]!r} in "
                          f"[{lo[i]!r}, {hi[i]!r}], |k - y64| = {dev[i] / max(float(st.A.numpy()[i]) * U, 1e-300):.2f} u A = {both}")
        break


def check_exact(res: F32Result, got: np.ndarray, want: np.ndarray, what: str):
    res.n += got.size
    if got.shape != want.shape:
        res.errors.append(f"{res.kernel}: {what}: shape {got.shape}, expected {want.shape}")
    elif not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        i = tuple(bad[0])
        res.errors.append(f"{res.kernel}: {what}: {len(bad)} of {got.size} values differ, first at {[int(v) for v in i]}: got "
                          f"{float(got[i])!r}, want {float(want[i])!r}")


def stem_operand(imgs: np.ndarray, mean, std, form: str = "divide") -> torch.Tensor:
    """The normalised image in the kernel's own float32 form, NCHW: (u8 / 255 - mean) * (1 / std) (conv_first_kernel,
    stem_kernel) or, form "reciprocal", (u8 * (1 / 255) - mean) * (1 / std) (enet_input_kernel)."""
    u8 = imgs.astype(np.float32)
    x = u8 / np.float32(255.0) if form == "divide" else u8 * (np.float32(1.0) / np.float32(255.0))
    x = x.transpose(0, 3, 1, 2) if imgs.ndim == 4 else np.repeat(x[:, None], 3, axis=1)
    m = np.asarray(mean, np.float32)[None, :, None, None]
    inv = np.asarray([np.float32(1.0) / np.float32(s) for s in std], np.float32)[None, :, None, None]
    return torch.from_numpy(np.ascontiguousarray(((x - m) * inv).astype(np.float32)))


# ---------------------------------------------------------------------------------------------------- plain VGG
def vgg_context(m, imgs: np.ndarray) -> dict:
    arch = m.model_str
    st = vgg_oracle.stages(m.block, arch)
    assert m.conv_shapes() == [(s["cin"], s["cout"]) for s in st] == vgg_oracle.conv_shapes(m.block, arch)
    assert [bn for _, bn in m.conv_info()] == [s["bn"] for s in st]
    params = synth.vgg_parameters(1234, m.conv_shapes(), [s["bn"] for s in st])
    _, _, mean, std = vgg_oracle.ARCHS[arch]
    assert tuple(m.mean) == tuple(mean) and tuple(m.std) == tuple(std)
    return dict(kind="vgg16", arch=arch, block=m.block, stages=st, params=list(params), stem_input=stem_operand(imgs, mean, std))


def check_vgg_layer(ctx, raw, taps, i: int, out: np.ndarray | None = None) -> F32Result:
    """Stage i: raw = the records, taps = {convolution: float32 NCHW tap}; out: the forward's output, checked with the last."""
    st, params = ctx["stages"], ctx["params"]
    s, last = st[i], i + 1 == len(st)
    act = "relu" if s["relu"] else ""
    name = f"conv 3x3, K = {27 if i == 0 else 9 * s['cin']}" + ("" if s["relu"] else ", no ReLU") + (", pool" if s["pool"] else "")
    res = F32Result(i, ("stem " if i == 0 else "") + name + (" -> out" if last else ""),
                    kernel="conv_first_kernel" if i == 0 else "conv_mfma_kernel")
    if i == 0:
        r = vgg_oracle.conv16(ctx["stem_input"], params[0], None, s["relu"], False, s["bn"], dtype=torch.float64, bound=True)
        got = raw[0] if last else np.ascontiguousarray(raw[0].transpose(0, 3, 1, 2))
        check_values(res, got, r, 27, act, tight=False)
        if last and out is not None:
            check_exact(res, out, raw[0], "out against the last record")
        return res
    tap = taps.get(i)
    if tap is None:
        res.errors.append("no feature tap for this convolution")
        return res
    r = vgg_oracle.conv16(_nchw(raw[i - 1], s["cin"]), params[i], None, s["relu"], False, s["bn"], dtype=torch.float64, bound=True)
    check_values(res, tap, r, r.K, act)
    if not np.all(np.isfinite(tap)) or tap.shape != tuple(r.y.shape):
        return res
    want = vc.pool2(tap) if s["pool"] else tap
    if last:
        check_exact(res, raw[i], want, "the last record against maxpool2x2?(tap)")
        if out is not None:
            check_exact(res, out, want, "out against maxpool2x2?(tap)")
    else:
        check_exact(res, raw[i], np.ascontiguousarray(want.transpose(0, 2, 3, 1)), "the record against maxpool2x2?(tap)")
    return res


def check_vgg_trace(ctx, tr) -> list:
    return [check_vgg_layer(ctx, tr.raw, tr.taps, i, tr.out) for i in range(len(ctx["stages"]))]


# ---------------------------------------------------------------------------------------------------- ResNet50
def resnet_context(m, imgs: np.ndarray) -> dict:
    specs = m.conv_specs()
    assert [tuple(s) for s in specs] == [tuple(s) for s in resnet_oracle.conv_specs(m.block)]
    return dict(kind="resnet", specs=specs, params=synth.resnet_parameters(1234, specs),
                stem_input=stem_operand(imgs, resnet_oracle.MEAN, resnet_oracle.STD))


def check_resnet_trace(ctx, tr) -> list:
    specs, params, raw = ctx["specs"], ctx["params"], tr.raw
    results = []
    res = F32Result(0, "stem 7x7 / 2, K = 147", kernel="stem_kernel")
    st = resnet_oracle.conv16(ctx["stem_input"], params[0], 2, 3, None, relu=True, dtype=torch.float64, bound=True)
    check_values(res, _nchw(raw[0], 64).numpy(), st, 147, "relu", tight=False)
    results.append(res)
    res = F32Result(1, "max pool 3x3 / 2", kernel="maxpool3_kernel")
    check_exact(res, _nchw(raw[1], 64).numpy(), F.max_pool2d(_nchw(raw[0], 64), 3, 2, 1).numpy(), "the max pool of the stem's record")
    results.append(res)
    bl = resnet_oracle.blocks(specs)
    x_rec = 1
    for kb, (i1, i2, i3, idn) in enumerate(bl):
        x = _nchw(raw[x_rec], specs[i1][0])
        t1 = _nchw(raw[1 + i1], specs[i1][1])
        t2 = _nchw(raw[1 + i2], specs[i2][1])
        r = x if idn is None else _nchw(raw[1 + idn], specs[idn][1])
        steps = [(i1, x, 1, 0, None, True, "conv 1x1"), (i2, t1, specs[i2][3], 1, None, True, f"conv 3x3 / {specs[i2][3]}"),
                 (i3, t2, 1, 0, r, True, "conv 1x1 + residual")]
        if idn is not None:
            steps.append((idn, x, specs[idn][3], 0, None, False, f"downsample 1x1 / {specs[idn][3]}"))
        for ci, a, stride, pad, rr, relu, name in steps:
            last = ci == i3 and kb + 1 == len(bl)
            res = F32Result(1 + ci, name + (" -> out" if last else ""), kernel=f"conv_gemm_kernel<{specs[ci][2]}, {stride}>")
            st = resnet_oracle.conv16(a, params[ci], stride, pad, None, res=rr, relu=relu, dtype=torch.float64, bound=True)
            got = raw[1 + ci] if last else _nchw(raw[1 + ci], specs[ci][1]).numpy()
            check_values(res, got, st, st.K, "relu" if relu else "")
            if last:
                check_exact(res, tr.out, raw[1 + ci], "out against the last record")
            results.append(res)
        x_rec = 1 + i3
    return results


# ---------------------------------------------------------------------------------------------------- EfficientNet
def effnet_context(m, imgs: np.ndarray) -> dict:
    ops = m.effnet_ops()
    return dict(kind="effnet", ops=ops, params=synth.effnet_parameters(1234, ops), bn_eps=m.bn_eps,
                stem_input=stem_operand(imgs, m.mean, m.std, "reciprocal"))


def effnet_inputs(ops, raw, i: int):
    """(x, block_in, scale) of layer i >= 1 from the trace (layer_cases.effnet_inputs for float32 records)."""
    j = i - 1
    while ops[j]["kind"] == 2:
        j -= 1
    x = _nchw(raw[j], ops[j]["cout"])
    b = max(k for k in range(i) if ops[k]["kind"] != 2 and ops[k]["block_end"])
    block_in = _nchw(raw[b], ops[b]["cout"])
    scale = None
    if ops[i]["kind"] == 0 and ops[i - 1]["kind"] == 2:
        scale = torch.from_numpy(np.ascontiguousarray(raw[i - 1][:, 0, 0, : ops[i]["cin"]]))[:, :, None, None]
    return x, block_in, scale


def check_effnet_layer(ctx, raw, i: int, out: np.ndarray | None = None) -> F32Result:
    ops, params, eps = ctx["ops"], ctx["params"], ctx["bn_eps"]
    op, last = ops[i], i + 1 == len(ops)
    act = "silu" if op["act"] == 2 else ""
    got = (lambda: raw[i] if last else _nchw(raw[i], op["cout"]).numpy())
    if op["kind"] == 2:
        res = F32Result(i, "squeeze-excitation factors", kernel="enet_pool_kernel + enet_fc1_kernel + enet_fc2_kernel")
        x = effnet_inputs(ops, raw, i)[0]
        f, e = effnet_oracle.se_step(op, params[i], x, dtype=torch.float64, bound=True, pool_chains=4)
        lc._check_f32(res, raw[i][:, 0, 0, : op["cin"]], f[:, :, 0, 0], (f - e)[:, :, 0, 0], (f + e)[:, :, 0, 0])
        if not np.all(np.isfinite(raw[i])):
            res.errors.append("NaN / Inf in the padded factors")
        return res
    if i == 0:
        res = F32Result(0, "stem 3x3 / 2, K = 144 (16 padded planes)" + (" -> out" if last else ""), kernel="conv_gemm_kernel<3, 2>")
        st = effnet_oracle.step16(op, params[0], ctx["stem_input"], None, None, eps, None, dtype=torch.float64, bound=True)
        check_values(res, got(), st, 144, act, tight=False)
    else:
        x, block_in, scale = effnet_inputs(ops, raw, i)
        st = effnet_oracle.step16(op, params[i], x, block_in, scale, eps, None, dtype=torch.float64, bound=True)
        if op["kind"] == 1:
            res = F32Result(i, f"depthwise {op['ks']}x{op['ks']} / {op['stride']}", kernel="enet_dw_kernel")
            check_values(res, got(), st, op["ks"] ** 2, act, tight=False)
        else:
            name = (f"conv {op['ks']}x{op['ks']} / {op['stride']}" + (" + SE operand" if scale is not None else "")
                    + (" + residual" if op["res"] else "") + (" -> out" if last else ""))
            res = F32Result(i, name, kernel=f"conv_gemm_kernel<{op['ks']}, {op['stride']}>")
            check_values(res, got(), st, -(-op["cin"] // 64) * 64 * op["ks"] ** 2, act)
    if last:
        if out is not None:
            check_exact(res, out, raw[i], "out against the last record")
    else:
        check_padded(res, raw[i], op["cout"])
    return res


def check_effnet_trace(ctx, tr) -> list:
    return [check_effnet_layer(ctx, tr.raw, i, tr.out) for i in range(len(ctx["ops"]))]


# ---------------------------------------------------------------------------------------------------- DenseNet_201
def densenet_fold(ops, params) -> list:
    """densenet16_cases.fold16 without its rounding: per layer the float32 w, b and pre-activation s / t of a float32 plan."""
    out = []
    for op, p in zip(ops, params):
        p = [np.asarray(a, dtype=np.float32) for a in p]
        k = op["kind"]
        if k == 0:
            w, b = p[0], np.zeros(64, np.float32)
            if op["flags"] & 1:
                s, t = dc._affine(*p[1:5])
                w, b = w * s[:, None, None, None], t
            out.append(dict(w=np.ascontiguousarray(w), b=b))
        elif k == 1:
            s1, t1 = dc._affine(*p[0:4])
            s2, t2 = dc._affine(*p[5:9])
            out.append(dict(s=s1, t=t1, w=np.ascontiguousarray(p[4] * s2[:, None, None, None]), b=t2))
        elif k == 2:
            out.append(dict(w=p[0], b=np.zeros(32, np.float32)))
        elif k == 3:
            s, t = dc._affine(*p[0:4])
            out.append(dict(s=s, t=t, w=p[4], b=np.zeros(op["cout"], np.float32)))
        else:
            s, t = dc._affine(*p[0:4])
            out.append(dict(s=s, t=t))
    return out


def densenet_context(m, imgs: np.ndarray) -> dict:
    ops = m.densenet_ops()
    assert ops[0]["flags"] & 4, "the per-layer check covers plans with the stem's max pool (block >= 4)"
    params = synth.densenet_parameters(1234, ops)
    return dict(kind="densenet", ops=ops, params=params, folded=densenet_fold(ops, params), recs=dc.records_of(ops),
                stem_input=stem_operand(imgs, m.mean, m.std))


def preact_step(x: torch.Tensor, f: dict, relu: bool):
    """A dense / transition 1x1 from the stored block tensor x (NCHW, its first cin channels): the operand max(x s + t, 0) in
    float64, the convolution, and the absolute term the operand's own float32 rounding adds: |W| * 2u (|x s| + |t|)."""
    s = torch.from_numpy(f["s"]).double()[None, :, None, None]
    t = torch.from_numpy(f["t"]).double()[None, :, None, None]
    xs = x.double() * s
    st = dc.conv_step(F.relu(xs + t), f, 0, relu)
    with torch.no_grad():
        extra = F.conv2d(2 * U * (xs.abs() + t.abs()), torch.from_numpy(f["w"]).double().abs())
    return st, extra


def avgpool_f32(x: np.ndarray) -> np.ndarray:
    """dnet_avgpool_kernel's own expression on a float32 NCHW array: (((a + b) + c) + d) * 0.25f, a, b the upper row."""
    h, w = x.shape[2] // 2 * 2, x.shape[3] // 2 * 2
    a, b, c, d = x[:, :, 0:h:2, 0:w:2], x[:, :, 0:h:2, 1:w:2], x[:, :, 1:h:2, 0:w:2], x[:, :, 1:h:2, 1:w:2]
    return (((a + b) + c) + d) * np.float32(0.25)


def check_densenet(ctx, raw, key, out: np.ndarray | None = None) -> F32Result:
    """One check of densenet16_cases.keys_of: a record, or a 32-channel slice / the prefix of a complete block tensor."""
    ops, fd = ctx["ops"], ctx["folded"]
    r, op = key
    rec = ctx["recs"][r]
    t = rec["type"]
    if t == "stem":
        res = F32Result(r, "stem 7x7 / 2, K = 147", kernel="stem_kernel")
        relu = bool(ops[0]["flags"] & 2)
        st = dc.conv_step(ctx["stem_input"], fd[0], 3, relu, stride=2)
        check_values(res, _nchw(raw[0], 64).numpy(), st, 147, "relu" if relu else "", tight=False)
    elif t == "pool":
        res = F32Result(r, "max pool 3x3 / 2", kernel="maxpool3_kernel")
        check_exact(res, _nchw(raw[1], 64).numpy(), F.max_pool2d(_nchw(raw[0], 64), 3, 2, 1).numpy(), "the max pool of the stem's record")
    elif t in ("dense 1x1", "transition 1x1"):
        o = ops[rec["op"]]
        res = F32Result(r, t + " (pre_s / pre_t operand)", kernel="conv_gemm_kernel<1, 1>")
        st, extra = preact_step(_nchw(raw[rec["block"]], o["cin"]), fd[rec["op"]], t == "dense 1x1")
        check_values(res, _nchw(raw[r], st.y.shape[1]).numpy(), st, st.K, "relu" if t == "dense 1x1" else "", extra=extra)
    elif op == "prefix":
        res = F32Result(r, "block prefix (untouched by the growth slices)", kernel="conv_gemm_kernel<3, 1> (c_off, ldc)")
        c0 = ops[rec["layers"][0]["op1"]]["cin"]
        check_exact(res, np.ascontiguousarray(raw[r][..., :c0]), np.ascontiguousarray(raw[rec["start"]][..., :c0]),
                    f"channels [0, {c0}) of the complete block tensor against what its pool stored")
    elif t == "block":
        res = F32Result(r, "dense 3x3 (growth slice at c_off)", kernel="conv_gemm_kernel<3, 1> (c_off, ldc)")
        d1 = next(l["d1"] for l in rec["layers"] if l["op2"] == op)
        st = dc.conv_step(_nchw(raw[d1], 128), fd[op], 1, False)
        c_off = ops[op]["c_off"]
        res.index = f"{r} [{c_off}, {c_off + 32})"
        check_values(res, np.ascontiguousarray(raw[r][..., c_off: c_off + 32].transpose(0, 3, 1, 2)), st, st.K, "")
    elif t == "transition pool":
        res = F32Result(r, "transition average pool 2x2", kernel="dnet_avgpool_kernel")
        c = ops[rec["op"]]["cout"]
        check_exact(res, _nchw(raw[r], c).numpy(), avgpool_f32(_nchw(raw[rec["conv"]], c).numpy()),
                    "the average pool against ((a + b) + c) + d) * 0.25 in float32")
    else:
        res = F32Result(r, "out (NCHW copy" + (" + norm5)" if rec["op"] is not None else ")"), kernel="dnet_out_kernel")
        x = _nchw(raw[rec["tensor"]], raw[r].shape[1])
        if rec["op"] is None:
            check_exact(res, raw[r], x.numpy(), "the output against the last tensor's stored values")
        else:
            f = fd[rec["op"]]
            s = torch.from_numpy(f["s"]).double()[None, :, None, None]
            tt = torch.from_numpy(f["t"]).double()[None, :, None, None]
            y = x.double() * s + tt
            e = U * ((x.double() * s).abs() + tt.abs())
            lc._check_f32(res, raw[r], y, y - e, y + e)
        if out is not None:
            check_exact(res, out, raw[r], "out against the last record")
    return res


def check_densenet_trace(ctx, tr) -> list:
    return [check_densenet(ctx, tr.raw, key, tr.out) for key in dc.keys_of(ctx)]


# ---------------------------------------------------------------------------------------------------- cases
CONTEXT = {"vgg16": vgg_context, "resnet": resnet_context, "effnet": effnet_context, "densenet": densenet_context}
CHECK = {"vgg16": check_vgg_trace, "resnet": check_resnet_trace, "effnet": check_effnet_trace, "densenet": check_densenet_trace}


def failures(results) -> list:
    return [f"layer {r.index} ({r.type}): {'; '.join(r.errors)}" for r in results if not r.ok]


def report(results, label: str = "") -> str:
    """Per layer type: layers, elements, the worst |k - y64| / (A u) observed next to the tight and the rigorous bound."""
    rows = {}
    for r in results:
        t = rows.setdefault((r.type.replace(" -> out", ""), r.k), [0, 0, 0.0, 0.0, 0.0, r.kernel])
        t[0] += 1; t[1] += r.n; t[2] = max(t[2], r.worst_acc); t[3] = max(t[3], r.tight); t[4] = max(t[4], r.rigorous)
    lines = [f"float32 per-layer parity {label}"]
    for (name, k), (cnt, n, acc, tight, rig, kernel) in rows.items():
        s = f"  {name:48s} layers {cnt:3d}  elements {n:9d}"
        if rig:
            s += f"  K {k:5d}  worst |k-y64|/(A u) {acc:8.3f}  tight {tight:7.1f}  rigorous {rig:7.1f}"
        lines.append(s)
    return "\n".join(lines)


def check_unwritten(tr, ctx):
    """Every record is written in full (the trace's interior started as 0xFF bytes = NaN), except the channels of a DenseNet
    block tensor behind what its pool wrote."""
    for r, a in enumerate(tr.raw):
        if ctx["kind"] == "densenet" and ctx["recs"][r]["type"] in ("pool", "transition pool"):
            op = ctx["ops"][ctx["recs"][r]["op"]]
            a = a[..., : 64 if op["kind"] == 0 else op["cout"]]
        assert np.all(np.isfinite(a)), f"record {r}: {int(np.count_nonzero(~np.isfinite(a)))} NaN / Inf (or unwritten) values"


def check_layers(arch, block, hw, n, device, lib, rgb: bool = False, keep=None, runs: bool = True, plain: bool = True) -> str:
    """Trace one batch of a float32 plan (plain VGG: a tap on every convolution); check the layout, every layer, the guard
    bands and the bit-identity of the other routes to the same result (plain: the plain forward; runs: plain VGG, the trace
    run without taps and Model.extract_taps_device); returns the report."""
    m = lc.make_model(arch, block, F32, device, lib)
    try:
        assert m.compute == F32
        kind = family(arch)
        imgs = vc.images(n, hw, rgb)
        check_layout(m, lib, n, hw)
        ctx = CONTEXT[kind](m, imgs)
        tr = run_trace(m, lib, device, imgs, plain=plain)
        same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert not plain or same(tr.out, tr.plain), "trace run's out differs from the plain forward"
        assert same(tr.raw[-1], tr.out), "the last record is not the output"
        check_unwritten(tr, ctx)
        results = CHECK[kind](ctx, tr)
        text = report(results, f"{arch}[:{block}] {hw[0]}x{hw[1]} n={n}" + (" RGB" if rgb else ""))
        print(text)
        bad = failures(results)
        assert not bad, "\n".join(bad) + "\n" + text
        if kind == "vgg16" and runs and len(ctx["stages"]) > 1:
            bare = run_trace(m, lib, device, imgs, taps=[], plain=False)
            assert same(bare.out, tr.out), "out differs between the trace runs with and without taps"
            for i, (a, b) in enumerate(zip(bare.raw, tr.raw)):
                assert same(a, b), f"record {i} differs between the trace runs with and without taps"
            feats = vc.tap_features(m)
            got = m.extract_taps_device(device.to_device(imgs), [t for t, _ in feats] + [block], in_channels=3 if rgb else 1)
            device.synchronize()
            for (t, i), a in zip(feats, got):
                assert same(np.asarray(device.to_host(a)), tr.taps[i]), f"extract_taps_device: tap {t} (convolution {i}) differs"
            assert same(np.asarray(device.to_host(got[-1])), tr.out), "extract_taps_device: out differs from the trace run's"
        if keep is not None:
            keep.update(trace=tr, ctx=ctx, results=results, imgs=imgs)
        return text
    finally:
        m.close()


def check_f32_layouts(device, lib, cases):
    """spr_*_trace_layout of float32 plans: SPR_OK, the expected records, total_bytes the sum of the 256-aligned records."""
    for arch, block, n, hw in cases:
        m = lc.make_model(arch, block, F32, device, lib)
        try:
            records = check_layout(m, lib, n, hw)
            c, oh, ow = m.output_shape(*hw)
            assert records[-1][1:] == (oh, ow, c, 0, 1), (records[-1], (c, oh, ow))
        finally:
            m.close()
