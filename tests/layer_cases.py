"""Per-layer (teacher-forced) parity of the 16-bit EfficientNet and ResNet extractors, shared by the emulated (not gpu) and
MI355X (gpu) tests.

spr_*_forward_trace records what every layer stored.  Each layer is recomputed in float64 from THOSE stored inputs (the
oracles' own per-layer steps: effnet_oracle.step16 / se_step, resnet_oracle.conv16) with the same rounded weights, so rounding
differences cannot build up through the network and every element can be held to that layer's own rounding:

- a 16-bit stored value: with e = gamma * A the bound on the kernel's float32 error (A = |W| * |a| + |b| (+ |res|)), the stored
  value is round16(y64) bit for bit unless [y64 - e, y64 + e] holds a rounding boundary of the type ("ambiguous"), in which
  case it is one of the values that interval rounds to; and always |k - y64| <= ulp16 / 2 + e;
- a float32 value (squeeze-excitation factors, the last layer's output): |k - y64| <= e;
- the ResNet max pool: bit-exact; every 16-bit record: padded channels hold 0; nothing is NaN or Inf.

gamma.  The convolutions run on v_mfma_f32_16x16x32_{bf16,f16}: products of 16-bit values are exact in float32, and the
accumulator takes one float32 rounding per 32-product step if the step's own sum is exact - K / 32 roundings for a reduction of
length K.  The epilogue adds the bias, SiLU (slope <= 1.1, a few roundings in expf and the division) and the residual, one
rounding each.  Hence gamma = s * (ceil(K / 32) + C_EPI) * 2^-24 with s = 1.1 behind SiLU, else 1 - not the textbook K * 2^-24,
which at K ~ 1000 is as large as the error of a missing operand re-rounding in bfloat16.  The hardware's internal order is not
documented; the float32 outputs of the last layers show the raw accumulation error directly, and the report gives the worst
observed |k - y64| / (A * 2^-24) next to ceil(K / 32) + C_EPI.  The emulator (tests/emu/spr_intrinsics.h) is a k-ordered f32
chain, one rounding per product: its worst case is K * 2^-24, its observed error (random-sign roundings) far below the bound.
The depthwise layers (an fmaf chain of taps from the bias) and the squeeze-excitation vectors (effnet_oracle.se_step) run on
the f32 vector units: their bounds are the worst case of those chains.

The stem reads the normalised image rounded to 16 bits; the kernel multiplies by 1 / std, the oracle divides.  An output
element whose receptive field holds a pixel where the two forms round differently is an "ambiguous input": it must match the
layer computed from either form (counted in the report), the rest of the layer is held to the one tight bound.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

from oracle import effnet_oracle, resnet_oracle
from shoeprint_image_retrieval_amd import network, synth

U = 2.0 ** -24
C_ACC = 2     # float32 roundings of an accumulation besides one per 32-product step: the bias add, one of margin
GUARD = 4096  # bytes of poisoned band on either side of every buffer a trace forward writes
SILU_ARGMIN, SILU_MIN = -1.2784645427610738, -0.2784645427610738  # SiLU is monotone on either side of its minimum
SILU_FLOOR = 1e-36  # v / (1 + expf(-v)) in float32 is -0 once expf overflows (v < -88.7, where |SiLU(v)| < 3e-37)


def gamma_mfma(k: int) -> float:
    """v_mfma_f32_16x16x32: one rounding per 32-product step of the padded reduction, + C_ACC."""
    return (math.ceil(k / 32) + C_ACC) * U


def gamma_dw(taps: int) -> float:  # enet_dw16_kernel: an fmaf chain of `taps` products from the bias
    return (taps + C_ACC) * U


def interval(st, e_acc: torch.Tensor, act: str):
    """[lo, hi] holding the kernel's float32 value of a layer restated as st (an effnet_oracle.Step): the accumulation
    interval pre +- e_acc carried through the activation - SiLU in front of the residual (its image of the interval, plus 4
    roundings of expf / add / divide and SILU_FLOOR), ReLU behind it - and the residual sum (2 roundings, with margin)."""
    lo, hi = st.pre - e_acc, st.pre + e_acc
    if act == "silu":
        sl, sh = F.silu(lo), F.silu(hi)
        inside = (lo <= SILU_ARGMIN) & (hi >= SILU_ARGMIN)
        lo, hi = torch.where(inside, torch.full_like(lo, SILU_MIN), torch.minimum(sl, sh)), torch.maximum(sl, sh)
        w = 4 * U * torch.maximum(lo.abs(), hi.abs()) + SILU_FLOOR
        lo, hi = lo - w, hi + w
    if st.res is not None:
        lo, hi = lo + st.res, hi + st.res
        w = 2 * U * torch.maximum(lo.abs(), hi.abs())
        lo, hi = lo - w, hi + w
    if act == "relu":
        lo, hi = F.relu(lo), F.relu(hi)
    return lo, hi


# ---------------------------------------------------------------------------------------------------- 16-bit arithmetic
def bits_to_f32(bits: np.ndarray, compute: str) -> np.ndarray:
    if compute == "float16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def f32_to_bits(v: np.ndarray, compute: str, mode: str = "rne") -> np.ndarray:
    """float32 -> 16-bit patterns, round to nearest even (the kernels' round16) or toward zero (a sensitivity mutation)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if compute == "float16":
        h = v.astype(np.float16)
        if mode == "rtz":
            over = np.abs(h.astype(np.float32)) > np.abs(v)
            h = np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)
        return h.view(np.uint16)
    b = v.view(np.uint32).astype(np.uint64)
    if mode == "rtz":
        return (b >> 16).astype(np.uint16)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def round16(v64: np.ndarray, compute: str) -> np.ndarray:
    """float64 -> the value of a 16-bit rounding (through float32: monotone, which is all the interval test needs)."""
    return bits_to_f32(f32_to_bits(np.asarray(v64, dtype=np.float32), compute), compute).astype(np.float64)


def ulp16(v: np.ndarray, compute: str) -> np.ndarray:
    mant, emin = (10, -14) if compute == "float16" else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** emin)))
    return np.exp2(e - mant)


# ---------------------------------------------------------------------------------------------------- running a trace
@dataclass
class Trace:
    records: list          # (offset, h, w, c, dtype, nchw) per record
    raw: list              # per record: uint16 [n][h][w][c] or float32 [n][c] / [n][c][h][w]
    out: np.ndarray        # the trace run's float32 output
    plain: np.ndarray      # the plain forward's output (same images)
    taps: dict = field(default_factory=dict)  # plain VGG: conv index -> float32 [n][c][h][w] feature tap of the trace run


def _images(n: int, hw) -> np.ndarray:
    """n differing images: a shoeprint, a low-contrast print, a constant image (n = 2: the print and the constant)."""
    h, w = hw
    base = synth.shoeprint_image(8, 0, h, w)
    low = (112 + synth.shoeprint_image(8, 1, h, w) // 8).astype(np.uint8)
    const = np.full((h, w), 131, np.uint8)
    pool = [base, low, const] if n >= 3 else [base, const]
    return np.stack([pool[i % len(pool)] for i in range(n)])


def trace_records(layout, handle, n: int, h: int, w: int):
    """(records, total bytes) of an spr_*_trace_layout: (offset, h, w, c, dtype, nchw) per record."""
    total = C.c_size_t(0)
    cnt = layout(handle, n, h, w, None, C.byref(total))
    assert cnt > 0, cnt
    rec = (C.c_int64 * (6 * cnt))()
    assert layout(handle, n, h, w, rec, C.byref(total)) == cnt
    return [tuple(int(v) for v in rec[6 * i: 6 * i + 6]) for i in range(cnt)], total.value


def run_guarded(dev, sizes, launch, fill: int = 0xFF, seed: int = 99) -> list:
    """Buffers of `sizes` bytes inside one allocation, each 256-byte aligned between poisoned bands of GUARD bytes that must
    stay untouched; the interiors start as `fill` bytes (all ones: NaN in every float type), so anything left unwritten shows.
    The bands hold random bytes of `seed`.  launch(buffers) enqueues the work; returns the buffers' bytes behind it (host
    arrays)."""
    starts, at = [], GUARD
    for sz in sizes:
        starts.append(at)
        at = (at + sz + GUARD + 255) // 256 * 256
    host = np.random.default_rng(seed).integers(0, 256, size=at + 256, dtype=np.uint8)
    buf = dev.to_device(host)
    shift = (-dev.ptr(buf)) % 256  # every buffer 256-byte aligned
    sl = [buf[shift + s0: shift + s0 + sz] for s0, sz in zip(starts, sizes)]
    for b in sl:
        b[:] = fill
    launch(sl)
    dev.synchronize()
    back = np.asarray(dev.to_host(buf))
    bands = np.ones(len(host), bool)
    for s0, sz in zip(starts, sizes):
        bands[shift + s0: shift + s0 + sz] = False
    bad = np.nonzero(bands & (back != host))[0]
    assert bad.size == 0, f"{bad.size} guard-band bytes overwritten, first at {bad[:8].tolist()} (buffers at {starts}, +{shift})"
    return [back[shift + s0: shift + s0 + sz] for s0, sz in zip(starts, sizes)]


def raw_records(tr: np.ndarray, records, n: int) -> list:
    """The trace buffer's bytes as one array per record."""
    raw = []
    for off, rh, rw, rc, dt, nchw in records:
        if dt == 0:
            a = tr[off: off + 4 * n * rh * rw * rc].view(np.float32)
            raw.append(a.reshape(n, rc, rh, rw).copy() if nchw else a.reshape(n, rc).copy())
        else:
            raw.append(tr[off: off + 2 * n * rh * rw * rc].view(np.uint16).reshape(n, rh, rw, rc).copy())
    return raw


def run_trace(m, lib, dev, imgs: np.ndarray) -> Trace:
    """One spr_*_forward_trace of `m` (a 16-bit effnet / resnet network.Model) on imgs, with `out`, the workspace (exactly
    spr_*_workspace_bytes) and the trace inside one allocation, each between poisoned bands that must stay untouched; the
    interiors start as all-ones bytes (NaN in every float type), so anything left unwritten shows.  Also runs the plain
    forward on the same images."""
    kind = "effnet" if m.effnet else "resnet"
    n, h, w = imgs.shape
    records, total = trace_records(getattr(lib, f"spr_{kind}_trace_layout"), m.handle, n, h, w)
    c, oh, ow = m.output_shape(h, w)
    sizes = [n * c * oh * ow * 4, getattr(lib, f"spr_{kind}_workspace_bytes")(m.handle, n, h, w), total]
    img_dev = dev.to_device(imgs)
    mean = (C.c_float * 3)(*m.mean)
    inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in m.std])
    fwd = getattr(lib, f"spr_{kind}_forward_trace")
    back = run_guarded(dev, sizes, lambda sl: lib.check(fwd(m.handle, dev.ptr(img_dev), n, h, w, 1, mean, inv_std,
                                                            dev.ptr(m.packed), dev.ptr(sl[1]), dev.ptr(sl[0]), dev.ptr(sl[2]),
                                                            dev.stream())))
    out = back[0].view(np.float32).reshape(n, c, oh, ow).copy()
    plain = np.asarray(dev.to_host(m.extract_device(img_dev)))
    return Trace(records, raw_records(back[2], records, n), out, plain)


# ---------------------------------------------------------------------------------------------------- the checks
@dataclass
class LayerResult:
    index: int
    type: str
    n: int = 0            # elements checked
    ambiguous: int = 0    # elements whose bound interval holds a rounding boundary
    ambiguous_input: int = 0  # (stems) elements whose input differs between the divided and the multiplied normalisation
    worst: float = 0.0    # max |k - y64| / bound
    worst_acc: float = 0.0  # float32 records: max |k - y64| / (A * 2^-24), the raw accumulation error
    gamma_units: float = 0.0  # ... against ceil(K / 32) + C_EPI (times 1.1 behind SiLU)
    errors: list = field(default_factory=list)

    @property
    def ok(self):
        return not self.errors


def _vals16(raw: np.ndarray, compute: str, c_real: int) -> torch.Tensor:
    """uint16 NHWC (padded) -> float32 NCHW tensor of the real channels."""
    v = bits_to_f32(raw[..., :c_real], compute)
    return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))


def _check_padded(res: LayerResult, raw: np.ndarray, c_real: int, compute: str):
    if raw.dtype == np.uint16 and raw.shape[-1] > c_real:
        pad = bits_to_f32(raw[..., c_real:], compute)
        if np.any(pad != 0):
            res.errors.append(f"{int(np.count_nonzero(pad))} nonzero padded-channel elements")


def _check_stored16(res: LayerResult, raw: np.ndarray, c_real: int, compute: str, cands):
    """cands: [(y64, lo, hi)] - the layer restated with the interval its float32 value lies in (the stem: from either input
    form, else one); an element passes if it passes against any of them."""
    got = bits_to_f32(raw[..., :c_real], compute).transpose(0, 3, 1, 2).astype(np.float64)
    res.n += got.size
    if not np.all(np.isfinite(got)):
        res.errors.append(f"{int(np.count_nonzero(~np.isfinite(got)))} NaN / Inf")
        return
    ok_any = np.zeros(got.shape, bool)
    worst = np.full(got.shape, np.inf)
    for j, (y, lo, hi) in enumerate(cands):
        y, lo, hi = y.numpy(), lo.numpy(), hi.numpy()
        rlo, rhi, near = round16(lo, compute), round16(hi, compute), round16(y, compute)
        amb = rlo != rhi
        e = np.maximum(hi - y, y - lo)
        bound = 0.5 * np.maximum(ulp16(y, compute), ulp16(got, compute)) + e
        dev = np.abs(got - y)
        ok = np.where(amb, (got >= rlo) & (got <= rhi), got == near) & (dev <= bound)
        ok_any |= ok
        worst = np.minimum(worst, dev / bound)
        if j == 0:
            res.ambiguous += int(np.count_nonzero(amb))
    if len(cands) > 1:
        res.ambiguous_input += int(np.count_nonzero(cands[0][0].numpy() != cands[1][0].numpy()))
    res.worst = max(res.worst, float(worst.max()))
    if not np.all(ok_any):
        bad = np.argwhere(~ok_any)
        i = tuple(bad[0])
        res.errors.append(f"{len(bad)} of {got.size} stored values off, first at [n,c,h,w]={list(map(int, i))}: "
                          f"got {got[i]!r}, y64 {cands[0][0].numpy()[i]!r} in [{cands[0][1].numpy()[i]!r}, "
                          f"{cands[0][2].numpy()[i]!r}]")


def _check_f32(res: LayerResult, got: np.ndarray, y: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor,
               A: torch.Tensor | None = None, units: float = 0.0):
    got = got.astype(np.float64)
    y, lo, hi = y.numpy(), lo.numpy(), hi.numpy()
    res.n += got.size
    if not np.all(np.isfinite(got)):
        res.errors.append(f"{int(np.count_nonzero(~np.isfinite(got)))} NaN / Inf")
        return
    dev = np.abs(got - y)
    e = np.maximum(np.maximum(hi - y, y - lo), 1e-300)
    res.worst = max(res.worst, float((dev / e).max()))
    if A is not None:
        res.worst_acc = max(res.worst_acc, float((dev / np.maximum(A.numpy() * U, 1e-300)).max()))
        res.gamma_units = units
    bad = (got < lo) | (got > hi)
    if np.any(bad):
        i = np.unravel_index(int(np.argmax(np.where(bad, dev / e, 0))), dev.shape)
        res.errors.append(f"{int(np.count_nonzero(bad))} of {got.size} float32 values outside the bound, worst at "
                          f"{list(map(int, i))}: got {got[i]!r}, y64 {y[i]!r} in [{lo[i]!r}, {hi[i]!r}]")


def _normalised(imgs: np.ndarray, mean, std, compute: str):
    """The stem's operand in both forms, rounded: the oracle's (x - mean) / std and the kernel's (x - mean) * (1 / std)."""
    x = torch.from_numpy(imgs.astype(np.float32) / np.float32(255.0))
    x = x.permute(0, 3, 1, 2).contiguous() if imgs.ndim == 4 else x[:, None].repeat(1, 3, 1, 1)  # RGB [N,H,W,3] | grey [N,H,W]
    m = torch.tensor(mean, dtype=torch.float32)[None, :, None, None]
    s = torch.tensor(std, dtype=torch.float32)[None, :, None, None]
    inv = torch.tensor([np.float32(1.0) / np.float32(v) for v in std], dtype=torch.float32)[None, :, None, None]
    rnd = effnet_oracle._round
    return rnd((x - m) / s, compute), rnd((x - m) * inv, compute)


# ---- EfficientNet
def effnet_inputs(ops, raw, i: int, compute: str):
    """(x, block_in, scale) of layer i >= 1 from the trace: the previous stored layer, the last block end, the squeeze-
    excitation factors in front of a scaled convolution (float32 [N, C, 1, 1])."""
    j = i - 1
    while ops[j]["kind"] == 2:
        j -= 1
    x = _vals16(raw[j], compute, ops[j]["cout"])
    b = max(k for k in range(i) if ops[k]["kind"] != 2 and ops[k]["block_end"])
    block_in = _vals16(raw[b], compute, ops[b]["cout"])
    scale = None
    if ops[i]["kind"] == 0 and ops[i - 1]["kind"] == 2:
        scale = torch.from_numpy(np.ascontiguousarray(raw[i - 1][:, : ops[i]["cin"]]))[:, :, None, None]
    return x, block_in, scale


def _effnet_type(op, i, last):
    if i == 0:
        return "stem"
    if last:
        return "out (f32)"
    if op["kind"] == 1:
        return f"depthwise {op['ks']}x{op['ks']}"
    if op["kind"] == 2:
        return "squeeze-excitation (f32)"
    return f"conv {op['ks']}x{op['ks']}" + (" + SE operand" if op.get("scaled") else "") + (" + residual" if op["res"] else "")


def check_effnet_layer(ctx, raw, i: int) -> LayerResult:
    ops, params, compute = ctx["ops"], ctx["params"], ctx["compute"]
    op, last = ops[i], i + 1 == len(ops)
    res = LayerResult(i, _effnet_type(dict(op, scaled=i > 0 and ops[i - 1]["kind"] == 2), i, last))
    if i == 0:
        cands = []
        for x in ctx["stem_inputs"]:
            st = effnet_oracle.step16(op, params[0], x, None, None, ctx["bn_eps"], compute, dtype=torch.float64, bound=True)
            cands.append((st.y, *interval(st, gamma_mfma(27) * st.A, "silu")))
        _check_stored16(res, raw[0], op["cout"], compute, cands)
        _check_padded(res, raw[0], op["cout"], compute)
        return res
    x, block_in, scale = effnet_inputs(ops, raw, i, compute)
    if op["kind"] == 2:
        f, e = effnet_oracle.se_step(op, params[i], x, dtype=torch.float64, bound=True)
        f, e = f[:, :, 0, 0], e[:, :, 0, 0]
        _check_f32(res, raw[i][:, : op["cin"]], f, f - e, f + e)
        if not np.all(np.isfinite(raw[i])):
            res.errors.append("NaN / Inf in the padded factors")
        return res
    st = effnet_oracle.step16(op, params[i], x, block_in, scale, ctx["bn_eps"], compute, dtype=torch.float64, bound=True)
    a_conv = st.A if st.res is None else st.A - st.res.abs()
    if op["kind"] == 1:
        g = gamma_dw(op["ks"] ** 2)
    else:
        g = gamma_mfma(-(-op["cin"] // 64) * 64 * op["ks"] ** 2)
    lo, hi = interval(st, g * a_conv, "silu" if op["act"] == 2 else "")
    if last:
        _check_f32(res, raw[i], st.y, lo, hi, a_conv, g / U)
    else:
        _check_stored16(res, raw[i], op["cout"], compute, [(st.y, lo, hi)])
        _check_padded(res, raw[i], op["cout"], compute)
    return res


def effnet_context(m, compute, imgs):
    ops = m.effnet_ops()
    return dict(ops=ops, params=synth.effnet_parameters(1234, ops), compute=compute, bn_eps=m.bn_eps,
                stem_inputs=_normalised(imgs, m.mean, m.std, compute))


def check_effnet_trace(ctx, raw) -> list:
    return [check_effnet_layer(ctx, raw, i) for i in range(len(ctx["ops"]))]


# ---- ResNet
def check_resnet_trace(ctx, raw) -> list:
    specs, params, compute = ctx["specs"], ctx["params"], ctx["compute"]
    results = []
    res = LayerResult(0, "stem 7x7")
    cands = []
    for x in ctx["stem_inputs"]:
        st = resnet_oracle.conv16(x, params[0], 2, 3, compute, relu=True, dtype=torch.float64, bound=True)
        cands.append((st.y, *interval(st, gamma_mfma(160) * st.A, "relu")))
    _check_stored16(res, raw[0], 64, compute, cands)
    results.append(res)
    res = LayerResult(1, "max pool")
    want = F.max_pool2d(_vals16(raw[0], compute, 64), 3, 2, 1)
    got = _vals16(raw[1], compute, 64)
    res.n = got.numel()
    if got.shape != want.shape or not torch.equal(got, want):
        res.errors.append("max pool not bit-exact")
    results.append(res)
    bl = resnet_oracle.blocks(specs)
    x_rec = 1
    for kb, (i1, i2, i3, idn) in enumerate(bl):
        x = _vals16(raw[x_rec], compute, specs[i1][0])
        t1 = _vals16(raw[1 + i1], compute, specs[i1][1])
        t2 = _vals16(raw[1 + i2], compute, specs[i2][1])
        r = x if idn is None else _vals16(raw[1 + idn], compute, specs[idn][1])
        steps = [(i1, x, 1, 0, None, True, "conv 1x1"), (i2, t1, specs[i2][3], 1, None, True, f"conv 3x3 /{specs[i2][3]}"),
                 (i3, t2, 1, 0, r, True, "conv 1x1 + residual")]
        if idn is not None:
            steps.append((idn, x, specs[idn][3], 0, None, False, "downsample"))
        for ci, a, stride, pad, rr, relu, name in steps:
            last = ci == i3 and kb + 1 == len(bl)
            res = LayerResult(1 + ci, "out (f32)" if last else name)
            st = resnet_oracle.conv16(a, params[ci], stride, pad, compute, res=rr, relu=relu, dtype=torch.float64, bound=True)
            a_conv = st.A if st.res is None else st.A - st.res.abs()
            g = gamma_mfma(st.K)
            lo, hi = interval(st, g * a_conv, "relu" if relu else "")
            if last:
                _check_f32(res, raw[1 + ci], st.y, lo, hi, a_conv, g / U)
            else:
                _check_stored16(res, raw[1 + ci], specs[ci][1], compute, [(st.y, lo, hi)])
            results.append(res)
        x_rec = 1 + i3
    return results


def resnet_context(m, compute, imgs):
    specs = m.conv_specs()
    return dict(specs=specs, params=synth.resnet_parameters(1234, specs), compute=compute,
                stem_inputs=_normalised(imgs, resnet_oracle.MEAN, resnet_oracle.STD, compute))


# ---------------------------------------------------------------------------------------------------- cases
def make_model(arch, block, compute, device, lib):
    from extractor_cases import CFG

    cfg = {"model": dict(CFG["model"], type=arch), "comparison": CFG["comparison"], "mi355x": {"extractor_dtype": compute}}
    return network.Model(cfg, block, device=device, library=lib)


def report(results, label="") -> str:
    """Per layer type: elements checked, ambiguous fraction, worst ratio to the bound (and, for float32 outputs, the worst
    observed error in units of A * 2^-24 against the gamma used)."""
    rows = {}
    for r in results:
        t = rows.setdefault(r.type, [0, 0, 0.0, 0.0, 0.0, 0, 0])
        t[0] += r.n; t[1] += r.ambiguous; t[2] = max(t[2], r.worst); t[3] = max(t[3], r.worst_acc)
        t[4] = max(t[4], r.gamma_units); t[5] += 1; t[6] += r.ambiguous_input
    lines = [f"per-layer parity {label}"]
    for k, (n, amb, worst, acc, units, cnt, ain) in rows.items():
        s = f"  {k:32s} layers {cnt:3d}  elements {n:9d}  ambiguous {amb / max(n, 1):7.3%}  worst/bound {worst:6.3f}"
        if ain:
            s += f"  ambiguous inputs {ain / max(n, 1):7.3%}"
        if units:
            s += f"  worst |k-y64|/(A 2^-24) {acc:7.3f} (gamma / 2^-24: {units:.1f})"
        lines.append(s)
    return "\n".join(lines)


def check_layers(arch, block, hw, n, compute, device, lib, keep=None):
    """Trace one batch, check every layer, the plain forward's bit-identity and the guard bands; returns the report."""
    m = make_model(arch, block, compute, device, lib)
    try:
        assert m.compute == compute
        imgs = _images(n, hw)
        tr = run_trace(m, lib, device, imgs)
        assert np.array_equal(tr.out.view(np.uint32), tr.plain.view(np.uint32)), "trace run's out differs from the plain forward"
        if m.effnet:
            ctx = effnet_context(m, compute, imgs)
            assert len(tr.raw) == len(ctx["ops"])
            results = check_effnet_trace(ctx, tr.raw)
            last = tr.raw[-1]
        else:
            ctx = resnet_context(m, compute, imgs)
            assert len(tr.raw) == 1 + len(ctx["specs"])
            results = check_resnet_trace(ctx, tr.raw)
            last = tr.raw[-1]
        assert np.array_equal(last.view(np.uint32), tr.out.view(np.uint32)), "the last record is not the output"
        text = report(results, f"{arch}[:{block}] {compute} {hw[0]}x{hw[1]} n={n}")
        print(text)
        bad = [f"layer {r.index} ({r.type}): {'; '.join(r.errors)}" for r in results if not r.ok]
        assert not bad, "\n".join(bad) + "\n" + text
        if keep is not None:
            keep.update(trace=tr, ctx=ctx, results=results, imgs=imgs)
        return text
    finally:
        m.close()
