"""Per-layer (teacher-forced) parity of the 16-bit DenseNet_201 extractor, shared by the emulated (not gpu) and MI355X (gpu)
tests; the method, the element rules and the helpers are tests/layer_cases.py's.

oracle/densenet_oracle.py has no 16-bit mode, so the network is restated here in float64, written from the list of rounding
points in the header of csrc/densenet.hip (T = the compute type, round16 = to T, nearest even):

- weights: conv0 with norm0 folded, a dense 1x1 with its second BatchNorm folded (w * s, float32), the 3x3 and the transition
  1x1 as they are, each rounded once; biases (the folded BatchNorms' shifts) and the pre-activation scale / shift float32;
- stem: the rounded normalised image, round16(max(acc + b, 0)); max pool: exact, into channels [0, 64) of block 1's tensor;
- dense 1x1 / transition 1x1: operand round16(max(fmaf(x, s, t), 0)), float32 accumulation + bias, ReLU behind the dense one;
- dense 3x3: the stored intermediate, zero padded, round16(acc) into channels [c_off, c_off + 32) of the block tensor;
- transition pool: ((a + b) + c) + d in float32, times 0.25, one round16; output: float32 of the last tensor, norm5 as one fmaf.

Bounds, all derived (layer_cases has the argument for gamma):
- a convolution: e = gamma_mfma(K) * A with K = cin * taps (the reduction runs in steps of 32 over exactly cin channels) and
  A = |W| * |a| + |b|.  Its pre-activated operand carries NO slack: x * s is exact in float64 (11 + 24 bits), so the single
  rounding of fmaf is reproduced exactly (fma32 below resolves the ties a float64 sum could hide) and so is the round16 behind
  it - an operand that is not re-rounded, or activated in another order, differs in the ninth bit and shows;
- the average pool: three float32 additions of same-signed-or-not terms, each off by at most 2^-24 of its partial sum <= S =
  |a| + |b| + |c| + |d|; the scaling by 0.25 is exact: e = 3 * 2^-24 * S / 4 (times 1 + 2^-20 for the second-order terms);
- the max pool, the copy of a finished slice and the float32 output of a plan without norm5: bit-exact;
- norm5: one fmaf: e = 2^-24 * (|x * s| + |t|) >= half an ulp of the result.
Unwritten channels of a block-tensor record (behind the pool that starts it) are not compared; every slice behind the layer
that wrote it is, and the prefix of a complete block tensor must still be what its pool stored.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import layer_cases as lc
from layer_cases import U, LayerResult, gamma_mfma, interval
from oracle import densenet_oracle
from oracle.effnet_oracle import Step
from shoeprint_image_retrieval_amd import synth

BN_EPS = 1e-5
ARCH = "DenseNet_201"


# ---------------------------------------------------------------------------------------------------- arithmetic
def r16(a: np.ndarray, compute: str, mode: str = "rne") -> np.ndarray:
    """float32 values rounded to the compute type (as float32)."""
    return lc.bits_to_f32(lc.f32_to_bits(np.asarray(a, dtype=np.float32), compute, mode), compute)


def fma32(x: np.ndarray, s: np.ndarray, t: np.ndarray) -> np.ndarray:
    """fmaf(x, s, t) for 16-bit values x and float32 s, t, exactly: x * s is exact in float64; TwoSum gives the float64 sum and
    its error, and where the sum sits exactly between two float32 values the error decides the direction."""
    a = x.astype(np.float64) * s.astype(np.float64)
    b = np.broadcast_to(t.astype(np.float64), a.shape)
    sm = a + b
    bb = sm - a
    err = (a - (sm - bb)) + (b - bb)
    r = sm.astype(np.float32)
    d = sm - r.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        other = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = (d != 0) & (np.abs(other.astype(np.float64) - sm) == np.abs(d))
    return np.where(tie & (err * d > 0), other, r).astype(np.float32)


def _affine(gamma, beta, mu, var):
    """Eval-mode BatchNorm as x * s + t, float32, as the library's packer computes it."""
    s = gamma / np.sqrt(var + np.float32(BN_EPS))
    return s, beta - mu * s


def fold16(ops, params, compute: str) -> list[dict]:
    """Per layer what a 16-bit plan computes with: w (rounded, float32 values), b, pre-activation s / t."""
    out = []
    for op, p in zip(ops, params):
        p = [np.asarray(a, dtype=np.float32) for a in p]
        k = op["kind"]
        if k == 0:
            s, t = _affine(*p[1:5])
            out.append(dict(w=r16(p[0] * s[:, None, None, None], compute), b=t))
        elif k == 1:
            s1, t1 = _affine(*p[0:4])
            s2, t2 = _affine(*p[5:9])
            out.append(dict(s=s1, t=t1, w=r16(p[4] * s2[:, None, None, None], compute), b=t2))
        elif k == 2:
            out.append(dict(w=r16(p[0], compute), b=np.zeros(32, np.float32)))
        elif k == 3:
            s, t = _affine(*p[0:4])
            out.append(dict(s=s, t=t, w=r16(p[4], compute), b=np.zeros(op["cout"], np.float32)))
        else:
            s, t = _affine(*p[0:4])
            out.append(dict(s=s, t=t))
    return out


def preact(x: torch.Tensor, f: dict, compute: str, mode: str = "") -> torch.Tensor:
    """The operand of a dense / transition 1x1 from the stored tensor x (NCHW): round16(max(fmaf(x, s, t), 0)).  mode (the
    sensitivity mutations): "unrounded" leaves the last rounding out, "relu first" activates in front of the affine."""
    xn = x.numpy()
    s, t = f["s"][None, :, None, None], f["t"][None, :, None, None]
    if mode == "relu first":
        return torch.from_numpy(r16(fma32(np.maximum(xn, 0), s, t), compute))
    v = np.maximum(fma32(xn, s, t), np.float32(0))
    if mode == "unrounded":
        return torch.from_numpy(np.maximum(xn.astype(np.float64) * s + t, 0))
    return torch.from_numpy(r16(v, compute))


def conv_step(a: torch.Tensor, f: dict, pad: int, relu: bool, stride: int = 1) -> Step:
    """One convolution in float64 from its operand a: y = [relu](W * a + b), A = |W| * |a| + |b|, K = cin * taps."""
    w = torch.from_numpy(f["w"]).double()
    b = torch.from_numpy(f["b"]).double()
    a = a.double()
    with torch.no_grad():
        pre = F.conv2d(a, w, b, stride=stride, padding=pad)
        A = F.conv2d(a.abs(), w.abs(), b.abs(), stride=stride, padding=pad)
    return Step(F.relu(pre) if relu else pre, A, w.shape[1] * w.shape[2] * w.shape[3], pre, None)


def avgpool_step(x: torch.Tensor):
    """(y64, e) of the 2x2 average pool of the stored tensor x."""
    xd = x.double()
    y = F.avg_pool2d(xd, 2, 2)
    e = 3 * U * F.avg_pool2d(xd.abs(), 2, 2) * (1 + 2.0 ** -20)
    return y, e


def store(y: torch.Tensor, compute: str, mode: str = "rne") -> torch.Tensor:
    return torch.from_numpy(r16(y.to(torch.float32).numpy(), compute, mode))


# ---------------------------------------------------------------------------------------------------- records
def records_of(ops) -> list[dict]:
    """What spr_densenet_trace_layout lists, restated from the header: type, the op it belongs to, and the records it reads
    (start: the pool record that began the block tensor; block: the complete tensor of the dense block)."""
    recs = [dict(type="stem", op=0), dict(type="pool", op=0)]
    start, layers, tensor = 1, [], 1
    for i, op in enumerate(ops):
        if op["kind"] == 1:
            layers.append(dict(op1=i, d1=len(recs)))
            recs.append(dict(type="dense 1x1", op=i, start=start))
        elif op["kind"] == 2:
            layers[-1]["op2"] = i
            if op["c_off"] + 32 == op["ctot"]:
                blk = len(recs)
                for l in layers:
                    recs[l["d1"]]["block"] = blk
                recs.append(dict(type="block", op=i, start=start, layers=layers))
                layers, tensor = [], blk
        elif op["kind"] == 3:
            recs.append(dict(type="transition 1x1", op=i, block=tensor))
            recs.append(dict(type="transition pool", op=i, conv=len(recs) - 1))
            start = tensor = len(recs) - 1
    last = ops[-1]
    recs.append(dict(type="out (f32)", op=len(ops) - 1 if last["kind"] == 4 else None, tensor=tensor))
    return recs


@dataclass
class Trace:
    records: list
    raw: list
    out: np.ndarray
    plain: np.ndarray


def run_trace(m, lib, dev, imgs: np.ndarray) -> Trace:
    """layer_cases.run_trace for spr_densenet_forward_trace: `out`, the workspace (exactly spr_densenet_workspace_bytes) and
    the trace inside one allocation, each between 4096-byte poisoned bands that must stay untouched, interiors all-ones bytes."""
    n, h, w = imgs.shape
    total = C.c_size_t(0)
    cnt = lib.spr_densenet_trace_layout(m.handle, n, h, w, None, C.byref(total))
    assert cnt > 0, cnt
    rec = (C.c_int64 * (6 * cnt))()
    assert lib.spr_densenet_trace_layout(m.handle, n, h, w, rec, C.byref(total)) == cnt
    records = [tuple(int(v) for v in rec[6 * i: 6 * i + 6]) for i in range(cnt)]
    c, oh, ow = m.output_shape(h, w)
    sizes = [n * c * oh * ow * 4, lib.spr_densenet_workspace_bytes(m.handle, n, h, w), total.value]
    starts, at = [], lc.GUARD
    for sz in sizes:
        starts.append(at)
        at = (at + sz + lc.GUARD + 255) // 256 * 256
    host = np.random.default_rng(99).integers(0, 256, size=at + 256, dtype=np.uint8)
    buf = dev.to_device(host)
    shift = (-dev.ptr(buf)) % 256
    sl = [buf[shift + s0: shift + s0 + sz] for s0, sz in zip(starts, sizes)]
    for b in sl:
        b[:] = 0xFF
    img_dev = dev.to_device(imgs)
    mean = (C.c_float * 3)(*m.mean)
    inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in m.std])
    lib.check(lib.spr_densenet_forward_trace(m.handle, dev.ptr(img_dev), n, h, w, 1, mean, inv_std, dev.ptr(m.packed),
                                             dev.ptr(sl[1]), dev.ptr(sl[0]), dev.ptr(sl[2]), dev.stream()))
    dev.synchronize()
    back = np.asarray(dev.to_host(buf))
    bands = np.ones(len(host), bool)
    for s0, sz in zip(starts, sizes):
        bands[shift + s0: shift + s0 + sz] = False
    bad = np.nonzero(bands & (back != host))[0]
    assert bad.size == 0, f"{bad.size} guard-band bytes overwritten, first at {bad[:8].tolist()} (buffers at {starts}, +{shift})"
    out = back[shift + starts[0]: shift + starts[0] + sizes[0]].view(np.float32).reshape(n, c, oh, ow).copy()
    tr = back[shift + starts[2]: shift + starts[2] + sizes[2]]
    raw = []
    for off, rh, rw, rc, dt, nchw in records:
        if dt == 0:
            assert nchw == 1
            raw.append(tr[off: off + 4 * n * rh * rw * rc].view(np.float32).reshape(n, rc, rh, rw).copy())
        else:
            raw.append(tr[off: off + 2 * n * rh * rw * rc].view(np.uint16).reshape(n, rh, rw, rc).copy())
    plain = np.asarray(dev.to_host(m.extract_device(img_dev)))
    return Trace(records, raw, out, plain)


# ---------------------------------------------------------------------------------------------------- the checks
def context(m, compute: str, imgs: np.ndarray) -> dict:
    ops = m.densenet_ops()
    params = synth.densenet_parameters(1234, ops)
    return dict(ops=ops, params=params, folded=fold16(ops, params, compute), compute=compute, recs=records_of(ops),
                stem_inputs=lc._normalised(imgs, m.mean, m.std, compute))


def _vals(raw: np.ndarray, compute: str, c0: int, c1: int) -> torch.Tensor:
    """Channels [c0, c1) of a uint16 NHWC record as a float32 NCHW tensor."""
    v = lc.bits_to_f32(raw[..., c0:c1], compute)
    return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))


def keys_of(ctx) -> list[tuple]:
    """Every check of a trace as (record, op): one per record, and one per 3x3 layer plus ("prefix") for a block record."""
    keys = []
    for r, rec in enumerate(ctx["recs"]):
        if rec["type"] == "block":
            keys.append((r, "prefix"))
            keys += [(r, l["op2"]) for l in rec["layers"]]
        else:
            keys.append((r, rec["op"]))
    return keys


def reads_of(ctx, key) -> set:
    """The records a check reads besides its own."""
    r, op = key
    rec = ctx["recs"][r]
    t = rec["type"]
    if t == "stem":
        return set()
    if t == "pool":
        return {0}
    if t == "dense 1x1":
        return {rec["block"]}
    if t == "block":
        return {rec["start"]} if op == "prefix" else {next(l["d1"] for l in rec["layers"] if l["op2"] == op)}
    if t == "transition 1x1":
        return {rec["block"]}
    if t == "transition pool":
        return {rec["conv"]}
    return {rec["tensor"]}


def expected(ctx, raw, key, mode: str = ""):
    """The float64 restatement of one check from its traced inputs: (y, lo, hi, A, gamma) - for the stem a list of two."""
    ops, fd, compute = ctx["ops"], ctx["folded"], ctx["compute"]
    r, op = key
    rec = ctx["recs"][r]
    t = rec["type"]
    if t == "stem":
        out = []
        for x in ctx["stem_inputs"]:
            st = conv_step(x, fd[0], 3, True, stride=2)
            out.append((st.y, *interval(st, gamma_mfma(160) * st.A, "relu")))
        return out
    if t in ("dense 1x1", "transition 1x1"):
        o = ops[rec["op"]]
        a = preact(_vals(raw[rec["block"]], compute, 0, o["cin"]), fd[rec["op"]], compute, mode)
        st = conv_step(a, fd[rec["op"]], 0, t == "dense 1x1")
        g = gamma_mfma(st.K)
        return (st.y, *interval(st, g * st.A, "relu" if t == "dense 1x1" else ""), st.A, g)
    if t == "block":
        d1 = next(l["d1"] for l in rec["layers"] if l["op2"] == op)
        st = conv_step(_vals(raw[d1], compute, 0, 128), fd[op], 1, False)
        g = gamma_mfma(st.K)
        return (st.y, *interval(st, g * st.A, ""), st.A, g)
    if t == "transition pool":
        y, e = avgpool_step(_vals(raw[rec["conv"]], compute, 0, ops[rec["op"]]["cout"]))
        return (y, y - e, y + e, None, 0.0)
    raise KeyError(key)


def check(ctx, raw, key) -> LayerResult:
    ops, fd, compute = ctx["ops"], ctx["folded"], ctx["compute"]
    r, op = key
    rec = ctx["recs"][r]
    t = rec["type"]
    res = LayerResult(r, t if op != "prefix" else "block prefix (copy)")
    if t == "stem":
        lc._check_stored16(res, raw[0], 64, compute, expected(ctx, raw, key))
    elif t == "pool":
        want = F.max_pool2d(_vals(raw[0], compute, 0, 64), 3, 2, 1)
        got = _vals(raw[1], compute, 0, 64)
        res.n = got.numel()
        if got.shape != want.shape or not torch.equal(got, want):
            res.errors.append("max pool not bit-exact")
    elif t in ("dense 1x1", "transition 1x1", "transition pool"):
        y, lo, hi, _, _ = expected(ctx, raw, key)
        lc._check_stored16(res, raw[r], y.shape[1], compute, [(y, lo, hi)])
    elif op == "prefix":
        c0 = ops[rec["layers"][0]["op1"]]["cin"]
        res.n = raw[r][..., :c0].size
        if not np.array_equal(raw[r][..., :c0], raw[rec["start"]][..., :c0]):
            res.errors.append(f"channels [0, {c0}) of the complete block tensor differ from what its pool stored")
    elif t == "block":
        res.type = "dense 3x3 (slice of the block tensor)"
        y, lo, hi, _, _ = expected(ctx, raw, key)
        c_off = ops[op]["c_off"]
        lc._check_stored16(res, raw[r][..., c_off: c_off + 32], 32, compute, [(y, lo, hi)])
    else:  # the float32 NCHW output
        src = rec["tensor"]
        c = raw[r].shape[1]
        x = _vals(raw[src], compute, 0, c)
        if rec["op"] is None:
            res.n = x.numel()
            if not np.array_equal(x.numpy().view(np.uint32), raw[r].view(np.uint32)):
                res.errors.append("the output is not the last tensor's stored values")
        else:
            f = fd[rec["op"]]
            s = torch.from_numpy(f["s"]).double()[None, :, None, None]
            tt = torch.from_numpy(f["t"]).double()[None, :, None, None]
            y = x.double() * s + tt
            e = U * ((x.double() * s).abs() + tt.abs()) + 1e-45
            lc._check_f32(res, raw[r], y, y - e, y + e)
    return res


def check_trace(ctx, raw, keys=None) -> list:
    return [check(ctx, raw, k) for k in (keys_of(ctx) if keys is None else keys)]


# ---------------------------------------------------------------------------------------------------- end to end
def restate16(img: np.ndarray, ops, params, mean, std, compute: str) -> np.ndarray:
    """The whole 16-bit network in float64 with the build's rounding points, on its own stored values (uint8 [H, W], already
    CLAHE'd, -> float32 [C, h, w]).  Not the parity claim: the sanity check against the float32 oracle."""
    fd = fold16(ops, params, compute)
    x = lc._normalised(img[None], mean, std, compute)[1]
    x = F.max_pool2d(store(conv_step(x, fd[0], 3, True, stride=2).y, compute), 3, 2, 1)
    for op, f in zip(ops[1:], fd[1:]):
        if op["kind"] == 1:
            mid = store(conv_step(preact(x[:, : op["cin"]], f, compute), f, 0, True).y, compute)
        elif op["kind"] == 2:
            x = torch.cat([x, store(conv_step(mid, f, 1, False).y, compute)], dim=1)
        elif op["kind"] == 3:
            x = store(avgpool_step(store(conv_step(preact(x, f, compute), f, 0, False).y, compute))[0], compute)
        else:
            x = (x.double() * torch.from_numpy(f["s"]).double()[None, :, None, None]
                 + torch.from_numpy(f["t"]).double()[None, :, None, None]).to(torch.float32)
    return x.to(torch.float32).numpy()[0]


def sanity_against_f32(m, compute: str, imgs: np.ndarray, got: np.ndarray) -> str:
    """rms distance of the kernel's output to the float32 oracle, held to twice the restatement's own distance d (computed
    here, on the CPU, from the restatement alone)."""
    ops = m.densenet_ops()
    params = synth.densenet_parameters(1234, ops)
    lines = []
    for i, img in enumerate(imgs):
        ref = densenet_oracle.get_feature_maps(img, ops, params, m.mean, m.std).astype(np.float64)
        d = float(np.sqrt(np.mean((restate16(img, ops, params, m.mean, m.std, compute).astype(np.float64) - ref) ** 2)))
        k = float(np.sqrt(np.mean((got[i].astype(np.float64) - ref) ** 2)))
        rel = float(np.abs(got[i] - ref).max() / max(np.abs(ref).max(), 1e-30))
        lines.append(f"  image {i}: rms |kernel - f32 oracle| {k:.3e} against 2 d = {2 * d:.3e}; largest deviation relative to "
                     f"max |f32| {rel:.3e}")
        assert k <= 2 * d, lines[-1]
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------- cases
def check_layers(block, hw, n, compute, device, lib, keep=None, sanity=True) -> str:
    """Trace one batch; check every layer, the plain forward's bit-identity, the guard bands and (sanity) the distance to the
    float32 network; returns the report."""
    m = lc.make_model(ARCH, block, compute, device, lib)
    try:
        assert m.compute == compute
        assert lib.spr_densenet_plan_compute(m.handle) == {"float16": 1, "bfloat16": 2}[compute]
        imgs = lc._images(n, hw)
        tr = run_trace(m, lib, device, imgs)
        assert np.array_equal(tr.out.view(np.uint32), tr.plain.view(np.uint32)), "trace run's out differs from the plain forward"
        ctx = context(m, compute, imgs)
        assert len(tr.raw) == len(ctx["recs"]), (len(tr.raw), len(ctx["recs"]))
        assert np.array_equal(tr.raw[-1].view(np.uint32), tr.out.view(np.uint32)), "the last record is not the output"
        results = check_trace(ctx, tr.raw)
        text = lc.report(results, f"{ARCH}[:{block}] {compute} {hw[0]}x{hw[1]} n={n}")
        print(text)
        bad = [f"record {r.index} ({r.type}): {'; '.join(r.errors)}" for r in results if not r.ok]
        assert not bad, "\n".join(bad[:20]) + "\n" + text
        if sanity:
            s = sanity_against_f32(m, compute, imgs, tr.out)
            print(s)
            text += "\n" + s
        if keep is not None:
            keep.update(trace=tr, ctx=ctx, results=results, imgs=imgs)
        return text
    finally:
        m.close()


def check_batch_invariance(block, hw, compute, device, lib):
    """Image i's features in a batch of 3 equal its features extracted alone, bit for bit."""
    m = lc.make_model(ARCH, block, compute, device, lib)
    try:
        imgs = lc._images(3, hw)
        batch = np.asarray(device.to_host(m.extract_device(device.to_device(imgs))))
        assert np.all(np.isfinite(batch))
        for i in range(3):
            alone = np.asarray(device.to_host(m.extract_device(device.to_device(imgs[i: i + 1]))))
            assert np.array_equal(alone[0].view(np.uint32), batch[i].view(np.uint32)), f"image {i} differs from its batch of one"
    finally:
        m.close()


def check_surface(device, lib):
    """The plan's compute codes, the refusals, a float32 plan's trace layout, and _ex(block, 0) against spr_densenet_plan_create."""
    from shoeprint_image_retrieval_amd import network

    for compute, code in (("bfloat16", 2), ("float16", 1)):
        m = lc.make_model(ARCH, 9, compute, device, lib)
        try:
            assert lib.spr_densenet_plan_compute(m.handle) == code
        finally:
            m.close()
    try:
        lc.make_model(ARCH, 4, "bfloat16", device, lib)
    except NotImplementedError:
        pass
    else:
        raise AssertionError("block 4 with bfloat16 did not raise NotImplementedError")
    handle = C.c_void_p()
    assert lib.spr_densenet_plan_create_ex(4, 2, C.byref(handle)) == -3 and not handle.value
    for block in (3, 6):
        a, b = C.c_void_p(), C.c_void_p()
        lib.check(lib.spr_densenet_plan_create(block, C.byref(a)))
        lib.check(lib.spr_densenet_plan_create_ex(block, 0, C.byref(b)))
        try:
            assert lib.spr_densenet_plan_compute(a) == 0 and lib.spr_densenet_plan_compute(b) == 0
            assert network.densenet_plan_ops(lib, a) == network.densenet_plan_ops(lib, b)
            assert lib.spr_densenet_packed_bytes(a) == lib.spr_densenet_packed_bytes(b)
            assert lib.spr_densenet_workspace_bytes(a, 2, 40, 36) == lib.spr_densenet_workspace_bytes(b, 2, 40, 36)
            # a float32 plan traces: SPR_OK, the same records from both constructors, and (through a Model of that block) the
            # expected count, every record's (h, w, c, dtype, nchw) and total_bytes = the sum of the 256-aligned records
            import f32_layer_cases as fc

            assert lc.trace_records(lib.spr_densenet_trace_layout, a, 1, 40, 40) == lc.trace_records(lib.spr_densenet_trace_layout, b, 1, 40, 40)
            m = lc.make_model(ARCH, block, "float32", device, lib)
            try:
                assert fc.check_layout(m, lib, 1, (40, 40)) == lc.trace_records(lib.spr_densenet_trace_layout, b, 1, 40, 40)[0]
            finally:
                m.close()
            total = C.c_size_t(0)
            assert lib.spr_densenet_trace_layout(b, 1, 16, 40, None, C.byref(total)) == -1  # SPR_ERR_ARG: at least 32 x 32
            assert lib.spr_densenet_forward_trace(b, None, 1, 40, 40, 1, (C.c_float * 3)(), (C.c_float * 3)(), None, None, None, None,
                                                  device.stream()) == -1              # a null trace
        finally:
            lib.spr_densenet_plan_destroy(a)
            lib.spr_densenet_plan_destroy(b)
    # the same output from both constructors: Model goes through _ex(block, 0)
    m = lc.make_model(ARCH, 6, "float32", device, lib)
    try:
        imgs = lc._images(2, (40, 36))
        got = np.asarray(device.to_host(m.extract_device(device.to_device(imgs))))
        h = C.c_void_p()
        lib.check(lib.spr_densenet_plan_create(6, C.byref(h)))
        try:
            c, oh, ow = m.output_shape(40, 36)
            out = device.empty((2, c, oh, ow), np.float32)
            ws = device.empty_bytes(lib.spr_densenet_workspace_bytes(h, 2, 40, 36))
            mean = (C.c_float * 3)(*m.mean)
            inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in m.std])
            img_dev = device.to_device(imgs)
            lib.check(lib.spr_densenet_forward(h, device.ptr(img_dev), 2, 40, 36, 1, mean, inv_std, device.ptr(m.packed),
                                               device.ptr(ws), device.ptr(out), device.stream()))
            device.synchronize()
            assert np.array_equal(np.asarray(device.to_host(out)).view(np.uint32), got.view(np.uint32))
        finally:
            lib.spr_densenet_plan_destroy(h)
    finally:
        m.close()


def check_get_feature_maps(block, hw, compute, device, lib) -> str:
    """Model.get_feature_maps (CLAHE included) of one print: bit-identical to the traced forward of the CLAHE'd image (the
    CPU oracle's CLAHE), whose every layer - the output included - passes the per-layer check against the restatement."""
    from oracle import clahe_oracle

    m = lc.make_model(ARCH, block, compute, device, lib)
    try:
        img = synth.shoeprint_image(7, 0, *hw)
        feats = m.get_feature_maps(img)
        pre = clahe_oracle.clahe(img, m.clahe_clip_limit, m.clahe_tile_grid_size)
        tr = run_trace(m, lib, device, pre[None])
        ctx = context(m, compute, pre[None])
        results = check_trace(ctx, tr.raw)
        bad = [f"record {r.index} ({r.type}): {'; '.join(r.errors)}" for r in results if not r.ok]
        assert not bad, "\n".join(bad[:20])
        assert feats.dtype == np.float32 and feats.shape == tr.out.shape[1:]
        assert np.array_equal(feats.view(np.uint32), tr.out[0].view(np.uint32)), "get_feature_maps differs from the traced forward"
        return lc.report(results, f"get_feature_maps {ARCH}[:{block}] {compute}")
    finally:
        m.close()
