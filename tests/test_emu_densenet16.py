"""The 16-bit DenseNet_201 extractor under emulation (tests/densenet16_cases.py): per-layer (teacher-forced) parity with
batches of differing images and tiles that straddle two images, guard bands around every buffer (interiors pre-filled with
all-ones bytes: block-tensor channels a layer must not read are NaN), sensitivity tests that prove the per-layer check catches
the subtle errors an end-to-end comparison cannot, batch invariance, the sanity distance to the float32 network, the surface."""

import functools

import numpy as np
import pytest
import torch

import densenet16_cases as dc
import layer_cases as lc
from emu_util import emu_library
from host_device import HostDevice


@pytest.mark.parametrize("block,hw,n,compute", [
    (5, (40, 36), 3, "bfloat16"),   # 270 pixels in block 1: three 128-pixel tiles, two of them across two images
    (6, (36, 40), 2, "float16"),    # the first transition; 9 x 10 -> 4 x 5: the pool drops the odd row
    (7, (48, 40), 2, "bfloat16"),   # block 2: reductions of 128 .. 480 channels, six of them with a half chunk
])
def test_emu_densenet16_per_layer_parity(block, hw, n, compute):
    dc.check_layers(block, hw, n, compute, HostDevice(), emu_library())


# ---------------------------------------------------------------------------------------------------- sensitivity
@functools.lru_cache(maxsize=None)
def _trace(compute):
    """A real emulator trace: DenseNet_201[:6] at 36 x 40, a print and a constant image - block 1 and the first transition."""
    keep = {}
    dc.check_layers(6, (36, 40), 2, compute, HostDevice(), emu_library(), keep=keep, sanity=False)
    return keep


def _record(y: torch.Tensor, old: np.ndarray, compute, c0=0, mode="rne"):
    """`old` with channels [c0, c0 + C) replaced by the float64 NCHW tensor y as stored."""
    rec = old.copy()
    v = y.to(torch.float32).numpy().transpose(0, 2, 3, 1)
    rec[..., c0: c0 + v.shape[3]] = lc.f32_to_bits(v, compute, mode)
    return rec


def _mutate(keep, what):
    """(key of the check that must fail, record index, new record) of one mutation, restated from the traced inputs."""
    ctx, raw = keep["ctx"], keep["trace"].raw
    recs, ops, compute = ctx["recs"], ctx["ops"], ctx["compute"]
    d1 = [r for r, rec in enumerate(recs) if rec["type"] == "dense 1x1"][3]  # the fourth dense layer: cin = 160, a half chunk
    blk = next(r for r, rec in enumerate(recs) if rec["type"] == "block")
    if what in ("pre-activated operand not re-rounded", "ReLU in front of the affine"):
        key = (d1, recs[d1]["op"])
        mode = "unrounded" if what.startswith("pre") else "relu first"
        return key, d1, _record(dc.expected(ctx, raw, key, mode)[0], raw[d1], compute)
    if what == "one 3x3 slice shifted by 32 channels":
        l = recs[blk]["layers"][2]
        c = ops[l["op2"]]["c_off"]
        rec = raw[blk].copy()
        rec[..., c + 32: c + 64], rec[..., c: c + 32] = raw[blk][..., c: c + 32], raw[blk][..., c + 32: c + 64]
        return (blk, l["op2"]), blk, rec
    if what == "average pool rounded toward zero":
        r = next(r for r, rec in enumerate(recs) if rec["type"] == "transition pool")
        key = (r, recs[r]["op"])
        return key, r, _record(dc.expected(ctx, raw, key)[0], raw[r], compute, mode="rtz")
    if what == "transition operand not activated":
        r = next(r for r, rec in enumerate(recs) if rec["type"] == "transition 1x1")
        o = ops[recs[r]["op"]]
        f = ctx["folded"][recs[r]["op"]]
        x = dc._vals(raw[recs[r]["block"]], compute, 0, o["cin"])
        a = dc.r16(dc.fma32(x.numpy(), f["s"][None, :, None, None], f["t"][None, :, None, None]), compute)  # no ReLU
        return (r, recs[r]["op"]), r, _record(dc.conv_step(torch.from_numpy(a), f, 0, False).y, raw[r], compute)
    raise KeyError(what)


MUTATIONS = ["pre-activated operand not re-rounded", "ReLU in front of the affine", "one 3x3 slice shifted by 32 channels",
             "average pool rounded toward zero", "transition operand not activated"]


@pytest.mark.parametrize("compute", ["bfloat16", "float16"])
@pytest.mark.parametrize("what", MUTATIONS)
def test_emu_densenet16_check_catches(what, compute):
    """Each mutation recomputes one record (or moves one slice) from the traced inputs under that mutation and splices it into
    the real trace: the check of THAT layer must fail, and nothing may fail that neither is it nor reads the mutated record."""
    keep = _trace(compute)
    ctx = keep["ctx"]
    key, r, rec = _mutate(keep, what)
    raw = list(keep["trace"].raw)
    assert not np.array_equal(raw[r], rec), "the mutation changed nothing"
    raw[r] = rec
    failed = [k for k in dc.keys_of(ctx) if not dc.check(ctx, raw, k).ok]
    assert key in failed, (what, key, failed)
    stray = [k for k in failed if k[0] != r and r not in dc.reads_of(ctx, k)]
    assert not stray, (what, key, stray)


# ---------------------------------------------------------------------------------------------------- buffers, surface
def test_emu_densenet16_batch_invariance():
    dc.check_batch_invariance(6, (40, 36), "bfloat16", HostDevice(), emu_library())


def test_emu_densenet16_surface():
    dc.check_surface(HostDevice(), emu_library())


def test_emu_densenet16_get_feature_maps():
    dc.check_get_feature_maps(5, (48, 32), "float16", HostDevice(), emu_library())


def test_fma32_resolves_hidden_ties():
    """fma32 against exact rational arithmetic, where the float64 sum lands on a float32 tie that the addend breaks."""
    from fractions import Fraction

    a = np.float32(1.0 + 2.0 ** -7)   # a * (1 + 2^-17) = 1 + 2^-7 + 2^-17 + 2^-24: halfway between two float32 values
    x = np.float32([a, a, a, 1.0, 0.5, -a])
    s = np.float32([1.0 + 2.0 ** -17] * 3 + [1.0, 1.0, 1.0 + 2.0 ** -17])
    t = np.float32([2.0 ** -60, -(2.0 ** -60), 0.0, 2.0 ** -30, 2.0 ** -30, 2.0 ** -60])
    got = dc.fma32(x, s, t)
    for i in range(len(x)):
        exact = Fraction(float(x[i])) * Fraction(float(s[i])) + Fraction(float(t[i]))
        mid = np.float32(float(exact))
        cands = [np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf))]
        # nearest; a true tie goes to the even mantissa
        best = min(cands, key=lambda c: (abs(Fraction(float(c)) - exact), int(np.float32(c).view(np.uint32)) & 1))
        assert got[i] == best, (i, got[i], best)
    assert got[0] != got[1]
