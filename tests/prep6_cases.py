"""Checks of the pipelined corner-sum gallery preparation of the 192 x 96 six-wave FFT layout (csrc/ncc_prep6.hip), shared by
the CPU-emulation tests and the MI355X tests.

The same inputs are prepared by two plans, one made with SPR_PREP6=0 (prep_fft_kernel) and one with SPR_PREP6=1 (the new
kernel; the switch is read when a plan is made).  Spectra and dead flags must agree byte for byte.  The 1/sigma slices come
from float64 sums added in another order (below 1e-12 relative), so a value may move by one float32 rounding step at most,
and a slot that is zero in one is zero in the other.
"""

import numpy as np

from oracle import ncc_oracle as oracle

# the six-wave layout of the 192 x 96 grid (ncc_fft_cfg.h): complex values of a channel's spectrum, floats of its 1/sigma slice
SPEC_PER_CHAN = 2 * 12 * 384 + 192
INV_PER_CHAN = 6 * 384 * 4
GUARD = 4096  # poison bytes on each side of a prepared buffer
POISON = 0xA7
TIGHT = 5e-6  # the tolerance of the FFT parity cases (parity_cases.py)


def relu_maps(seed, n, channels, h, w, zero_channels=()):
    """Post-ReLU-like maps: about half the pixels zero, the others positive noise on a smooth ramp - no window of a quarter
    of the map or more is constant, so no variance sits at the zero threshold of inv_sigma_from_sums."""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(0.0, 1.0, h * w, dtype=np.float32).reshape(h, w)
    x = rng.standard_normal((n, channels, h, w)).astype(np.float32) + 0.5 * ramp
    x = np.maximum(x, 0.0).astype(np.float32)
    for c in zero_channels:
        x[:, c] = 0.0
    return np.ascontiguousarray(x)


def zero_channels_for(channels):
    """One all-zero channel in the middle and one as the last channel, where the channel count has room for them."""
    if channels >= 3:
        return (channels // 2, channels - 1)
    if channels == 2:
        return (1,)
    return ()


def two_plans(make_scorer, monkeypatch, channels, q_hw, g_hw, dtype):
    """(scorer, plan) made with SPR_PREP6=0 and with SPR_PREP6=1; both on the 192 x 96 six-wave grid."""
    out = []
    for flag in ("0", "1"):
        monkeypatch.setenv("SPR_PREP6", flag)
        sc = make_scorer()
        plan = sc.plan(channels, q_hw, g_hw, dtype=dtype)
        assert plan.fft_size == (192, 96), plan.fft_size
        per_item = channels * (SPEC_PER_CHAN * 8 + INV_PER_CHAN * 4) + channels
        assert plan.gallery_item_bytes == (per_item + 255) // 256 * 256, "not the six-wave layout"
        out.append((sc, plan))
    monkeypatch.delenv("SPR_PREP6")
    return out


def prepare_guarded(sc, plan, g_dev, n):
    """The prepared gallery as host bytes; the poison on both sides of the buffer must be untouched."""
    nbytes = plan.gallery_item_bytes * n
    buf = sc.dev.to_device(np.full(nbytes + 2 * GUARD, POISON, dtype=np.uint8))
    sc.prepare_gallery(plan, g_dev, out=sc.dev.narrow0(buf, GUARD, nbytes))
    sc.dev.synchronize()
    host = sc.dev.to_host(buf)
    assert (host[:GUARD] == POISON).all(), "bytes before the prepared buffer were written"
    assert (host[GUARD + nbytes:] == POISON).all(), "bytes after the prepared buffer were written"
    return host[GUARD: GUARD + nbytes]


def split_item(item_bytes, channels):
    spec_bytes = channels * SPEC_PER_CHAN * 8
    inv_bytes = channels * INV_PER_CHAN * 4
    spec = item_bytes[:spec_bytes]
    inv = item_bytes[spec_bytes: spec_bytes + inv_bytes].view(np.float32).reshape(channels, INV_PER_CHAN)
    flags = item_bytes[spec_bytes + inv_bytes: spec_bytes + inv_bytes + channels]
    return spec, inv, flags


def compare_prepared(old, new, n, channels, item_bytes, zero_channels=(), exact=False):
    """`exact`: the two plans ran the same kernel (fall-back plans): every byte the kernel writes is the same."""
    steps_max = 0.0
    for i in range(n):
        so, io, fo = split_item(old[i * item_bytes: (i + 1) * item_bytes], channels)
        sn, inn, fn = split_item(new[i * item_bytes: (i + 1) * item_bytes], channels)
        assert np.array_equal(so, sn), f"item {i}: spectra differ"
        assert np.array_equal(fo, fn), f"item {i}: dead flags differ"
        assert sorted(np.flatnonzero(fo).tolist()) == sorted(zero_channels), f"item {i}: dead flags {fo.tolist()}"
        assert np.isfinite(inn).all()
        if exact:
            assert np.array_equal(io.view(np.uint32), inn.view(np.uint32)), f"item {i}: 1/sigma bytes differ"
            continue
        assert np.array_equal(io == 0.0, inn == 0.0), f"item {i}: zero slots of 1/sigma differ"
        step = np.spacing(np.maximum(np.abs(io), np.abs(inn)).astype(np.float32))
        diff = np.abs(io.astype(np.float64) - inn.astype(np.float64))
        steps = float((diff / step)[io != 0.0].max()) if (io != 0.0).any() else 0.0
        steps_max = max(steps_max, steps)
        assert (diff <= step).all(), f"item {i}: 1/sigma moved by {steps:.2f} float32 steps"
        for c in zero_channels:
            assert not inn[c].any(), f"item {i}: 1/sigma of the all-zero channel {c} is not zero"
    return steps_max


def check_same_preparation(make_scorer, monkeypatch, n, channels, hw, storage):
    """Equal query and gallery size: the corner-window case the new kernel takes."""
    zc = zero_channels_for(channels)
    maps = relu_maps(1000 * channels + 10 * n + len(storage), n, channels, hw[0], hw[1], zc)
    (sc0, p0), (sc1, p1) = two_plans(make_scorer, monkeypatch, channels, hw, hw,
                                     _storage_dtype(make_scorer, storage))
    g0 = sc0.dev.astype_storage(sc0.dev.to_device(maps), storage)
    g1 = sc1.dev.astype_storage(sc1.dev.to_device(maps), storage)
    old = prepare_guarded(sc0, p0, g0, n)
    new = prepare_guarded(sc1, p1, g1, n)
    steps = compare_prepared(old, new, n, channels, p0.gallery_item_bytes, zc)
    print(f"{n} x {channels} x {hw} {storage}: 1/sigma within {steps:.2f} float32 steps")


def _storage_dtype(make_scorer, storage):
    dev = make_scorer().dev
    return dev.astype_storage(dev.to_device(np.zeros((1, 1, 1, 1), np.float32)), storage).dtype


def check_smaller_template_falls_back(make_scorer, monkeypatch, n=2, channels=3, q_hw=(120, 60), g_hw=(128, 64)):
    """A template smaller than the map has general windows: both plans run prep_fft_kernel, byte for byte."""
    maps = relu_maps(77, n, channels, g_hw[0], g_hw[1], zero_channels_for(channels))
    (sc0, p0), (sc1, p1) = two_plans(make_scorer, monkeypatch, channels, q_hw, g_hw, np.float32)
    old = prepare_guarded(sc0, p0, sc0.dev.to_device(maps), n)
    new = prepare_guarded(sc1, p1, sc1.dev.to_device(maps), n)
    compare_prepared(old, new, n, channels, p0.gallery_item_bytes, zero_channels_for(channels), exact=True)


def check_scores(make_scorer, monkeypatch, nq=4, ng=6, channels=3, hw=(128, 64)):
    """Scores from both preparations against the float64 oracle, at the tolerance of the FFT parity cases."""
    q = relu_maps(5, nq, channels, hw[0], hw[1])
    g = relu_maps(6, ng, channels, hw[0], hw[1], zero_channels_for(channels))
    g[:nq] += 0.5 * q  # some pairs correlate
    ref = oracle.similarity_matrix(list(q), list(g), precise=True)
    for sc, plan in two_plans(make_scorer, monkeypatch, channels, hw, hw, np.float32):
        dev = sc.dev
        pq = sc.prepare_queries(plan, dev.to_device(q))
        pg = sc.prepare_gallery(plan, dev.to_device(g))
        scores = dev.zeros((nq, ng), np.float32)
        sc.score_prepared(plan, pq, nq, pg, ng, scores, ng, 0)
        dev.synchronize()
        got = dev.to_host(scores)
        print(f"max |score - oracle| = {np.abs(got - ref).max():.2e}")
        np.testing.assert_allclose(got, ref, atol=TIGHT, rtol=0)
