"""Feature taps of the EfficientNet, ResNet50 and DenseNet_201 extractors (spr_*_forward_taps), shared by the emulated (not
gpu) and MI355X (gpu) tests.

The contract: the tap at slice end t of a plan truncated at block >= t is bit for bit the `out` of a plan of the same arch,
compute type and parameters truncated at t; in a 16-bit plan it is the unrounded float32 value whose round16 the tapped layer
stores for the next one.  Every comparison here is an equality of bit patterns (``view(np.uint32)``): both sides run the same
kernels on the same operands in the same order, so there is no rounding to allow for.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

import layer_cases as lc
from layer_cases import _images, make_model, run_guarded, run_trace
from oracle import resnet_oracle
from shoeprint_image_retrieval_amd import network

SPR_ERR_ARG = -1


@dataclass(frozen=True)
class Case:
    arch: str
    block: int        # the deep model
    taps: tuple       # every accepted tap of it, taken in one pass
    compute: str
    hw: tuple
    n: int
    rgb: bool = False

    @property
    def id(self):
        return f"{self.arch}-{self.block}-{self.compute}-{self.hw[0]}x{self.hw[1]}-n{self.n}" + ("-rgb" if self.rgb else "")


# 72 x 40: odd maps at every stride (36 x 20, 18 x 10, 9 x 5, 5 x 3); n = 3 of 96 x 80: no map's pixel count times 3 is a
# multiple of the 128-pixel tile of conv_gemm16_kernel (3 * 24 * 20 = 1440, 3 * 12 * 10 = 360, 3 * 6 * 5 = 90; the f32
# kernel's 64-pixel tile: the same), so the last tile of every tapped layer is ragged and tiles straddle two images.
CASES = [
    # conv_gemm_kernel (f32): 3x3 / 1 (stage 1), 1x1 / 1 (stages 2 - 5) block ends
    Case("EfficientNetV2_M", 6, (2, 3, 4, 5), "float32", (72, 40), 2),
    # conv_gemm16_kernel<KIND = bfloat16, BN = 64>: 3x3 / 1 and 1x1 / 1 block ends, SE-scaled operand (stages 4, 5)
    Case("EfficientNetV2_M", 6, (2, 3, 4, 5), "bfloat16", (96, 80), 3),
    # conv_gemm16_kernel<KIND = float16, BN = 64>, RGB input
    Case("EfficientNetV2_M", 6, (2, 3, 4, 5), "float16", (72, 40), 2, True),
    # conv_gemm_kernel: squeeze-excitation in every block, real widths 16 / 24 / 40 padded to 64
    Case("EfficientNet_B1", 5, (2, 3, 4), "float32", (96, 80), 3),
    # conv_gemm16_kernel<bfloat16, 64>: the same narrow padded stages (cout_real < 64 in the NCHW store)
    Case("EfficientNet_B1", 5, (2, 3, 4), "bfloat16", (72, 40), 2),
    # conv_gemm_kernel: 1x1 + residual + ReLU block ends (layer1: 256, layer2: 512 channels)
    Case("ResNet50", 7, (5, 6), "float32", (72, 40), 2),
    # conv_gemm16_kernel<bfloat16, 64> (and <bfloat16, 128> in the wide-tile test: SPR_GEMM16_BN=128)
    Case("ResNet50", 7, (5, 6), "bfloat16", (96, 80), 3),
    # conv_gemm16_kernel<float16, 64> (and <float16, 128> in the wide-tile test)
    Case("ResNet50", 7, (5, 6), "float16", (72, 40), 2),
    # dnet_out_kernel on the live block tensor: behind denseblock1 (5), transition1 (6), denseblock2 (7)
    Case("DenseNet_201", 8, (5, 6, 7), "float32", (72, 40), 2),
    # dnet_out16_kernel<bfloat16>
    Case("DenseNet_201", 8, (5, 6, 7), "bfloat16", (96, 80), 3),
]
# Emulated, a float32 EfficientNetV2_M pass costs about 10 ms per image pixel (five minutes for that case): the emulated suite
# reaches conv_gemm_kernel's tap store through EfficientNet_B1 and ResNet50 instead; the MI355X runs every case.
EMU_CASES = [c for c in CASES if not (c.arch == "EfficientNetV2_M" and c.compute == "float32")]
WIDE_CASES = [c for c in CASES if c.arch == "ResNet50" and c.compute != "float32"]  # run again with 128-channel tiles


def images(case: Case) -> np.ndarray:
    g = _images(case.n, case.hw)
    if not case.rgb:
        return g
    return np.ascontiguousarray(np.stack([g, np.roll(g, 5, axis=2), 255 - np.roll(g, 3, axis=1)], axis=-1))  # differing planes


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _call_args(m, dev, imgs):
    n, h, w = imgs.shape[:3]
    mean = (C.c_float * 3)(*m.mean)
    inv_std = (C.c_float * 3)(*[np.float32(1.0) / np.float32(s) for s in m.std])
    return n, h, w, 3 if imgs.ndim == 4 else 1, mean, inv_std


def run_taps(m, lib, dev, imgs, taps, expect=0):
    """One spr_*_forward_taps of `m` with `out`, the workspace (exactly spr_*_workspace_bytes) and every tap buffer inside one
    allocation, each between poisoned bands that must stay untouched (run_guarded); interiors start as all-ones bytes.  Returns
    (status, out, {tap: array}, the raw bytes of every buffer)."""
    n, h, w, ch, mean, inv_std = _call_args(m, dev, imgs)
    pre = m.family.prefix
    oshape = tuple(m.output_shape(h, w))
    # a refused tap has no shape: its buffer is one block-sized map
    tshapes = [tuple(m.tap_shape(t, h, w)) if t in m.accepted_taps() else oshape for t in taps]
    sizes = [4 * n * int(np.prod(oshape)), getattr(lib, f"spr_{pre}_workspace_bytes")(m.handle, n, h, w)]
    sizes += [4 * n * int(np.prod(s)) for s in tshapes]
    img_dev = dev.to_device(imgs)
    status = []

    def launch(sl):
        nt = len(taps)
        status.append(getattr(lib, f"spr_{pre}_forward_taps")(
            m.handle, dev.ptr(img_dev), n, h, w, ch, mean, inv_std, dev.ptr(m.packed), dev.ptr(sl[1]), dev.ptr(sl[0]), nt,
            (C.c_int32 * max(1, nt))(*taps), (C.c_void_p * max(1, nt))(*[dev.ptr(b) for b in sl[2:]]), dev.stream()))

    back = run_guarded(dev, sizes, launch)
    assert status[0] == expect, (status[0], lib.spr_last_error())
    out = back[0].view(np.float32).reshape((n,) + oshape).copy()
    got = {t: back[2 + j].view(np.float32).reshape((n,) + s).copy() for j, (t, s) in enumerate(zip(taps, tshapes))}
    return status[0], out, got, back


def trace(m, lib, dev, imgs) -> lc.Trace:
    """spr_*_forward_trace of any family, compute type and input form (layer_cases.run_trace where it applies: 16-bit
    EfficientNet / ResNet plans on grey images); a float32 plan's records are not read (raw = [])."""
    if imgs.ndim == 3 and not m.densenet and m.compute != "float32":
        return run_trace(m, lib, dev, imgs)
    n, h, w, ch, mean, inv_std = _call_args(m, dev, imgs)
    pre = m.family.prefix
    records, total = lc.trace_records(getattr(lib, f"spr_{pre}_trace_layout"), m.handle, n, h, w)
    oshape = tuple(m.output_shape(h, w))
    sizes = [4 * n * int(np.prod(oshape)), getattr(lib, f"spr_{pre}_workspace_bytes")(m.handle, n, h, w), total]
    img_dev = dev.to_device(imgs)
    fwd = getattr(lib, f"spr_{pre}_forward_trace")
    back = run_guarded(dev, sizes, lambda sl: lib.check(fwd(m.handle, dev.ptr(img_dev), n, h, w, ch, mean, inv_std,
                                                            dev.ptr(m.packed), dev.ptr(sl[1]), dev.ptr(sl[0]), dev.ptr(sl[2]),
                                                            dev.stream())))
    out = back[0].view(np.float32).reshape((n,) + oshape).copy()
    plain = np.asarray(dev.to_host(m.extract_device(img_dev, in_channels=ch)))
    return lc.Trace(records, lc.raw_records(back[2], records, n) if m.compute != "float32" else [], out, plain)


def truncated(deep, t: int, dev, lib):
    """`deep`'s backbone truncated at t, built with the prefix of the same parameter list."""
    fam = deep.family
    return network.Model(deep.config, t, device=dev, library=lib, parameters=fam.seeded(fam.layers(deep)))


def tapped_record(m, t: int) -> tuple[int, int]:
    """(index of the trace record the layer at slice end t stores for the next layer, its real channels)."""
    if m.effnet:
        ops = m.effnet_ops()
        i = max(k for k, o in enumerate(ops) if o["feature"] == t - 1)
        assert ops[i]["kind"] == 0 and ops[i]["block_end"]
        return i, ops[i]["cout"]
    if m.resnet:
        specs = m.conv_specs()
        bl = resnet_oracle.blocks(specs)
        layer = 0
        for kb, (_, _, i3, idn) in enumerate(bl):
            layer += idn is not None  # a layer opens with a downsample branch
            if 4 + layer == t and kb + 1 < len(bl) and bl[kb + 1][3] is not None:
                return 1 + i3, specs[i3][1]
        raise KeyError(t)
    ops = m.densenet_ops()  # the walk of densenet_trace_layout: stem, pooled stem, then per layer
    rec = 2
    for i, o in enumerate(ops[1:], 1):
        if o["kind"] == 1:
            rec += 1
        elif o["kind"] == 2 and o["c_off"] + 32 == o["ctot"]:
            rec += 1
            if o["feature"] == t - 1:
                return rec - 1, o["ctot"]
        elif o["kind"] == 3:
            rec += 2
            if o["feature"] == t - 1:
                return rec - 1, o["cout"]
    raise KeyError(t)


def check_case(case: Case, dev, lib):
    """Tests 1 - 3 of one case: every tap equals its truncated plan, the stored record is round16(tap), `out` equals the plain
    and the trace forward's, the guard bands hold (run_taps / trace), and image 1 alone gives what it gives inside the batch."""
    imgs = images(case)
    deep = make_model(case.arch, case.block, case.compute, dev, lib)
    try:
        assert deep.accepted_taps() == list(case.taps)
        _, out, got, _ = run_taps(deep, lib, dev, imgs, list(case.taps))
        # (the buffers started as NaN patterns: nothing of out and the taps is left unwritten)
        assert np.isfinite(out).all() and all(np.isfinite(v).all() for v in got.values())
        # ---- 1. tap == the truncated plan's out, bit for bit
        for t in case.taps:
            cut = truncated(deep, t, dev, lib)
            try:
                want = np.asarray(dev.to_host(cut.extract_device(dev.to_device(imgs), in_channels=3 if case.rgb else 1)))
            finally:
                cut.close()
            assert got[t].shape == want.shape, (t, got[t].shape, want.shape)
            diff = int(np.count_nonzero(bits(got[t]) != bits(want)))
            assert diff == 0, f"{case.id}: tap {t} differs from features[:{t}] in {diff} of {want.size} elements"
        # ---- 3. out with taps == the plain forward == the trace forward
        tr = trace(deep, lib, dev, imgs)
        assert np.array_equal(bits(out), bits(tr.plain)), "out with taps differs from the plain forward"
        assert np.array_equal(bits(out), bits(tr.out)), "out with taps differs from the trace forward"
        # ---- 2. a 16-bit plan stores round16(tap) for the next layer; padded channels as without taps (zeros)
        if case.compute != "float32":
            for t in case.taps:
                i, c_real = tapped_record(deep, t)
                rec = tr.raw[i]
                assert rec.dtype == np.uint16 and rec.shape[:3] == (case.n,) + got[t].shape[2:] and got[t].shape[1] == c_real
                want16 = lc.f32_to_bits(got[t].transpose(0, 2, 3, 1), case.compute)
                diff = int(np.count_nonzero(rec[..., :c_real] != want16))
                assert diff == 0, f"{case.id}: record {i} != round16(tap {t}) in {diff} of {want16.size} elements"
                if deep.effnet:
                    assert not rec[..., c_real:].any(), f"{case.id}: padded channels of record {i} are not zero"
        # ---- 3. the batch does not matter: image 1 alone
        if case.n >= 3:
            _, out1, got1, _ = run_taps(deep, lib, dev, np.ascontiguousarray(imgs[1:2]), list(case.taps))
            assert np.array_equal(bits(out1[0]), bits(out[1])), "out depends on the batch"
            for t in case.taps:
                assert np.array_equal(bits(got1[t][0]), bits(got[t][1])), f"tap {t} depends on the batch"
    finally:
        deep.close()


# ---------------------------------------------------------------------------------------------------- refusals
# (arch, block, refused tap lists): the stem alone / the ends inside the stem, a tap >= block, a tap named twice
REFUSALS = [
    ("EfficientNet_B1", 4, [[1], [0], [4], [5], [2, 2], [2, 3, 2]]),
    ("ResNet50", 6, [[1], [2], [3], [4], [6], [7], [5, 5]]),
    ("DenseNet_201", 7, [[1], [2], [3], [4], [7], [8], [5, 6, 5]]),
]


def check_refusals(arch, block, tap_lists, dev, lib):
    m = make_model(arch, block, "float32", dev, lib)
    try:
        imgs = _images(2, (40, 32))
        for taps in tap_lists:
            status, _, _, back = run_taps(m, lib, dev, imgs, taps, expect=SPR_ERR_ARG)
            assert all((raw == 0xFF).all() for raw in back), f"{arch} taps {taps}: a refused call wrote into a buffer"
            msg = lib.spr_last_error().decode()
            assert all(str(t) in msg for t in m.accepted_taps()), msg  # names the accepted values
            if taps != [block]:  # (the Python surface hands out the output for a tap equal to block, as for the VGGs)
                try:
                    m.extract_taps_device(dev.to_device(imgs), taps)
                except ValueError as e:
                    assert str(m.accepted_taps()) in str(e)
                else:
                    raise AssertionError(f"{arch} taps {taps}: extract_taps_device did not raise ValueError")
            bad = [t for t in taps if t not in m.accepted_taps()]
            if bad:
                c = C.c_int32()
                assert getattr(lib, f"spr_{m.family.prefix}_tap_shape")(m.handle, bad[0], 40, 32, C.byref(c), C.byref(c),
                                                                        C.byref(c)) == SPR_ERR_ARG
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------- routes
def check_feature_sets(arch, block, taps, dev, lib, sizes=((48, 40), (64, 32))):
    """get_multiple_feature_maps_device(taps=...) over a ragged image list of two sizes, in batches of two (one class has
    three images): one FeatureSet per tap whose items equal per-item extract_taps_device, and the set of a tap equal to
    block is today's single set - shapes, item order and bits."""
    from shoeprint_image_retrieval_amd import synth

    m = make_model(arch, block, "float32", dev, lib)
    try:
        m.batch_size = 2
        imgs = [synth.shoeprint_image(9, i, *sizes[k]) for i, k in enumerate((0, 1, 0, 0, 1))]
        sets = m.get_multiple_feature_maps_device(imgs, progress=False, taps=taps)
        assert len(sets) == len(taps) and all(len(s) == len(imgs) for s in sets)
        hosts = [s.to_host_list() for s in sets]
        for i, im in enumerate(imgs):
            per = m.extract_taps_device(m.clahe_device(dev.to_device(im[None])), taps)
            for j, t in enumerate(taps):
                want = np.asarray(dev.to_host(per[j]))[0]
                assert hosts[j][i].shape == want.shape and np.array_equal(bits(hosts[j][i]), bits(want)), (i, t)
        assert taps[-1] == block
        single = m.get_multiple_feature_maps_device(imgs, progress=False)
        assert len(sets[-1].classes) == len(single.classes)
        for (s1, i1, b1), (s2, i2, b2) in zip(sets[-1].classes, single.classes):
            assert s1 == s2 and np.array_equal(i1, i2)
            assert np.array_equal(bits(np.asarray(dev.to_host(b1))), bits(np.asarray(dev.to_host(b2))))
    finally:
        m.close()


def _pipeline_images(hw, n_gallery=5, n_queries=3):
    from shoeprint_image_retrieval_amd import synth

    gallery = np.stack([synth.shoeprint_image(23, g, *hw) for g in range(n_gallery)])
    rng = np.random.default_rng(5)
    queries = np.stack([np.clip(np.roll(gallery[q].astype(np.int32), (1, -2), axis=(0, 1)) + rng.normal(0, 20, hw), 0, 255)
                        .astype(np.uint8) for q in range(n_queries)])
    return queries, gallery


def check_pipeline(dev, lib, scorer, hw, compute, arch="EfficientNetV2_M", taps=(4, 6)):
    """MultiLayerPipeline(arch[:taps[1]], taps) - by default EfficientNetV2_M[:6] with taps (4, 6) - on Q = 3 x G = 5 uniform
    images (gallery batches of two, the last ragged): its fused matrix equals, bit for bit, multi_layer_scores_device fed with the features of the two separately
    truncated models; a float32 plan is also within the 1e-4 score contract of the oracle mean (effnet_oracle features of
    either truncation through ncc_oracle) with identical ranks."""
    from oracle import clahe_oracle, effnet_oracle, ncc_oracle
    from shoeprint_image_retrieval_amd import pipeline, synth

    m = make_model(arch, taps[1], compute, dev, lib)
    cut = truncated(m, taps[0], dev, lib)
    try:
        queries, gallery = _pipeline_images(hw)
        try:
            pipeline.MultiLayerPipeline(m, scorer)
        except ValueError as e:
            assert "taps" in str(e)
        else:
            raise AssertionError("a non-VGG model without taps was accepted")
        pipe = pipeline.MultiLayerPipeline(m, scorer, taps=taps, batch_size=2)
        qd, gd = dev.to_device(queries), dev.to_device(gallery)
        got = np.asarray(dev.to_host(pipe.scores_device(qd, gd)))
        layers = [(mod.extract_device(mod.clahe_device(qd)), mod.extract_device(mod.clahe_device(gd))) for mod in (cut, m)]
        want = np.asarray(dev.to_host(scorer.multi_layer_scores_device(layers)))
        assert got.shape == (3, 5) and np.array_equal(bits(got), bits(want)), np.abs(got - want).max()
        if compute == "float32":
            assert scorer.crop == ncc_oracle.CROP  # (the oracle crops by its own constant)
            params = synth.effnet_parameters(1234, m.effnet_ops())
            ref = np.zeros((3, 5), dtype=np.float64)
            for mod in (cut, m):
                ops = mod.effnet_ops()
                f = lambda im: effnet_oracle.get_feature_maps(clahe_oracle.clahe(im, 2.0, (8, 8)), ops, params[:len(ops)], m.mean,
                                                              m.std, m.bn_eps)
                ref += ncc_oracle.similarity_matrix([f(im) for im in queries], [f(im) for im in gallery],
                                                    precise=True).astype(np.float32)
            ref /= len(taps)
            err = float(np.abs(got - ref).max())
            print(f"fused score against the oracle mean: max |d| = {err:.3e}")
            assert err <= 1e-4, err
            ranks = pipe.ranks(qd, gd, [0, 1, 2])
            np.testing.assert_array_equal(ranks, ncc_oracle.ranks_from_matrix(ref.astype(np.float32), [0, 1, 2]))
    finally:
        cut.close()
        m.close()


def check_ragged_fusion(dev, lib, scorer, arch="EfficientNet_B1", block=4, taps=(3, 4), sizes=((96, 64), (112, 80)),
                        query_sizes=((64, 48), (80, 64))):
    """multi_layer_score_matrix_device on ragged sets of two sizes with rotations = [3] and scales = [1.04]: bit for bit the
    spr_scores_fuse chain over the per-layer score_matrix_device results."""
    from shoeprint_image_retrieval_amd import synth

    m = make_model(arch, block, "float32", dev, lib)
    try:
        gal = [synth.shoeprint_image(31, i, *sizes[k]) for i, k in enumerate((0, 1, 0, 1))]
        qry = [synth.shoeprint_image(31, i, *query_sizes[k]) for i, k in enumerate((1, 0, 0))]  # (every mark fits every print)
        q_sets = m.get_multiple_feature_maps_device(qry, progress=False, taps=taps)
        g_sets = m.get_multiple_feature_maps_device(gal, progress=False, taps=taps)
        kw = dict(rotations=[3], scales=[1.04])
        got = np.asarray(dev.to_host(scorer.multi_layer_score_matrix_device(list(zip(q_sets, g_sets)), **kw)))
        fused = dev.zeros((len(qry), len(gal)), np.float32)
        for k, (q, g) in enumerate(zip(q_sets, g_sets)):
            layer = scorer.score_matrix_device(q, g, **kw)
            lib.check(lib.spr_scores_fuse(dev.ptr(fused), dev.ptr(layer), len(qry) * len(gal), 0.0 if k == 0 else 1.0,
                                          1.0 / len(taps), dev.stream()))
        want = np.asarray(dev.to_host(fused))
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
        assert np.isfinite(got).all() and got.max() > 0
    finally:
        m.close()


def check_bad_fuse_blocks():
    """Each bad [mi355x].fuse_blocks form raises at load_config (normalise is what load_config applies to the parsed file)."""
    from shoeprint_image_retrieval_amd.config import MI355X_DEFAULTS, normalise

    def cfg(model="EfficientNetV2_M", **extra):
        return {"model": {"type": model}, "comparison": {}, "mi355x": extra}

    assert MI355X_DEFAULTS["fuse_blocks"] == [] and normalise(cfg())["mi355x"]["fuse_blocks"] == []
    assert normalise(cfg(fuse_blocks=[4, 2]))["mi355x"]["fuse_blocks"] == [4, 2]
    assert normalise(cfg("ResNet50", fuse_blocks=[5]))["mi355x"]["fuse_blocks"] == [5]
    assert normalise(cfg("VGG16", fuse_blocks=[16, 23]))["mi355x"]["fuse_blocks"] == [16, 23]
    bad = [cfg(fuse_blocks=4), cfg(fuse_blocks="4"), cfg(fuse_blocks=[4.0]), cfg(fuse_blocks=[True]), cfg(fuse_blocks=["4"]),
           cfg(fuse_blocks=[1]), cfg(fuse_blocks=[9]), cfg("ResNet50", fuse_blocks=[4]), cfg("ResNet50", fuse_blocks=[7]),
           cfg("DenseNet_201", fuse_blocks=[4]), cfg("VGG16", fuse_blocks=[15]),
           cfg(fuse_blocks=[4], shortlist=3), cfg(fuse_blocks=[4], gallery_cache="cache")]
    for c in bad:
        try:
            normalise(c)
        except ValueError as e:
            assert "fuse_blocks" in str(e)
        else:
            raise AssertionError(f"accepted: {c['model']['type']} {c['mi355x']}")
