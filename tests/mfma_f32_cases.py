"""Parity checks of the float32 matrix-core method ("mfma_f32": ncc_mfma.hip, SPR_NCC_MFMA_F32), shared by the CPU-emulation
tests (not gpu) and the MI355X tests (gpu).

The oracle is always the float64-statistics restatement of the reference on the UNROUNDED float32 inputs
(``oracle.similarity_matrix(..., precise=True)`` / ``oracle.normxcorr``), never the method under test.  Bounds: scores within
``TIGHT`` (5e-6, what the project's float32 kernels hold; the contract is ``TOL`` = 1e-4), per-channel maps within 20 TOL as
for the 16-bit matrix-core cases.  The scheme itself (both centred maps as two bfloat16 numbers, three of the four products)
restated in numpy with exact products stays within 1.1e-6 of the oracle on these generators at offsets 0, 100 and 1000, and
``hi * hi`` alone is 3.3e-4 away: the bound leaves the kernel's float32 accumulation a factor of four.  That holds for THESE
generators (several half-normal channels under templates of about 28 x 12 taps and more), not for the whole general instance:
under a handful of taps or a single channel the scheme itself is up to 6.1e-6 from the oracle (mfma_map_cases.py, which
therefore holds the kernel to TIGHT against the restated scheme and to TOL against the oracle).
"""

import numpy as np
import pytest

from oracle import ncc_oracle as oracle
from parity_cases import MFMA_GENERAL_SHAPES, TIGHT, TOL
from shoeprint_image_retrieval_amd import _lib, similarity, synth

SCALES = [1.02, 1.04, 1.08]  # the reference's run.toml


def _report(what, got, ref):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
    print(f"[mfma_f32] {what}: max |score - oracle| = {err:.3g}")
    return err


def _scores(sc, q, g, **kw):
    dev = sc.dev
    return dev.to_host(sc.scores_device(dev.to_device(np.stack(q)), dev.to_device(np.stack(g)), **kw))


def _equal_sets(seed, channels, nq, ng, offset=0.0):
    g = [np.maximum(synth.gallery_features(seed, i, channels, 32, 16), 0) + np.float32(offset) for i in range(ng)]
    q = [np.maximum(synth.query_features(seed, i % ng, i, channels, 32, 16), 0) + np.float32(offset) for i in range(nq)]
    return q, g


def _check_maps(sc, plan, q0, g0, channels, what):
    dev = sc.dev
    pq = sc.prepare_queries(plan, dev.to_device(q0[None]))
    pg = sc.prepare_gallery(plan, dev.to_device(g0[None]))
    maps = dev.to_host(sc.ncc_maps_device(plan, pq, pg))
    want = np.stack([oracle.normxcorr(q0[c, 2:-2, 2:-2], g0[c, 2:-2, 2:-2], precise=True) for c in range(channels)])
    assert maps.shape == want.shape
    _report(f"maps {what}", maps, want)
    np.testing.assert_allclose(maps, want, atol=20 * TOL, rtol=0, err_msg=f"maps {what}")


def check_resolution(make_scorer, channels=3):
    """"mfma_f32" is taken for float32 maps inside the bounds of the two instances and refused, with the bounds in the
    message, for 16-bit plans and for sizes beyond them; "auto" and "mfma" on float32 stay what they were."""
    sc = make_scorer("mfma_f32")
    assert sc.plan(channels, (32, 16), (32, 16)).method == _lib.NCC_MFMA_F32
    assert sc.plan(channels, (33, 16), (32, 16)).method == _lib.NCC_MFMA_F32
    assert sc.plan(channels, (34, 20), (32, 16)).method == _lib.NCC_MFMA_F32  # the largest template: 30 x 16
    for kw, q_hw, g_hw in (({"dtype": "bfloat16"}, (32, 16), (32, 16)), ({"dtype": np.float16}, (32, 16), (32, 16)),
                           ({}, (32, 16), (33, 16)),      # map beyond 28 x 12
                           ({}, (32, 16), (32, 17)),
                           ({}, (35, 16), (32, 16)),      # template beyond 30 x 16
                           ({}, (32, 21), (32, 16))):
        with pytest.raises(_lib.SprError, match="28x12.*30x16") as e:
            make_scorer("mfma_f32").plan(channels, q_hw, g_hw, **kw)
        assert e.value.code == _lib.SPR_ERR_UNSUPPORTED
    auto = make_scorer("auto")
    assert auto.plan(channels, (32, 16), (32, 16)).method == _lib.NCC_FFT
    with pytest.raises(Exception, match="matrix-core"):
        make_scorer("mfma").plan(channels, (32, 16), (32, 16), dtype=np.float32)


def check_equal_size(make_scorer, channels, nq, ng, tol=TIGHT):
    """The equal-size instance: scores, the running maximum over variants, the per-channel maps of one pair."""
    q, g = _equal_sets(43, channels, nq, ng)
    sc = make_scorer("mfma_f32")
    dev = sc.dev
    plan = sc.plan(channels, (32, 16), (32, 16))
    assert plan.method == _lib.NCC_MFMA_F32
    ref = oracle.similarity_matrix(q, g, precise=True)
    got = _scores(sc, q, g)
    err = _report(f"32x16 on 32x16, {channels} ch, {nq} x {ng}", got, ref)
    np.testing.assert_allclose(got, ref, atol=tol, rtol=0)
    scores = dev.to_device(np.full((nq, ng), 0.05, np.float32))
    sc.scores_device(dev.to_device(np.stack(q)), dev.to_device(np.stack(g)), scores=scores, accumulate_max=True)
    np.testing.assert_allclose(dev.to_host(scores), np.maximum(ref, 0.05), atol=tol, rtol=0)
    _check_maps(sc, plan, q[0], g[1 % ng], channels, "32x16 on 32x16")
    return err


def check_general_shapes(make_scorer, channels=3, nq=2, ng=3, tol=TIGHT, shapes=None):
    """Every pair of MFMA_GENERAL_SHAPES through the general instance, a dead channel on either side."""
    worst = 0.0
    for k, (qs, gs) in enumerate(shapes or MFMA_GENERAL_SHAPES):
        g = [np.maximum(synth.gallery_features(61 + k, i, channels, *gs), 0) for i in range(ng)]
        q = [np.maximum(synth.gallery_features(67 + k, 10 + i, channels, *qs), 0) for i in range(nq)]
        q[1][channels - 1] = 0.0  # a dead query channel
        g[ng - 1][0] = 0.0        # a dead gallery channel
        ref = oracle.similarity_matrix(q, g, precise=True)
        sc = make_scorer("mfma_f32")
        plan = sc.plan(channels, qs, gs)
        assert plan.method == _lib.NCC_MFMA_F32, (qs, gs)
        got = _scores(sc, q, g)
        worst = max(worst, _report(f"{qs} on {gs}, {channels} ch", got, ref))
        np.testing.assert_allclose(got, ref, atol=tol, rtol=0, err_msg=f"{qs} on {gs}")
        _check_maps(sc, plan, q[0], g[1], channels, f"{qs} on {gs}")
    return worst


def check_conditioning(make_scorer, channels=6, nq=3, ng=3, tol=TIGHT):
    """Maps riding on an offset (mean / sigma up to ~1000): centred in float32 before anything is rounded."""
    worst = 0.0
    for offset in (0.0, 3.0, 100.0, 1000.0):
        g = [np.maximum(synth.gallery_features(41, i, channels, 32, 16), 0) + np.float32(offset) for i in range(ng)]
        q = [np.maximum(synth.query_features(41, i, i, channels, 32, 16), 0) + np.float32(offset) for i in range(nq)]
        ref = oracle.similarity_matrix(q, g, precise=True)
        got = _scores(make_scorer("mfma_f32"), q, g)
        worst = max(worst, _report(f"offset {offset}, {channels} ch", got, ref))
        np.testing.assert_allclose(got, ref, atol=tol, rtol=0, err_msg=f"offset {offset}")
    return worst


def check_degenerate_channels(make_scorer, tol=TIGHT):
    """All-zero, constant and single-spike channels on either side: finite, equal to the oracle."""
    c, nq, ng = 6, 2, 2
    g = [np.maximum(synth.gallery_features(41, i, c, 32, 16), 0) for i in range(ng)]
    q = [np.maximum(synth.query_features(41, i, i, c, 32, 16), 0) for i in range(nq)]
    g[0][1] = 0.0
    q[1][2] = 0.0
    g[1][3] = 7.0
    q[0][4] = 0.5
    g[1][5] = 0.0
    g[1][5][9, 7] = 3.0
    q[1][0] = 0.0
    q[1][0][20, 3] = 2.0
    ref = oracle.similarity_matrix(q, g, precise=True)
    got = _scores(make_scorer("mfma_f32"), q, g)
    assert np.isfinite(got).all()
    _report("degenerate channels", got, ref)
    np.testing.assert_allclose(got, ref, atol=tol, rtol=0)


def check_lo_terms_needed(make_scorer, channels=6, nq=3, ng=3):
    """The same inputs rounded to bfloat16 - what hi * hi alone would see - score more than TOL away from the float32 oracle;
    the method stays within TIGHT of it: the lo products are issued."""
    q, g = _equal_sets(41, channels, nq, ng, offset=3.0)
    ref = oracle.similarity_matrix(q, g, precise=True)
    q16 = list(synth.from_bfloat16_bits(synth.bfloat16_bits(np.stack(q))))
    g16 = list(synth.from_bfloat16_bits(synth.bfloat16_bits(np.stack(g))))
    rounded = oracle.similarity_matrix(q16, g16, precise=True)
    gap = float(np.abs(rounded - ref).max())
    print(f"[mfma_f32] bfloat16-rounded inputs: max |score - float32 oracle| = {gap:.3g}")
    assert gap > TOL
    got = _scores(make_scorer("mfma_f32"), q, g)
    _report("same inputs, float32, mfma_f32", got, ref)
    np.testing.assert_allclose(got, ref, atol=TIGHT, rtol=0)


def check_opt_in_flag(make_scorer, channels=3):
    """NccScorer("auto", f32_matrix_cores=True): the new method where it covers a float32 plan, what "auto" gives elsewhere
    and for other storage types; flag off: as before."""
    on = make_scorer("auto", f32_matrix_cores=True)
    assert on.plan(channels, (32, 16), (32, 16)).method == _lib.NCC_MFMA_F32
    assert on.plan(channels, (34, 17), (32, 16)).method == _lib.NCC_MFMA_F32
    assert on.plan(channels, (64, 32), (64, 32)).method == _lib.NCC_FFT
    assert on.plan(channels, (32, 16), (32, 16), dtype="bfloat16").method == _lib.NCC_MFMA
    off = make_scorer("auto")
    assert off.plan(channels, (32, 16), (32, 16)).method == _lib.NCC_FFT
    assert off.plan(channels, (64, 32), (64, 32)).method == _lib.NCC_FFT
    # an explicit method is not overridden by the flag
    assert make_scorer("fft", f32_matrix_cores=True).plan(channels, (32, 16), (32, 16)).method == _lib.NCC_FFT
    q, g = _equal_sets(47, channels, 3, 4)
    ref = oracle.similarity_matrix(q, g, precise=True)
    np.testing.assert_allclose(_scores(on, q, g), ref, atol=TIGHT, rtol=0)
    # a ragged set mixes methods per shape
    rq = q[:2] + [np.maximum(synth.gallery_features(48, 7, channels, 64, 32), 0)]
    rg = g[:2] + [np.maximum(synth.gallery_features(48, 8, channels, 64, 32), 0)]
    np.testing.assert_allclose(on.score_matrix(rq, rg), oracle.similarity_matrix(rq, rg, precise=True), atol=TIGHT, rtol=0)
    assert {p.method for p in on._plans.values()} >= {_lib.NCC_MFMA_F32, _lib.NCC_FFT}


def check_config_flag(make_from_config, seed=5, channels=3, nq=3, ng=5):
    """[mi355x] f32_matrix_cores = true through compare_maps with the reference's scales on 32 x 16 maps (variants of
    32 x 16, 33 x 16 and 34 x 17: both instances): the oracle's ranks.  The seed is one whose oracle scores separate the true
    match from every other item of its row by more than 2 TIGHT - asserted, since only then do scores within TIGHT fix the rank."""
    from shoeprint_image_retrieval_amd.config import MI355X_DEFAULTS, normalise

    assert MI355X_DEFAULTS["f32_matrix_cores"] is False
    cfg = normalise({"comparison": {"n_processes": 1, "rotations": "", "scales": SCALES}, "mi355x": {"f32_matrix_cores": True}})
    q, g, m = synth.dataset(seed, nq, ng, channels, 32, 16)
    ref = oracle.similarity_matrix(q, g, scales=SCALES, precise=True)
    for i, mi in enumerate(m):
        others = np.delete(ref[i], mi)
        assert np.abs(others - ref[i, mi]).min() > 2 * TIGHT, (i, ref[i])
    sc = make_from_config(cfg)
    assert sc.f32_matrix_cores and sc is make_from_config(cfg)
    plain = make_from_config(normalise({"comparison": {"n_processes": 1, "rotations": "", "scales": SCALES}, "mi355x": {}}))
    assert plain is not sc and not plain.f32_matrix_cores  # the key is part of the scorer cache's key
    ranks = similarity.compare_maps(q, g, m, cfg, scorer=sc)
    np.testing.assert_array_equal(ranks, oracle.ranks_from_matrix(ref, m))
    methods = {p.q_hw: p.method for p in sc._plans.values()}
    assert methods == {(32, 16): _lib.NCC_MFMA_F32, (33, 16): _lib.NCC_MFMA_F32, (34, 17): _lib.NCC_MFMA_F32}, methods
    np.testing.assert_allclose(sc.score_matrix(q, g, scales=SCALES), ref, atol=TIGHT, rtol=0)


def check_table_prep(make_scorer, monkeypatch, channels=3, nq=2, ng=3):
    """SPR_MFMA_PREP=0 (galleries through the table kernel) against the default wave kernel: both within TIGHT of the oracle
    and of each other, on both instances."""
    for qs, gs in (((32, 16), (32, 16)), ((33, 16), (32, 16)), ((31, 15), (30, 14))):
        g = [np.maximum(synth.gallery_features(71, i, channels, *gs), 0) for i in range(ng)]
        q = [np.maximum(synth.gallery_features(73, 10 + i, channels, *qs), 0) for i in range(nq)]
        ref = oracle.similarity_matrix(q, g, precise=True)
        monkeypatch.setenv("SPR_MFMA_PREP", "1")
        wave = _scores(make_scorer("mfma_f32"), q, g)
        monkeypatch.setenv("SPR_MFMA_PREP", "0")
        table = _scores(make_scorer("mfma_f32"), q, g)
        monkeypatch.delenv("SPR_MFMA_PREP")
        np.testing.assert_allclose(wave, ref, atol=TIGHT, rtol=0, err_msg=f"wave {qs} on {gs}")
        np.testing.assert_allclose(table, ref, atol=TIGHT, rtol=0, err_msg=f"table {qs} on {gs}")
        np.testing.assert_allclose(table, wave, atol=TIGHT, rtol=0, err_msg=f"{qs} on {gs}")


def check_mean_term(make_scorer, monkeypatch, channels=6):
    """What the mean(t_hi + t_lo) * S1 term of the epilogue is worth (SPR_MFMA_F32_MEAN=0 drops it): printed; both within
    TIGHT."""
    out = {}
    for offset in (0.0, 1000.0):
        q, g = _equal_sets(41, channels, 3, 3, offset=offset)
        ref = oracle.similarity_matrix(q, g, precise=True)
        for keep in ("1", "0"):
            monkeypatch.setenv("SPR_MFMA_F32_MEAN", keep)
            got = _scores(make_scorer("mfma_f32"), q, g)
            out[offset, keep] = (_report(f"offset {offset}, mean term {keep}", got, ref), got)
        monkeypatch.delenv("SPR_MFMA_F32_MEAN")
        diff = float(np.abs(out[offset, "1"][1] - out[offset, "0"][1]).max())
        print(f"[mfma_f32] offset {offset}: the term moves a score by at most {diff:.3g}")
        assert out[offset, "1"][0] <= TIGHT and out[offset, "0"][0] <= TIGHT
    return out


def check_large_gallery(make_scorer, monkeypatch, channels, nq, ng, oracle_pairs=12):
    """A gallery of more than a thousand items at the full ResNet50-layer3 width, float32: against the FFT form on every
    pair, the oracle on sampled pairs, identical true-match ranks, unchanged when the launches are sliced."""
    mf, ff = make_scorer("mfma_f32"), make_scorer("fft")
    dev = mf.dev
    q, g = _equal_sets(47, channels, nq, ng)
    qd, gd = dev.to_device(np.stack(q)), dev.to_device(np.stack(g))
    got = dev.to_host(mf.scores_device(qd, gd))
    other = dev.to_host(ff.scores_device(qd, gd))
    _report(f"{nq} x {ng}, {channels} ch against the FFT form", got, other)
    np.testing.assert_allclose(got, other, atol=TIGHT, rtol=0)
    rng = np.random.default_rng(5)
    for qi, gi in zip(rng.integers(0, nq, oracle_pairs), rng.integers(0, ng, oracle_pairs)):
        want = float(oracle.get_similarity(q[qi], g[gi], precise=True))
        assert abs(got[qi, gi] - max(want, 0.0)) <= TIGHT, (qi, gi, got[qi, gi], want)
    match = dev.to_device((np.arange(nq) % ng).astype(np.int32))
    r_m = dev.to_host(mf.ranks_device(dev.to_device(got), match))
    r_f = dev.to_host(ff.ranks_device(dev.to_device(other), match))
    np.testing.assert_array_equal(r_m, r_f)
    monkeypatch.setenv("SPR_NCC_MAX_TILES", str(max(1, ng // 3)))  # three launches over the gallery
    np.testing.assert_array_equal(dev.to_host(mf.scores_device(qd, gd)), got)
    monkeypatch.delenv("SPR_NCC_MAX_TILES")
