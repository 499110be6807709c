"""Shortlist retrieval checks shared by the CPU-emulation tests (not gpu) and the MI355X tests (gpu): spr_topk_rows,
spr_maps_peak and their host mirror (NccScorer.topk_device / locate, similarity.retrieve).

The two kernels are exact by contract - a total order on (score, index), a fixed float64 summation order - so they are
compared bit for bit with NumPy.  Scores of located pairs are compared with the float64 oracle within parity_cases.TIGHT;
peak positions wherever the oracle's own peak leads its runner-up pixel by more than POSITION_LEAD = 1e-4 = 20 x TIGHT
(both sides then agree on the pixel unless one of them is off by more than the score tolerance allows).
"""

import functools
import os

import numpy as np
import pytest

from oracle import ncc_oracle as oracle
from parity_cases import GOLDEN, TIGHT
from shoeprint_image_retrieval_amd import _lib, similarity, synth

POSITION_LEAD = 1e-4
TOPK_SIZES = [(1, 1), (3, 7), (5, 300), (2, 1500), (2, 70000)]
TOPK_KS = [1, 5, 64, 256]
PEAK_SHAPES = [(1, 1, 1, 1), (3, 5, 16, 10), (2, 1024, 28, 12), (1, 2, 124, 60)]
PLANTED_CASES = [(7, 4, 6, 5, 20, 14), (9, 3, 5, 6, 32, 16), (12, 2, 3, 2, 128, 64)]  # synth.dataset(seed, nq, ng, c, h, w)


def _cfg(rot=None, sc=None):
    return {"comparison": {"n_processes": 1, "rotations": rot, "scales": sc}}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ spr_topk_rows
def expected_topk(s, k, index=None, col0=0):
    """NumPy statement of the order: score descending, index descending among equal scores (np.lexsort((-idx, -s))),
    truncated to k and padded with (-1, 0).  ``index`` [Q,G]: item index per column, negative = no item."""
    nq, ng = s.shape
    out_s = np.zeros((nq, k), np.float32)
    out_i = np.full((nq, k), -1, np.int32)
    for q in range(nq):
        ids = np.arange(ng, dtype=np.int64) + col0 if index is None else index[q].astype(np.int64)
        cols = np.nonzero(ids >= 0)[0]
        order = cols[np.lexsort((-ids[cols], -s[q, cols]))][:k]
        out_s[q, :len(order)] = s[q, order]
        out_i[q, :len(order)] = ids[order]
    return out_s, out_i


@functools.lru_cache(maxsize=None)
def topk_matrix(nq, ng):
    """Random scores of both signs with plenty of exact ties (as check_rank_kernel plants them), zeros of both signs and a
    repeated maximum.  Shared by the tests of one size: treat as read-only."""
    s = np.random.default_rng(1000 * nq + ng).standard_normal((nq, ng)).astype(np.float32)
    s[:, ::3] = s[:, :1]
    if ng >= 7:
        s[:, 1], s[:, 4], s[:, 5] = -0.0, 0.0, -0.0
        s[:, 2] = s[:, ng - 1] = 7.5
    s.setflags(write=False)
    return s


def _topk(scorer, s, k, **kw):
    dev = scorer.dev
    if kw.get("col_index") is not None:
        kw["col_index"] = dev.to_device(np.ascontiguousarray(kw["col_index"], dtype=np.int32))
    top_s, top_i = scorer.topk_device(dev.to_device(np.array(s, dtype=np.float32, order="C")), k, **kw)
    top_s, top_i = dev.to_host(top_s), dev.to_host(top_i)
    assert top_s.dtype == np.float32 and top_i.dtype == np.int32 and top_s.shape == top_i.shape == (s.shape[0], k)
    return top_s, top_i


def check_topk_order(scorer, size, k):
    nq, ng = size
    s = topk_matrix(nq, ng)
    got_s, got_i = _topk(scorer, s, k)
    want_s, want_i = expected_topk(s, k)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
    # the item at position p is the item the ranker ranks p
    for p in range(min(k, ng)):
        for q in range(nq):
            assert oracle.rank_true_match(s[q], int(got_i[q, p])) == p + 1, (q, p)
    # a shard: the same columns under global indices
    sh_s, sh_i = _topk(scorer, s, k, global_col0=1000)
    np.testing.assert_array_equal(sh_i, np.where(want_i >= 0, want_i + 1000, -1))
    np.testing.assert_array_equal(_bits(sh_s), _bits(want_s))


def check_topk_edges(scorer):
    """Padding beyond the row, the empty row, the argument errors, and a leading dimension beyond the row."""
    lib, dev = scorer.lib, scorer.dev
    s = topk_matrix(2, 7)
    got_s, got_i = _topk(scorer, s, 10)
    want_s, want_i = expected_topk(s, 10)
    assert (want_i[:, 7:] == -1).all() and (want_i[:, :7] >= 0).all()
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
    got_s, got_i = _topk(scorer, np.zeros((3, 0), np.float32), 4)
    assert (got_i == -1).all() and not _bits(got_s).any()
    for k in (0, 257):
        with pytest.raises(RuntimeError):
            _topk(scorer, s, k)
    # the C entry point itself: error codes as the rank entry points give them
    sd = dev.to_device(np.array(s))
    o_s, o_i = dev.zeros((2, 4), np.float32), dev.zeros((2, 4), np.int32)
    args = lambda **kw: [kw.get("scores", dev.ptr(sd)), kw.get("ld", 7), kw.get("nq", 2), kw.get("ng", 7), None, kw.get("col0", 0),
                         kw.get("k", 4), kw.get("o_s", dev.ptr(o_s)), dev.ptr(o_i), dev.stream()]
    assert lib.spr_topk_rows(*args()) == 0
    for bad in ({"k": 0}, {"k": 257}, {"k": -1}, {"nq": -1}, {"ng": -1}, {"ld": 6}, {"scores": None}, {"o_s": None}, {"col0": -1},
                {"col0": 2 ** 31 - 3}):
        assert lib.spr_topk_rows(*args(**bad)) == _lib.SPR_ERR_ARG, bad
    assert lib.spr_topk_rows(*args(nq=0, scores=None)) == 0
    # ld > n_cols: the tail of every row (scores and index list) is never read as data
    nq, ng, ld, k = 3, 37, 50, 6
    s = topk_matrix(nq, ng)
    wide = np.full((nq, ld), 3.0e38, np.float32)
    wide[:, :ng] = s
    index = np.full((nq, ld), 5, np.int32)  # (a tail that looks like items)
    index[:, :ng] = np.random.default_rng(3).permutation(4 * ng)[:ng].astype(np.int32)[None] + np.arange(nq, dtype=np.int32)[:, None]
    index[:, 7] = -1
    wd, idd = dev.to_device(wide), dev.to_device(index)
    for col_index in (None, idd):
        o_s, o_i = dev.zeros((nq, k), np.float32), dev.zeros((nq, k), np.int32)
        lib.check(lib.spr_topk_rows(dev.ptr(wd), ld, nq, ng, None if col_index is None else dev.ptr(col_index), 0, k,
                                    dev.ptr(o_s), dev.ptr(o_i), dev.stream()))
        want_s, want_i = expected_topk(s, k, index=None if col_index is None else index[:, :ng])
        np.testing.assert_array_equal(dev.to_host(o_i), want_i)
        np.testing.assert_array_equal(_bits(dev.to_host(o_s)), _bits(want_s))


def check_strided_views_are_refused(scorer):
    """A strided view of a larger matrix is not a dense [Q, G] buffer: refused, not misread."""
    dev = scorer.dev
    wide = dev.to_device(np.array(topk_matrix(5, 300)))
    index = dev.to_device(np.tile(np.arange(300, dtype=np.int32), (5, 1)))
    with pytest.raises(ValueError, match="scores must be contiguous"):
        scorer.topk_device(wide[:, :100], 3, global_col0=5)
    with pytest.raises(ValueError, match="col_index must be contiguous"):
        scorer.topk_device(dev.to_device(np.array(topk_matrix(5, 300)[:, :100])), 3, col_index=index[:, :100])


def check_topk_merge(scorer):
    """Local top-k of three uneven column shards, concatenated (with empty slots) and merged == the global top-k."""
    rng = np.random.default_rng(21)
    s = rng.standard_normal((4, 1000)).astype(np.float32)
    s[:, ::5] = s[:, :1]
    s[:, 328:338] = 4.0   # ties at the top that straddle both shard boundaries
    s[:, 696:704] = 4.0
    s[2, 333] = s[2, 332] = 5.0
    bounds = [(0, 333), (333, 700), (700, 1000)]
    for k in (1, 20):
        cand_s, cand_i = [], []
        for a, b in bounds:
            ls, li = _topk(scorer, s[:, a:b], k, global_col0=a)
            want_s, want_i = expected_topk(s[:, a:b], k, col0=a)
            np.testing.assert_array_equal(li, want_i)
            cand_s += [ls, np.full((4, 2), 9.0e9, np.float32)]   # padding: no item, whatever the score slot holds
            cand_i += [li, np.full((4, 2), -1, np.int32)]
        got_s, got_i = _topk(scorer, np.concatenate(cand_s, axis=1), k, col_index=np.concatenate(cand_i, axis=1))
        want_s, want_i = expected_topk(s, k)
        np.testing.assert_array_equal(got_i, want_i)
        np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
        whole_s, whole_i = _topk(scorer, s, k)
        np.testing.assert_array_equal(got_i, whole_i)
        np.testing.assert_array_equal(_bits(got_s), _bits(whole_s))


def check_grid_stride(scorer, monkeypatch):
    """More rows / pairs than workgroups (SPR_TOPK_MAX_GRID lowers the 65 535 of a launch): the same results."""
    s = topk_matrix(5, 300)
    maps = peak_maps(3, 5, 16, 10)
    monkeypatch.setenv("SPR_TOPK_MAX_GRID", "2")
    got_s, got_i = _topk(scorer, s, 5, global_col0=7)
    score, yx = _peak(scorer, maps)
    monkeypatch.delenv("SPR_TOPK_MAX_GRID")
    want_s, want_i = expected_topk(s, 5, col0=7)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
    want_score, want_yx = expected_peak(maps)
    np.testing.assert_array_equal(_bits(score), _bits(want_score))
    np.testing.assert_array_equal(yx, want_yx)


# ------------------------------------------------------------------------------------------------ spr_maps_peak
@functools.lru_cache(maxsize=None)
def peak_maps(p, c, h, w):
    """[P,C,h,w] float32 of mixed signs and magnitudes from 1e-3 to 1e3 (the float64 partial sums depend on the order of the
    channels); pair 0 has an exact two-way tie of its summed maximum, the last of three pairs is all zero."""
    rng = np.random.default_rng(p * 1000003 + c * 1009 + h * 31 + w)
    maps = (10.0 ** rng.uniform(-3, 3, (p, c, h, w)) * rng.choice([-1.0, 1.0], (p, c, h, w))).astype(np.float32)
    n = h * w
    if n >= 3:
        flat = maps.reshape(p, c, n)
        flat[0, :, 2 * n // 3] = flat[0, :, n // 3] = 4096.0  # C * 4096 exactly, far above any sum of the random values
    if p >= 3:
        maps[p - 1] = 0.0
    maps.setflags(write=False)
    return maps


def expected_peak(maps):
    p, c, h, w = maps.shape
    score, yx = np.zeros(p, np.float32), np.zeros((p, 2), np.int32)
    for i in range(p):
        acc = np.zeros((h, w), np.float64)
        for ch in range(c):
            acc += maps[i, ch].astype(np.float64)
        pix = int(np.argmax(acc))
        score[i] = np.float32(acc.flat[pix] / c)
        yx[i] = divmod(pix, w)
    return score, yx


def _peak(scorer, maps, guard=8):
    """spr_maps_peak into the middle of guarded output buffers; the guard bands must come back untouched."""
    lib, dev = scorer.lib, scorer.dev
    p, c, h, w = maps.shape
    md = dev.to_device(np.array(maps))
    o_s = dev.to_device(np.full(p + 2 * guard, 777.0, np.float32))
    o_yx = dev.to_device(np.full(2 * p + 2 * guard, -777, np.int32))
    lib.check(lib.spr_maps_peak(dev.ptr(md), p, c, h, w, dev.ptr(o_s) + 4 * guard, dev.ptr(o_yx) + 4 * guard, dev.stream()))
    o_s, o_yx = dev.to_host(o_s), dev.to_host(o_yx)
    assert (o_s[:guard] == 777.0).all() and (o_s[guard + p:] == 777.0).all()
    assert (o_yx[:guard] == -777).all() and (o_yx[guard + 2 * p:] == -777).all()
    return o_s[guard:guard + p], o_yx[guard:guard + 2 * p].reshape(p, 2)


def check_maps_peak_exact(scorer, shape):
    maps = peak_maps(*shape)
    p, c, h, w = shape
    want_score, want_yx = expected_peak(maps)
    if h * w >= 3:  # the planted tie: the first of the two pixels in row-major order
        assert tuple(want_yx[0]) == divmod(h * w // 3, w) and want_score[0] == 4096.0
    if p >= 3:
        assert want_score[p - 1] == 0.0 and tuple(want_yx[p - 1]) == (0, 0)
    score, yx = _peak(scorer, maps)
    np.testing.assert_array_equal(yx, want_yx)
    np.testing.assert_array_equal(_bits(score), _bits(want_score))


def check_maps_peak_arguments(scorer):
    lib, dev = scorer.lib, scorer.dev
    md, o_s, o_yx = dev.zeros((1, 2, 3, 4), np.float32), dev.zeros((1,), np.float32), dev.zeros((2,), np.int32)
    ok = [dev.ptr(md), 1, 2, 3, 4, dev.ptr(o_s), dev.ptr(o_yx), dev.stream()]
    assert lib.spr_maps_peak(*ok) == 0
    for pos, bad in ((1, -1), (2, 0), (3, 0), (4, 0), (0, None), (5, None), (6, None)):
        args = list(ok)
        args[pos] = bad
        assert lib.spr_maps_peak(*args) == _lib.SPR_ERR_ARG, (pos, bad)
    assert lib.spr_maps_peak(None, 0, 2, 3, 4, None, None, dev.stream()) == 0  # no pairs: nothing to do


# ------------------------------------------------------------------------------------------------ locate
def _rounded(items, storage):
    """The float32 values the scorer sees once the maps are stored as ``storage`` (the oracle's inputs)."""
    if storage == "bfloat16":
        return [synth.from_bfloat16_bits(synth.bfloat16_bits(a)) for a in items]
    return [np.asarray(a, np.float32) for a in items]


@functools.lru_cache(maxsize=None)
def planted_reference(case, storage):
    """Per pair of the case: oracle similarity, oracle peak and its lead over the runner-up pixel (computed once)."""
    seed, nq, ng, c, h, w = case
    q, g, m = synth.dataset(seed, nq, ng, c, h, w)
    q, g = _rounded(q, storage), _rounded(g, storage)
    sim, peak, lead = np.zeros((nq, ng)), np.zeros((nq, ng, 2), np.int64), np.zeros((nq, ng))
    for qi in range(nq):
        for gi in range(ng):
            summed = oracle.ncc_maps(q[qi][:, 2:-2, 2:-2], g[gi][:, 2:-2, 2:-2], precise=True).sum(axis=0)
            top = np.sort(summed.ravel())[::-1]
            sim[qi, gi] = float(oracle.get_similarity(q[qi], g[gi], precise=True))
            peak[qi, gi] = np.unravel_index(int(summed.argmax()), summed.shape)
            lead[qi, gi] = top[0] - top[1]
    return q, g, m, sim, peak, lead


def check_locate_planted(scorer, case):
    """Every pair of a synthetic set: score and peak against the oracle; true matches: the planted shift."""
    seed, nq, ng, c, h, w = case
    q, g, m, sim, peak, lead = planted_reference(case, scorer.storage)
    ih, iw = h - 4, w - 4
    pairs = [(qi, gi) for qi in range(nq) for gi in range(ng)]
    score, variant, yx = scorer.locate(q, g, pairs)
    assert score.dtype == np.float32 and variant.dtype == np.int32 and yx.dtype == np.int32 and yx.shape == (len(pairs), 2)
    assert not variant.any()
    score, yx = score.reshape(nq, ng), yx.reshape(nq, ng, 2)
    print(f"\n{case}: max |score - oracle| = {np.abs(score - sim).max():.2e}, smallest oracle lead = {lead.min():.2e}")
    np.testing.assert_allclose(score, sim, atol=TIGHT, rtol=0)
    sure = lead > POSITION_LEAD
    assert (~sure).sum() <= 0.1 * len(pairs)
    np.testing.assert_array_equal(yx[sure], peak[sure])
    short = similarity.retrieve(q, g, _cfg(), k=ng, scorer=scorer)
    for qi in range(nq):
        dy, dx = synth.query_shift(seed, qi)
        assert lead[qi, m[qi]] >= 0.5  # (the planted peaks stand far above their runner-up pixel)
        assert tuple(yx[qi, m[qi]]) == (ih // 2 + dy, iw // 2 + dx)
        p = int(np.nonzero(short.index[qi] == m[qi])[0][0])
        assert tuple(short.peak_yx[qi, p]) == (ih // 2 + dy, iw // 2 + dx) and tuple(short.offset[qi, p]) == (dy, dx)


def check_locate_variants(scorer):
    """The best variant per true-match pair against the oracle's variant lists: rotations and scales separately, then both
    set (the reference's 1 + (R+1)*S lists, similarity.py:321-353).

    Compared where the oracle's best variant leads the best DIFFERENT variant by more than 1e-4.  On this data set (20 x 14
    maps) Pillow's 3-degree NEAREST rotation and its 1.02 resize (int(20 * 1.02) = 20) leave the query unchanged inside the
    2-pixel crop (np.array_equal below), so variant 0 and that variant tie exactly on both sides in every pair; variants whose
    cropped maps are bit-identical count as one variant for the lead, and the lowest number of them - what np.argmax gives - is the required answer.  That leaves
    3 of 3 pairs under rotations (leads 0.39 and more), 3 of 3 under scales (0.19 and more) and, no variant being a copy
    there, 3 of 3 with both set."""
    z = np.load(os.path.join(GOLDEN, "variants.npz"))
    nq, ng, c, h, w, seed = (int(v) for v in z["shape"])
    q, g, m = synth.dataset(seed, nq, ng, c, h, w)
    pairs = [(qi, m[qi]) for qi in range(nq)]
    from shoeprint_image_retrieval_amd.variants import variant_labels

    for rot, sc in (([-15, 3, 180], None), (None, [1.02, 1.08]), ([9, 180], [1.08, 0.9])):
        lists = oracle.transform_variants(q, rot, sc)
        assert len(variant_labels(rot, sc)) == len(lists)
        score, variant, yx = scorer.locate(q, g, pairs, rotations=rot, scales=sc)
        compared = 0
        for qi in range(nq):
            sims = np.array([float(oracle.get_similarity(v[qi], g[m[qi]], precise=True)) for v in lists])
            best = int(np.argmax(sims))
            seen = lambda v: v[qi][:, 2:-2, 2:-2]  # what the scorer sees of a variant: its maps under the crop
            other = [sims[k] for k, v in enumerate(lists)
                     if not (seen(v).shape == seen(lists[best]).shape and np.array_equal(seen(v), seen(lists[best])))]
            if sims[best] - max(other) <= 1e-4:
                continue
            compared += 1
            assert variant[qi] == best, (rot, sc, qi, variant[qi], sims)
            assert abs(score[qi] - sims[best]) <= TIGHT, (rot, sc, qi, score[qi], sims)
        assert 2 * compared >= nq, (rot, sc, compared)
    # a 180-degree copy of a gallery item comes back under the 180-degree variant, laid exactly on the print
    turned = [np.ascontiguousarray(g[1][:, ::-1, ::-1]), np.ascontiguousarray(g[4][:, ::-1, ::-1])]
    short = similarity.retrieve(turned, g, _cfg(rot=[-15, 3, 180]), k=2, scorer=scorer)
    np.testing.assert_array_equal(short.index[:, 0], [1, 4])
    np.testing.assert_array_equal(short.variant[:, 0], [3, 3])
    np.testing.assert_array_equal(short.offset[:, 0], [[0, 0], [0, 0]])
    np.testing.assert_array_equal(short.peak_yx[:, 0], [[(h - 4) // 2, (w - 4) // 2]] * 2)
    np.testing.assert_allclose(short.score[:, 0], 1.0, atol=TIGHT, rtol=0)
    # rotations AND scales: lists [original, 1.0, 1.08, 9 + 1.0, 9 + 1.08, 180 + 1.0, 180 + 1.08]; a resize by 1.0 is a copy, so
    # number 5 is the turned query turned back (offset 0) and number 6 cannot beat it; the true-match query of the data set
    # stays with number 0 (number 1 is its copy: the lowest number), shifted as planted
    rot, sc = [9, 180], [1.0, 1.08]
    labels = variant_labels(rot, sc)
    assert labels == ["original", "scale 1.0", "scale 1.08", "rotation 9, scale 1.0", "rotation 9, scale 1.08",
                      "rotation 180, scale 1.0", "rotation 180, scale 1.08"]
    assert variant_labels([3], None) == ["original", "rotation 3"] and variant_labels(None, None) == ["original"]
    short = similarity.retrieve(turned + [q[0]], g, _cfg(rot=rot, sc=sc), k=1, scorer=scorer)
    np.testing.assert_array_equal(short.index[:, 0], [1, 4, m[0]])
    np.testing.assert_array_equal(short.variant[:, 0], [5, 5, 0])
    assert [labels[v] for v in short.variant[:, 0]] == ["rotation 180, scale 1.0"] * 2 + ["original"]
    np.testing.assert_array_equal(short.offset[:, 0], [[0, 0], [0, 0], list(synth.query_shift(seed, 0))])
    # a larger template: the offset follows the winning variant's own size (scaled by 1.08: 21 x 15, cropped 17 x 11)
    big = similarity.retrieve([q[0]], g, _cfg(sc=[1.08]), k=1, scorer=scorer)
    score, variant, yx = scorer.locate([q[0]], g, [(0, int(big.index[0, 0]))], scales=[1.08])
    th, tw = (h - 4, w - 4) if variant[0] == 0 else (int(h * 1.08) - 4, int(w * 1.08) - 4)
    np.testing.assert_array_equal(big.offset[0, 0], [yx[0, 0] - th // 2, yx[0, 1] - tw // 2])
    forced = scorer._locate([np.ascontiguousarray(oracle.apply_transformations([q[0]], 1.08, "scale")[0])], g, [(0, m[0])], None, None)
    np.testing.assert_array_equal(forced[3], [[int(h * 1.08) - 4, int(w * 1.08) - 4]])


def check_retrieve_surface(scorer):
    z = np.load(os.path.join(GOLDEN, "compare_maps.npz"))
    nq, ng, c, h, w, seed = (int(v) for v in z["tiny_shape"])
    q, g, m = synth.dataset(seed, nq, ng, c, h, w)
    mat = scorer.score_matrix(q, g)
    short = similarity.retrieve(q, g, _cfg(), k=ng, locate=False, scorer=scorer)
    assert short.variant is None and short.peak_yx is None and short.offset is None
    assert short.index.dtype == np.int32 and short.score.dtype == np.float32 and short.index.shape == short.score.shape == (nq, ng)
    for qi in range(nq):
        assert sorted(short.index[qi]) == list(range(ng))
        assert int(np.nonzero(short.index[qi] == m[qi])[0][0]) + 1 == z["tiny_ranks"][qi]  # the real reference's rank
        np.testing.assert_array_equal(_bits(short.score[qi]), _bits(mat[qi, short.index[qi]]))
    # the ragged golden set, located; k beyond the gallery pads with -1
    rq = [synth.query_features(1236, i, i, 6, hh, ww) for i, (hh, ww) in enumerate([(18, 12), (16, 14), (18, 12)])]
    rg = [synth.gallery_features(1236, i, 6, hh, ww) for i, (hh, ww) in
          enumerate([(18, 12), (20, 12), (16, 14), (18, 12), (17, 15)])]
    rmat = scorer.score_matrix(rq, rg)
    for k in (3, 8):
        short = similarity.retrieve(rq, rg, _cfg(), k=k, scorer=scorer)
        want_s, want_i = expected_topk(rmat, k)
        np.testing.assert_array_equal(short.index, want_i)
        np.testing.assert_array_equal(_bits(short.score), _bits(want_s))
        assert short.variant.shape == (3, k) and short.peak_yx.shape == short.offset.shape == (3, k, 2)
        assert short.variant.dtype == short.peak_yx.dtype == short.offset.dtype == np.int32
        filled = want_i >= 0
        assert (short.variant[filled] == 0).all() and (short.variant[~filled] == -1).all()
        assert (short.peak_yx[~filled] == -1).all() and not short.offset[~filled].any()
        for qi in range(3):
            for p in np.nonzero(filled[qi])[0]:
                gi = int(want_i[qi, p])
                summed = oracle.ncc_maps(rq[qi][:, 2:-2, 2:-2], rg[gi][:, 2:-2, 2:-2], precise=True).sum(axis=0)
                top = np.sort(summed.ravel())[::-1]
                if top[0] - top[1] > POSITION_LEAD:
                    y, x = np.unravel_index(int(summed.argmax()), summed.shape)
                    assert tuple(short.peak_yx[qi, p]) == (y, x)
                    assert tuple(short.offset[qi, p]) == (y - (rq[qi].shape[1] - 4) // 2, x - (rq[qi].shape[2] - 4) // 2)
    assert (np.array([z["ragged_ranks"][qi] for qi in range(3)]) ==
            [int(np.nonzero(expected_topk(rmat, 5)[1][qi] == mm)[0][0]) + 1 for qi, mm in enumerate([0, 2, 3])]).all()
    empty = similarity.retrieve([], rg, _cfg(), k=2, scorer=scorer)
    assert empty.index.shape == (0, 2) and empty.offset.shape == (0, 2, 2)
