"""Checks of spr_ncc_score_peaks - the pair kernels' arg-max beside their max - and of its host mirror
(NccScorer.score_prepared(peaks=...), score_matrix_located, the fused similarity.retrieve), shared by the CPU-emulation runner
(test_emu_peaks.py, not gpu) and the MI355X runner (test_gpu_peaks.py, gpu).

The contract (include/shoeprint_mi355x.h) is exact: scores bit for bit those of spr_ncc_score, the position the first maximum
of the float32 channel sums in row-major order.  Positions are therefore compared exactly wherever the float64 oracle names the
pixel beyond doubt (planted peaks with a margin of 1e-3, leads above POSITION_LEAD = 1e-4 = 20 x TIGHT), and everywhere else
the pixel the kernel names must lie within POSITION_LEAD of the oracle's maximum - a mis-mapped accumulator slot names a pixel
far below that.  Every buffer the entry point writes sits between guard bands inside a wider matrix (ld > n_gallery, col0 > 0).
"""

import os

import numpy as np

import ncc_map_cases as mc
import shortlist_cases as sc_cases
from oracle import ncc_oracle as oracle
from parity_cases import GOLDEN, TIGHT
from shortlist_cases import POSITION_LEAD
from shoeprint_image_retrieval_amd import _lib, similarity, synth
from shoeprint_image_retrieval_amd.variants import VariantBuilder, variant_labels

GUARD = 8
POISON_F, POISON_I = 777.0, -777
EXTRA_LD, COL0 = 5, 3  # the matrices the entry point writes are ld = n_gallery + 5 wide and start at column 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unpack(packed):
    """(y << 16) | x -> [..., 2], -1 stays (-1, -1)."""
    packed = np.asarray(packed, dtype=np.int32)
    return np.where((packed < 0)[..., None], -1, np.stack([packed >> 16, packed & 0xFFFF], axis=-1)).astype(np.int32)


class PeakMatrices:
    """scores / peak_yx / peak_tag of one [nq, ng] block inside guarded, wider device buffers, started at 0 / -1 / -1."""

    def __init__(self, scorer, nq, ng, with_tags=True):
        self.sc, self.nq, self.ng, self.ld = scorer, nq, ng, ng + EXTRA_LD
        n = nq * self.ld + 2 * GUARD
        self.inside = np.zeros(n, dtype=bool)
        body = self.inside[GUARD:GUARD + nq * self.ld].reshape(nq, self.ld)
        body[:, COL0:COL0 + ng] = True
        dev = scorer.dev
        self.scores = dev.to_device(np.where(self.inside, 0.0, POISON_F).astype(np.float32))
        self.yx = dev.to_device(np.where(self.inside, -1, POISON_I).astype(np.int32))
        self.tags = dev.to_device(np.where(self.inside, -1, POISON_I).astype(np.int32)) if with_tags else None

    def score(self, plan, pq, pg, accumulate=False, tag=0):
        dev, lib = self.sc.dev, self.sc.lib
        return lib.spr_ncc_score_peaks(plan.handle, dev.ptr(pq), self.nq, dev.ptr(pg), self.ng, dev.ptr(self.scores) + 4 * GUARD,
                                       dev.ptr(self.yx) + 4 * GUARD, None if self.tags is None else dev.ptr(self.tags) + 4 * GUARD,
                                       self.ld, COL0, 1 if accumulate else 0, tag, dev.stream())

    def read(self):
        """(scores, packed positions, tags or None) of the block; guard bands and the columns outside the block untouched."""
        dev = self.sc.dev
        out = []
        for buf, poison in ((self.scores, POISON_F), (self.yx, POISON_I), (self.tags, POISON_I)):
            if buf is None:
                out.append(None)
                continue
            host = np.array(dev.to_host(buf))
            assert (host[~self.inside] == poison).all(), "written outside the [n_queries, n_gallery] block"
            out.append(host[self.inside].reshape(self.nq, self.ng))
        return out


def prepare(scorer, plan, q_batch, g_batch):
    dev = scorer.dev
    return scorer.prepare_queries(plan, dev.to_device(q_batch)), scorer.prepare_gallery(plan, dev.to_device(g_batch))


def plain_scores(scorer, plan, pq, nq, pg, ng):
    s = scorer.dev.zeros((nq, ng), np.float32)
    scorer.score_prepared(plan, pq, nq, pg, ng, s, ng, 0)
    return np.array(scorer.dev.to_host(s))


def score_peaks(scorer, plan, pq, nq, pg, ng, with_tags=True, tag=0):
    """One non-accumulating spr_ncc_score_peaks call: (scores, yx [nq, ng, 2], tags), scores checked against spr_ncc_score."""
    m = PeakMatrices(scorer, nq, ng, with_tags)
    scorer.lib.check(m.score(plan, pq, pg, tag=tag))
    scores, packed, tags = m.read()
    np.testing.assert_array_equal(bits(scores), bits(plain_scores(scorer, plan, pq, nq, pg, ng)))
    hit = scores > 0
    assert (packed[~hit] == -1).all() and (packed[hit] >= 0).all()
    if tags is not None:
        assert (tags[hit] == tag).all() and (tags[~hit] == -1).all()
    return scores, unpack(packed), tags


# ------------------------------------------------------------------------------------------------ 1. planted peaks
DIRECT_SWEEPS = [((5, 5), (16, 12)), ((9, 7), (90, 44))]


def check_sweep(make_scorer, case, monkeypatch, method="fft"):
    """Every template against every item of the oracle-checked sweep set; every good matched pair's peak is the planted pixel."""
    templates, items, pos, want, good = mc._sweep_inputs(case.t, case.i)
    mc._set_env(monkeypatch, case)
    sc = make_scorer(method)
    plan = sc.plan(1, case.t, case.i)
    if method == "fft":
        assert plan.fft_size == case.grid, case.id
    assert plan.has_peaks
    pq, pg = prepare(sc, plan, templates[:, None], items[:, None])
    scores, yx, _ = score_peaks(sc, plan, pq, len(templates), pg, len(items))
    sc.close()
    off = [k for k in np.flatnonzero(good) if tuple(yx[k % mc.N_TEMPLATES, k]) != pos[k]]
    print(f"[peaks sweep] {case.id},{method}: {len(pos)} positions, {int(good.sum())} good, {len(off)} off")
    if off:
        lines = [f"item {k} planted at {pos[k]}: got {tuple(yx[k % mc.N_TEMPLATES, k])}" for k in off[:25]]
        raise AssertionError(f"{case.id},{method}: {len(off)} planted peaks off: planted rows {sorted({pos[k][0] for k in off})}, "
                             f"planted columns {sorted({pos[k][1] for k in off})}\n" + "\n".join(lines))


def direct_sweep_case(t, i):
    return mc.SweepCase(t, i, "direct", len(mc.sweep_positions(*i)))


# ------------------------------------------------------------------------------------------------ 2. every instance
INSTANCE_CASES = mc.BASE_CASES + mc.POW2_CASES + mc.STORAGE_CASES + [big for _, big in mc.FORCE_BIG_CASES]


def check_instance(make_scorer, case, monkeypatch, method=None):
    """One multi-channel pair with dead channels: the named pixel holds the oracle's maximum within POSITION_LEAD."""
    q, g, want = mc._inputs(case.t, case.i, case.channels, case.dtype)
    sc, plan = mc.make_plan(make_scorer, case, monkeypatch, method)
    assert plan.has_peaks
    pq, pg = prepare(sc, plan, q[None], g[None])
    scores, yx, tags = score_peaks(sc, plan, pq, 1, pg, 1, tag=4)
    sc.close()
    summed = want.sum(axis=0)
    top = float(summed.max())
    y, x = (int(v) for v in yx[0, 0])
    print(f"[peaks instance] {case.id}{',direct' if method else ''}: score {scores[0, 0]:.7f}, peak ({y}, {x}), oracle max {top:.7f}"
          f"{'' if y < 0 else f', oracle at peak {summed[y, x]:.7f}'}")
    if top < -TIGHT:
        assert scores[0, 0] == 0 and (y, x) == (-1, -1) and tags[0, 0] == -1
        return
    if top > TIGHT:
        assert scores[0, 0] > 0
    if scores[0, 0] > 0:
        assert 0 <= y < case.i[0] and 0 <= x < case.i[1], (case.id, y, x)
        assert summed[y, x] >= top - POSITION_LEAD, (case.id, (y, x), float(summed[y, x]), top)
        assert abs(float(scores[0, 0]) - top / case.channels) <= TIGHT


# ------------------------------------------------------------------------------------------------ 3. whole matrices
def score_tolerance(scorer, th, tw):
    """Bound on |score - float64 oracle| for a cropped th x tw template.  The FFT kernels reach parity_cases.TIGHT on every size
    of these tests.  The direct kernel forms each pixel of a channel's map as ONE float32 fma chain over the n = th * tw taps:
    every step rounds the running sum with a relative error of at most u = 2^-24, the running sum times 1/sigma stays within
    [-1, 1] (Cauchy-Schwarz on the normalised template and window), so the accumulated error behaves as a random walk of n
    steps of size <= u - standard deviation <= u * sqrt(n) - and the mean over channels does not enlarge it.  Four standard
    deviations: 4 * 2^-24 * sqrt(n), i.e. 3.0e-6 for the 16 x 10 templates (TIGHT governs) and 2.1e-5 for 124 x 60, still
    five times inside the 1e-4 contract (parity_cases.TOL).  From the number format and the tap count alone."""
    if scorer.method != _lib.NCC_DIRECT:
        return TIGHT
    return max(TIGHT, 4.0 * 2.0 ** -24 * float(np.sqrt(th * tw)))


def check_planted_matrix(scorer, case):
    seed, nq, ng, c, h, w = case
    q, g, m, sim, peak, lead = sc_cases.planted_reference(case, scorer.storage)
    ih, iw = h - 4, w - 4
    scores, variant, yx = scorer.score_matrix_located(q, g)
    assert scores.dtype == np.float32 and variant.dtype == np.int32 and yx.dtype == np.int32
    assert scores.shape == variant.shape == (nq, ng) and yx.shape == (nq, ng, 2)
    np.testing.assert_array_equal(bits(scores), bits(scorer.score_matrix(q, g)))
    tol = score_tolerance(scorer, h - 4, w - 4)
    print(f"[peaks matrix] {case}: max |score - oracle| = {np.abs(scores - np.maximum(sim, 0.0)).max():.2e}, bound {tol:.2e}")
    np.testing.assert_allclose(scores, np.maximum(sim, 0.0), atol=tol, rtol=0)
    hit = scores > 0
    assert (variant[hit] == 0).all() and (variant[~hit] == -1).all() and (yx[~hit] == -1).all()
    sure = (lead > POSITION_LEAD) & hit
    print(f"[peaks matrix] {case}: {int(sure.sum())} of {nq * ng} pairs compared")
    np.testing.assert_array_equal(yx[sure], peak[sure])
    for qi in range(nq):
        dy, dx = synth.query_shift(seed, qi)
        assert tuple(yx[qi, m[qi]]) == (ih // 2 + dy, iw // 2 + dx)


# ------------------------------------------------------------------------------------------------ 4. variants, accumulate
def check_accumulate_rule(make_scorer, method="fft"):
    """Two query batches A, B against the same items through accumulate_max, in both orders of the calls and of the tags."""
    t, i = (5, 5), (16, 12)
    templates, items, pos, want, good = mc._sweep_inputs(t, i)
    sc = make_scorer(method)
    plan = sc.plan(1, t, i)
    nq, ng = len(templates), len(items)
    pq_a, pg = prepare(sc, plan, templates[:, None], items[:, None])
    pq_b = sc.prepare_queries(plan, sc.dev.to_device(np.ascontiguousarray(np.roll(templates, 1, axis=0)[:, None])))
    s_a, yx_a, _ = score_peaks(sc, plan, pq_a, nq, pg, ng)
    s_b, yx_b, _ = score_peaks(sc, plan, pq_b, nq, pg, ng)
    assert (s_b > s_a).any() and (s_b < s_a).any()  # both a strictly better and a worse second batch occur

    def run(calls, with_tags=True):
        m = PeakMatrices(sc, nq, ng, with_tags)
        for pq, tag in calls:
            sc.lib.check(m.score(plan, pq, pg, accumulate=True, tag=tag))
        s, packed, tags = m.read()
        return s, unpack(packed), tags

    # the same batch twice: equal scores, the lower tag stays whichever call brought it
    for tags_in in ((5, 2), (2, 5)):
        s, yx, tags = run([(pq_a, tags_in[0]), (pq_a, tags_in[1])])
        np.testing.assert_array_equal(bits(s), bits(s_a))
        np.testing.assert_array_equal(yx, yx_a)
        np.testing.assert_array_equal(tags, np.where(s_a > 0, 2, -1))
    # A then B, B then A: a strictly better second batch replaces all three values, a worse one none
    for first, second in (((pq_a, s_a, yx_a, 1), (pq_b, s_b, yx_b, 2)), ((pq_b, s_b, yx_b, 2), (pq_a, s_a, yx_a, 1))):
        s, yx, tags = run([(first[0], first[3]), (second[0], second[3])])
        take = second[1] > first[1]
        np.testing.assert_array_equal(bits(s), bits(np.where(take, second[1], first[1])))
        np.testing.assert_array_equal(yx, np.where(take[..., None], second[2], first[2]))
        want_tag = np.where(take, second[3], first[3])
        np.testing.assert_array_equal(tags, np.where(s > 0, want_tag, -1))
        # without a tag matrix: the same scores and positions where the scores differ
        s2, yx2, none = run([(first[0], first[3]), (second[0], second[3])], with_tags=False)
        assert none is None
        np.testing.assert_array_equal(bits(s2), bits(s))
        np.testing.assert_array_equal(yx2, yx)
    sc.close()


VARIANT_SETTINGS = (([-15, 3, 180], None), (None, [1.02, 1.08]), ([9, 180], [1.08, 0.9]))


def check_located_variants(scorer):
    """score_matrix_located under rotations / scales against the oracle's variant lists, by the rule of
    shortlist_cases.check_locate_variants: compared where the best variant leads every different variant by more than 1e-4,
    bit-identical cropped variants count as one, the lowest number is required."""
    z = np.load(os.path.join(GOLDEN, "variants.npz"))
    nq, ng, c, h, w, seed = (int(v) for v in z["shape"])
    q, g, m = synth.dataset(seed, nq, ng, c, h, w)
    for rot, sc in VARIANT_SETTINGS:
        lists = oracle.transform_variants(q, rot, sc)
        required = {}
        for qi in range(nq):
            sims = np.array([float(oracle.get_similarity(v[qi], g[m[qi]], precise=True)) for v in lists])
            best = int(np.argmax(sims))
            seen = lambda v: v[qi][:, 2:-2, 2:-2]
            other = [sims[k] for k, v in enumerate(lists)
                     if not (seen(v).shape == seen(lists[best]).shape and np.array_equal(seen(v), seen(lists[best])))]
            if sims[best] - max(other) > 1e-4:
                required[qi] = (best, sims[best])
        assert 2 * len(required) >= nq, (rot, sc, len(required))  # from the oracle alone
        scores, variant, yx = scorer.score_matrix_located(q, g, rotations=rot, scales=sc)
        np.testing.assert_array_equal(bits(scores), bits(scorer.score_matrix(q, g, rotations=rot, scales=sc)))
        assert ((variant >= 0) == (scores > 0)).all() and variant.max() < len(lists)
        for qi, (best, sim) in required.items():
            assert variant[qi, m[qi]] == best, (rot, sc, qi, variant[qi, m[qi]])
            assert abs(scores[qi, m[qi]] - sim) <= TIGHT
        # the position is that of the winning variant's own map
        pairs = [(qi, m[qi]) for qi in required]
        _, l_variant, l_yx = scorer.locate(q, g, pairs, rotations=rot, scales=sc)
        for k, (qi, gi) in enumerate(pairs):
            assert l_variant[k] == variant[qi, gi] and tuple(l_yx[k]) == tuple(yx[qi, gi]), (rot, sc, qi)


def ragged_set():
    rq = [synth.query_features(1236, i, i, 6, hh, ww) for i, (hh, ww) in enumerate([(18, 12), (16, 14), (18, 12)])]
    rg = [synth.gallery_features(1236, i, 6, hh, ww) for i, (hh, ww) in
          enumerate([(18, 12), (20, 12), (16, 14), (18, 12), (17, 15)])]
    return rq, rg


def check_ragged(scorer):
    rq, rg = ragged_set()
    scores, variant, yx = scorer.score_matrix_located(rq, rg)
    np.testing.assert_array_equal(bits(scores), bits(scorer.score_matrix(rq, rg)))
    pairs = [(qi, gi) for qi in range(len(rq)) for gi in range(len(rg))]
    _, l_variant, l_yx = scorer.locate(rq, rg, pairs)
    compared = 0
    for k, (qi, gi) in enumerate(pairs):
        summed = oracle.ncc_maps(rq[qi][:, 2:-2, 2:-2], rg[gi][:, 2:-2, 2:-2], precise=True).sum(axis=0)
        top = np.sort(summed.ravel())[::-1]
        if top[0] - top[1] > POSITION_LEAD and top[0] > TIGHT:
            compared += 1
            assert variant[qi, gi] == l_variant[k] == 0 and tuple(yx[qi, gi]) == tuple(l_yx[k]), (qi, gi)
            assert tuple(yx[qi, gi]) == np.unravel_index(int(summed.argmax()), summed.shape)
    assert 2 * compared >= len(pairs)


# ------------------------------------------------------------------------------------------------ 5. no second pass
def count_maps_calls(monkeypatch, lib):
    calls = []
    real = lib.spr_ncc_maps
    monkeypatch.setattr(lib, "spr_ncc_maps", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def check_no_second_pass(scorer, monkeypatch):
    """retrieve(locate=True) of a peak-capable scorer gathers from the located matrices: no spr_ncc_maps call."""
    case = sc_cases.PLANTED_CASES[0]
    q, g, m, sim, peak, lead = sc_cases.planted_reference(case, scorer.storage)
    calls = count_maps_calls(monkeypatch, scorer.lib)
    short = similarity.retrieve(q, g, sc_cases._cfg(), k=3, scorer=scorer)
    assert (short.score > 0).all()
    assert not calls, f"{len(calls)} spr_ncc_maps calls"
    for qi in range(len(q)):
        for p in range(3):
            gi = int(short.index[qi, p])
            assert short.variant[qi, p] == 0
            if lead[qi, gi] > POSITION_LEAD:
                assert tuple(short.peak_yx[qi, p]) == tuple(peak[qi, gi])
                assert tuple(short.offset[qi, p]) == (peak[qi, gi][0] - (case[4] - 4) // 2, peak[qi, gi][1] - (case[5] - 4) // 2)
    # k = the whole gallery: entries whose score is 0 (if any) still come back located, by the second pass
    full = similarity.retrieve(q, g, sc_cases._cfg(), k=len(g), scorer=scorer)
    assert (full.variant == 0).all() and (full.peak_yx >= 0).all()


def check_mfma_keeps_the_second_pass(scorer, monkeypatch):
    case = sc_cases.PLANTED_CASES[0]
    q, g, m, sim, peak, lead = sc_cases.planted_reference(case, scorer.storage)
    plan = scorer.plan(case[3], (case[4], case[5]), (case[4], case[5]), dtype=scorer.storage)
    assert plan.method == _lib.NCC_MFMA and not plan.has_peaks and scorer.lib.spr_ncc_plan_has_peaks(plan.handle) == 0
    pq, pg = scorer.prepare_queries(plan, scorer.dev.astype_storage(scorer.dev.stack_to_device(q), scorer.storage)), \
        scorer.prepare_gallery(plan, scorer.dev.astype_storage(scorer.dev.stack_to_device(g), scorer.storage))
    m_ = PeakMatrices(scorer, len(q), len(g))
    assert m_.score(plan, pq, pg) == _lib.SPR_ERR_UNSUPPORTED
    s, packed, tags = m_.read()
    assert not s.any() and (packed == -1).all() and (tags == -1).all()  # nothing was launched
    calls = count_maps_calls(monkeypatch, scorer.lib)
    short = similarity.retrieve(q, g, sc_cases._cfg(), k=3, scorer=scorer)
    assert len(calls) == len(q) * 3 * 1, len(calls)  # Q * k * V: the shortlisted pairs only, as before the peak form existed
    del calls[:]
    rot = [-15, 180]
    similarity.retrieve(q, g, sc_cases._cfg(rot=rot), k=2, scorer=scorer)
    assert len(calls) == len(q) * 2 * (1 + len(rot)), len(calls)
    scores = scorer.score_matrix(q, g)
    today = similarity._shortlist(scorer, q, g, scores, 3, True, None, None)
    for a, b in ((short.index, today.index), (bits(short.score), bits(today.score)), (short.variant, today.variant),
                 (short.peak_yx, today.peak_yx), (short.offset, today.offset)):
        np.testing.assert_array_equal(a, b)
    del calls[:]
    l_scores, l_variant, l_yx = scorer.score_matrix_located(q, g)  # the public form fills every pair of such a block
    assert len(calls) == len(q) * len(g)
    np.testing.assert_array_equal(bits(l_scores), bits(scores))
    sure = (lead > POSITION_LEAD) & (scores > 0)
    np.testing.assert_array_equal(l_yx[sure], peak[sure])


def check_has_peaks(make_scorer):
    for method, want in (("fft", 1), ("direct", 1)):
        sc = make_scorer(method)
        plan = sc.plan(2, (8, 6), (16, 8))
        assert sc.lib.spr_ncc_plan_has_peaks(plan.handle) == want and plan.has_peaks == bool(want)
        sc.close()
    assert sc.lib.spr_ncc_plan_has_peaks(None) == 0


# (method, storage, calls counted); the matrix-core scorer has no peak form: the unfused path (its plain score_matrix is the
# other scorers' walk, launch for launch, and the emulation of its pair kernel is slow)
CALL_COUNT_SCORERS = [("fft", "float32", ("score_matrix", "score_matrix_located", "locate")),
                      ("direct", "float32", ("score_matrix", "score_matrix_located", "locate")),
                      ("mfma", "bfloat16", ("score_matrix_located", "locate"))]
COUNTED = ("spr_ncc_prepare_gallery", "spr_ncc_prepare_queries", "spr_ncc_score", "spr_ncc_score_peaks", "spr_ncc_maps")


def count_calls(monkeypatch, lib):
    """A dict that counts, from now on, the VariantBuilder.variants calls ("expansions") and those of the COUNTED entry points."""
    n = dict.fromkeys(COUNTED + ("expansions",), 0)

    def counting(name, real):
        def call(*a, **kw):
            n[name] += 1
            return real(*a, **kw)
        return call

    for name in COUNTED:
        monkeypatch.setattr(lib, name, counting(name, getattr(lib, name)))
    monkeypatch.setattr(VariantBuilder, "variants", counting("expansions", VariantBuilder.variants))
    return n


def check_call_counts(make_scorer, monkeypatch, counted=("score_matrix", "score_matrix_located", "locate")):
    """How often score_matrix, score_matrix_located and locate expand, prepare and launch on the ragged set under one
    rotation and one scale, against counts derived here from the shapes, the pair list and the budget alone:

    * every query shape class of the call is expanded once;
    * a gallery chunk is prepared once per distinct variant shape of the query classes that meet it, whatever the number of
      classes and variants of that shape;
    * queries are prepared, and the pair kernels launched, once per (chunk, query class, variant);
    * the chunk size of a gallery class is min over its plans of budget // (number of plans) // bytes per item, at least 1;
    * locate visits only the classes and chunks of the items its pairs name, with one spr_ncc_maps call per pair and variant;
    * a scorer without a peak form adds to score_matrix_located a locate over every pair, a scorer with one adds nothing.

    The variant list is [original, scaled, rotated-then-scaled]: the last two share a shape, so each query class brings two
    variant shapes for three variants.  (Two shape classes of the ragged set - 18 x 12 and 16 x 14 - cannot share a variant
    shape under one scale s: that needs int(18 s) == int(16 s) and int(12 s) == int(14 s), or a scaled class equal to the other
    as it is, 16 s >= 18 with 14 s < 13 or 18 s < 17 with 12 s >= 14; none has a solution with maps larger than the crop.)
    The budget holds one item of each of a gallery class's four prepared forms and splits the two-item class into two chunks
    for the scoring walk; locate's pairs leave the 16 x 14 query and the 16 x 14 and 17 x 15 gallery items untouched."""
    rq, rg = ragged_set()
    rot, scale = [180], [0.9]
    n_variants = 3
    pairs = [(0, 0), (2, 3), (0, 1), (2, 0)]
    assert len(variant_labels(rot, scale)) == n_variants

    def shapes_of(a):  # the variant shapes of an item, in variant order
        h, w = a.shape[1:]
        scaled = (int(h * scale[0]), int(w * scale[0]))
        return [(h, w), scaled, scaled]

    def classes(items, used):
        groups = {}
        for i in used:
            groups.setdefault(items[i].shape[1:], []).append(i)
        return groups

    every = [(qi, gi) for qi in range(len(rq)) for gi in range(len(rg))]
    keys = ("expansions", "spr_ncc_prepare_gallery", "spr_ncc_prepare_queries", "launches", "spr_ncc_maps")

    def expected(sc, pair_list=None):
        """Counts of one walk: the scoring walk over everything (pair_list None) or locate over pair_list."""
        todo = every if pair_list is None else pair_list
        q_classes = classes(rq, sorted({qi for qi, _ in todo}))
        g_classes = classes(rg, sorted({gi for _, gi in todo}))
        want = dict.fromkeys(keys, 0)
        want["expansions"] = len(q_classes)
        for g_hw, g_idx in g_classes.items():
            plan_shapes = sorted({vs for q_idx in q_classes.values() for vs in shapes_of(rq[q_idx[0]])})
            per_item = [sc.plan(6, vs, g_hw, dtype=sc.storage).gallery_item_bytes for vs in plan_shapes]
            chunk = max(1, min(len(g_idx), min(sc.max_prepared_bytes // len(plan_shapes) // b for b in per_item)))
            for start in range(0, len(g_idx), chunk):
                part = g_idx[start:start + chunk]
                met = [q_idx for q_idx in q_classes.values() if any(qi in q_idx and gi in part for qi, gi in todo)]
                want["spr_ncc_prepare_gallery"] += len({vs for q_idx in met for vs in shapes_of(rq[q_idx[0]])})
                want["spr_ncc_prepare_queries"] += len(met) * n_variants
        if pair_list is None:
            want["launches"] = want["spr_ncc_prepare_queries"]
        else:
            want["spr_ncc_maps"] = len(pair_list) * n_variants
        return want

    sc = make_scorer()
    two_item_class = [sc.plan(6, vs, (18, 12), dtype=sc.storage) for q in rq[:2] for vs in set(shapes_of(q))]
    assert len({p.q_hw for p in two_item_class}) == 4
    budget = 4 * max(p.gallery_item_bytes for p in two_item_class) * 1 + 17  # room for one item of every form, not for two
    sc.close()
    sc = make_scorer(max_prepared_bytes=budget)
    fused = all(sc.plan(6, vs, g.shape[1:], dtype=sc.storage).has_peaks for q in rq for vs in shapes_of(q) for g in rg)
    n = count_calls(monkeypatch, sc.lib)
    for name, call, pair_list in (("score_matrix", lambda: sc.score_matrix(rq, rg, rotations=rot, scales=scale), None),
                                  ("score_matrix_located", lambda: sc.score_matrix_located(rq, rg, rotations=rot, scales=scale), None),
                                  ("locate", lambda: sc.locate(rq, rg, pairs, rotations=rot, scales=scale), pairs)):
        if name not in counted:
            continue
        before = dict(n)
        call()
        got = {k: n[k] - before[k] for k in n}
        got["launches"] = got.pop("spr_ncc_score") + got.pop("spr_ncc_score_peaks")
        want = expected(sc, pair_list)
        if pair_list is None:
            # the same in closed form: Qc = 2 query classes, V = 3 variants, S_g = 4 variant shapes, sum of K_g = 5 chunks
            # (four gallery classes, the two-item one in two chunks)
            assert want["spr_ncc_prepare_gallery"] == 5 * 4 and want["launches"] == 5 * 2 * n_variants
        if name == "score_matrix_located" and not fused:  # the second pass: a locate over every pair
            want = {k: want[k] + v for k, v in expected(sc, every).items()}
        print(f"[call counts] {name}, budget {budget}: {got}")
        assert got == want, (name, got, want)
    sc.close()


# ------------------------------------------------------------------------------------------------ 6. edges
EDGE_SHAPES = [("fft", (5, 5), (16, 12), 75), ("fft", (9, 7), (126, 64), 40), ("direct", (5, 5), (16, 12), 75)]
PAIR_TILE = 16  # the FFT pair kernels (four- and six-wave) launch in tiles of 16 queries x 16 gallery items


def check_edges(make_scorer, monkeypatch, method, t, i, n_items):
    """An odd query count, sliced launches, no tag matrix and an all-constant query, inside guarded wider matrices."""
    templates, items, pos, want, good = mc._sweep_inputs(t, i)
    items = items[:n_items]
    queries = np.concatenate([templates, np.full((2,) + t, 0.75, np.float32)])[:, None]  # 5 queries, the last two constant
    mc._set_env(monkeypatch, mc.SweepCase(t, i, "", 0))
    sc = make_scorer(method)
    plan = sc.plan(1, t, i)
    nq, ng = len(queries), len(items)
    assert nq % 2 == 1
    pq, pg = prepare(sc, plan, queries, items[:, None])
    scores, yx, tags = score_peaks(sc, plan, pq, nq, pg, ng, tag=9)
    assert not scores[3:].any() and (yx[3:] == -1).all() and (tags[3:] == -1).all()
    for k in np.flatnonzero(good[:ng]):
        assert tuple(yx[k % mc.N_TEMPLATES, k]) == pos[k]
    no_tag = score_peaks(sc, plan, pq, nq, pg, ng, with_tags=False)
    assert no_tag[2] is None
    np.testing.assert_array_equal(bits(no_tag[0]), bits(scores))
    np.testing.assert_array_equal(no_tag[1], yx)
    assert -(-nq // PAIR_TILE) * -(-ng // PAIR_TILE) >= 3  # one tile (direct: one gallery item) per launch: several launches
    monkeypatch.setenv("SPR_NCC_MAX_TILES", "1")
    sliced = score_peaks(sc, plan, pq, nq, pg, ng, tag=9)
    monkeypatch.delenv("SPR_NCC_MAX_TILES")
    np.testing.assert_array_equal(bits(sliced[0]), bits(scores))
    np.testing.assert_array_equal(sliced[1], yx)
    np.testing.assert_array_equal(sliced[2], tags)
    # argument checks as spr_ncc_score makes them
    m = PeakMatrices(sc, nq, ng)
    lib, dev = sc.lib, sc.dev
    ok = [plan.handle, dev.ptr(pq), nq, dev.ptr(pg), ng, dev.ptr(m.scores) + 4 * GUARD, dev.ptr(m.yx) + 4 * GUARD, None, m.ld, COL0, 0, 0,
          dev.stream()]
    for at, bad in ((0, None), (1, None), (3, None), (5, None), (6, None), (2, -1), (4, -1), (8, ng), (9, -1), (2, 65536)):
        args = list(ok)
        args[at] = bad
        assert lib.spr_ncc_score_peaks(*args) == _lib.SPR_ERR_ARG, (at, bad)
    args = list(ok)
    args[2] = 0
    assert lib.spr_ncc_score_peaks(*args) == 0
    m.read()  # nothing written by any of them
    sc.close()


# ------------------------------------------------------------------------------------------------ 8. torch op
SCHEMA = ("shoeprint_mi355x::ncc_scores_located(Tensor q, Tensor g, int crop=2, str method=\"auto\", int max_prepared_bytes=0)"
          " -> (Tensor, Tensor)")
