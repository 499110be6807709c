"""Checks of spr_ncc_score_surfaces - the list form that also stores every pair's channel-mean NCC map -, of spr_surface_peaks
and spr_maps_mean, and of what stands on them (NccScorer.pair_surfaces, similarity.retrieve(..., surfaces=True)), shared by the
CPU-emulation runner (test_emu_surfaces.py, not gpu) and the MI355X runner (test_gpu_surfaces.py, gpu).

The contract (include/shoeprint_mi355x.h) is exact towards the sibling: the three list outputs have the bits of
spr_ncc_score_list, max(max(surface), 0) has the bits of the score, and the surface at the peak holds its maximum.  Towards the
float64 oracle every pixel is held to parity_cases.TIGHT, the bound ncc_map_cases holds each per-channel map to: a mean of C
values within a bound is within it.  spr_surface_peaks and spr_maps_mean are compared with NumPy restatements, values and
positions bit for bit; the peak-to-sidelobe ratio within 2^-22 relative: its final rounding to float32 (2^-24) plus a float64
accumulation error that is negligible for fewer than 2^15 pixels of magnitude <= 1.
"""

import functools

import numpy as np

import score_list_cases as lc
import shortlist_cases as sc_cases
from oracle import ncc_oracle as oracle
from parity_cases import BIG_SHAPE_CASES, SHAPE_CASES, TIGHT
from score_list_cases import GUARD, POISON_F, SENTINEL, START, bits
from shoeprint_image_retrieval_amd import _lib, similarity, synth

CROP = 2
PSR_REL = 2.0 ** -22
ANTI = lc.CASES[5]  # template 46 x 36 over a 16 x 16 map (64 x 64 grid): at every 'same' lag the template covers the whole map


def map_hw(case):
    return case.shape[3] - 2 * CROP, case.shape[4] - 2 * CROP


def case_counts(case):
    return (2, 3) if case.shape == BIG_SHAPE_CASES[3] else (lc.NQ, lc.NG)


class SurfOutputs(lc.ListOutputs):
    """The list outputs and beside them the surfaces [n, ih, iw], started at ``fill`` (NaN: an unwritten pixel shows) between
    guard bands of GUARD poisoned floats."""

    def __init__(self, scorer, n, hw, start=START, with_tags=True, fill=np.nan):
        super().__init__(scorer, n, start, with_tags)
        self.hw = hw
        host = np.full(n * hw[0] * hw[1] + 2 * GUARD, POISON_F, dtype=np.float32)
        host[GUARD:len(host) - GUARD] = fill
        self.surf = scorer.dev.to_device(host)

    def score(self, p, pairs_dev, n_pairs, accumulate=False, tag=0):
        dev, lib = self.sc.dev, self.sc.lib
        return lib.spr_ncc_score_surfaces(p.plan.handle, dev.ptr(p.pq), p.nq, dev.ptr(p.pg), p.ng, dev.ptr(pairs_dev), n_pairs,
                                          dev.ptr(self.scores) + 4 * GUARD, dev.ptr(self.yx) + 4 * GUARD,
                                          None if self.tags is None else dev.ptr(self.tags) + 4 * GUARD,
                                          dev.ptr(self.surf) + 4 * GUARD, 1 if accumulate else 0, tag, dev.stream())

    def read(self):
        """(scores, packed positions, tags or None, surfaces [n, ih, iw]); every guard band must be as it was."""
        triple = super().read()
        host = np.array(self.sc.dev.to_host(self.surf))
        assert (host[:GUARD] == POISON_F).all() and (host[len(host) - GUARD:] == POISON_F).all(), "written outside the surfaces"
        return (*triple, host[GUARD:len(host) - GUARD].reshape(self.n, *self.hw))

    def overwrite_surfaces(self, value):
        """The surfaces set to ``value`` behind the library's back: a later rewrite shows."""
        host = np.array(self.sc.dev.to_host(self.surf))
        host[GUARD:len(host) - GUARD] = value
        self.surf = self.sc.dev.to_device(host)


def run_surfaces(p, pairs, case, start=START, with_tags=True, tag=0):
    """One non-accumulating spr_ncc_score_surfaces call over ``pairs`` (host [n, 2])."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    out = SurfOutputs(p.scorer, len(pairs), map_hw(case), start, with_tags)
    p.scorer.lib.check(out.score(p, p.scorer.dev.to_device(pairs), len(pairs), tag=tag))
    return out.read()


def assert_same_bits(got, want, what):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32), err_msg=what)


def assert_surface_consequences(scores, yx, surfaces, what):
    """No NaN left; max(max(surface), 0) has the score's bits; where the score is positive the peak pixel holds the maximum."""
    assert not np.isnan(surfaces).any(), f"{what}: a pixel of a live entry was not written"
    for k in range(len(scores)):
        top = surfaces[k].max()
        assert_same_bits(np.float32(max(top, np.float32(0.0))), np.float32(scores[k]), f"{what}: entry {k}, floored maximum")
        if scores[k] > 0:
            assert yx[k] >= 0
            assert_same_bits(surfaces[k][yx[k] >> 16, yx[k] & 0xFFFF], top, f"{what}: entry {k}, the surface at the peak")
        else:
            assert yx[k] == -1


# ------------------------------------------------------------------------------------------------ 1. siblings, exact
def check_siblings(make_scorer, case):
    nq, ng = case_counts(case)
    p = lc.prepare(make_scorer, case, nq, ng)
    assert p.plan.has_surfaces and p.scorer.lib.spr_ncc_plan_has_surfaces(p.plan.handle) == 1
    for name, pairs in lc.case_lists(nq, ng, sum(case.shape)).items():
        want = lc.run_list(p, pairs, tag=3)
        got = run_surfaces(p, pairs, case, tag=3)
        for k in range(3):
            assert_same_bits(got[k], want[k], f"{case.id}, {name}: output {k} against spr_ncc_score_list")
        assert_surface_consequences(got[0], got[1], got[3], f"{case.id}, {name}")
        pairs = np.asarray(pairs)
        for a in range(len(pairs)):  # repeated pairs give equal surfaces
            for b in range(a):
                if tuple(pairs[a]) == tuple(pairs[b]):
                    assert_same_bits(got[3][a], got[3][b], f"{case.id}, {name}: entries {a} and {b} name one pair")
    # without a tag vector
    pairs = lc.case_lists(nq, ng, 5)["odd with repeats"]
    want = lc.run_list(p, pairs, with_tags=False, tag=3)
    got = run_surfaces(p, pairs, case, with_tags=False, tag=3)
    assert got[2] is None and want[2] is None
    for k in range(2):
        assert_same_bits(got[k], want[k], f"{case.id}, no tags: output {k}")
    assert_surface_consequences(got[0], got[1], got[3], f"{case.id}, no tags")
    # entries that name no item, interleaved: all four outputs keep what they held, their neighbours are right
    bad = [(-1, 0), (nq, 0), (0, -1), (0, ng)]
    valid = lc.case_lists(nq, ng, 6)["permutation"][:5]
    mixed = np.array([bad[0], valid[0], bad[1], bad[2], valid[1], valid[2], bad[3], valid[3], valid[4]], dtype=np.int32)
    is_bad = np.array([tuple(e) in bad for e in mixed.tolist()])
    want = lc.run_list(p, mixed, start=SENTINEL, tag=3)
    got = run_surfaces(p, mixed, case, start=SENTINEL, tag=3)
    for k in range(3):
        assert_same_bits(got[k], want[k], f"{case.id}, skipped entries: output {k}")
        assert (got[k][is_bad] == SENTINEL[k]).all()
    assert np.isnan(got[3][is_bad]).all(), f"{case.id}: the surface of a skipped entry was written"
    assert_surface_consequences(got[0][~is_bad], got[1][~is_bad], got[3][~is_bad], f"{case.id}, neighbours of skipped entries")
    got = run_surfaces(p, np.array(bad, dtype=np.int32), case, start=SENTINEL)
    assert all((got[k] == SENTINEL[k]).all() for k in range(3)) and np.isnan(got[3]).all()
    p.scorer.close()


# ------------------------------------------------------------------------------------------------ 2. the oracle
def case_maps(case, nq, ng, seed=0):
    """The maps score_list_cases.prepare uploads for the case, as the scorer sees them once stored."""
    c, qh, qw, gh, gw = case.shape
    rng = np.random.default_rng(1000 * seed + sum(case.shape))
    q = rng.random((nq, c, qh, qw), dtype=np.float32)
    g = rng.random((ng, c, gh, gw), dtype=np.float32)
    if case.storage == "float16":
        q, g = q.astype(np.float16).astype(np.float32), g.astype(np.float16).astype(np.float32)
    if case.storage == "bfloat16":
        q, g = synth.from_bfloat16_bits(synth.bfloat16_bits(q)), synth.from_bfloat16_bits(synth.bfloat16_bits(g))
    return q, g


def oracle_surface(q, g):
    """The float64 channel-mean map of one [C, h, w] query over one [C, h', w'] gallery item."""
    return oracle.ncc_maps(q[:, CROP:-CROP, CROP:-CROP], g[:, CROP:-CROP, CROP:-CROP], precise=True).mean(axis=0)


def check_oracle(make_scorer, case):
    nq, ng = case_counts(case)
    p = lc.prepare(make_scorer, case, nq, ng)
    q, g = case_maps(case, nq, ng)
    pairs = np.array([(a, b) for a in range(nq) for b in range(ng)], dtype=np.int32)
    got = run_surfaces(p, pairs, case)
    worst = 0.0
    for k, (a, b) in enumerate(pairs):
        worst = max(worst, float(np.abs(got[3][k] - oracle_surface(q[a], g[b])).max()))
    print(f"\n[surfaces] {case.id}: max |surface - oracle mean map| over {len(pairs)} pairs = {worst:.2e}, bound {TIGHT:.0e}")
    assert worst <= TIGHT
    p.scorer.close()


def check_anticorrelated(make_scorer, case=ANTI):
    """A map that is negative everywhere: the score is 0, the peak -1, and the surface is written all the same.  The template
    is a convex paraboloid at least twice the map's size, the map a concave one: at every 'same' lag the template covers the
    whole map, the lag's linear term meets a symmetric zero-mean map and vanishes, and what is left is -var(r^2)."""
    c, qh, qw, gh, gw = case.shape
    assert qh - 2 * CROP >= 2 * (gh - 2 * CROP) and qw - 2 * CROP >= 2 * (gw - 2 * CROP)
    yy, xx = np.mgrid[0:qh, 0:qw]
    t = ((yy - qh / 2) ** 2 + (xx - qw / 2) ** 2).astype(np.float32)
    yy, xx = np.mgrid[0:gh, 0:gw]
    i = (-((yy - (gh - 1) / 2) ** 2 + (xx - (gw - 1) / 2) ** 2)).astype(np.float32)
    q = np.stack([t * (k + 1) for k in range(c)])[None]
    g = np.stack([i * (k + 2) for k in range(c)])[None]
    want = oracle_surface(q[0], g[0])
    assert want.max() < -1000 * TIGHT  # (from the oracle: negative everywhere, and far from 0 on the scale of the bound)
    sc = make_scorer(case.method, storage=case.storage)
    plan = sc.plan(c, (qh, qw), (gh, gw), dtype=case.storage)
    assert plan.fft_size == case.grid
    p = lc.Prepared(sc, plan, sc.prepare_queries(plan, sc.dev.to_device(q)), 1, sc.prepare_gallery(plan, sc.dev.to_device(g)), 1)
    got = run_surfaces(p, [(0, 0)], case, start=SENTINEL)
    assert (got[0][0], got[1][0], got[2][0]) == (0.0, -1, -1)
    assert not np.isnan(got[3]).any() and got[3].max() < 0
    print(f"\n[surfaces] anti-correlated pair: max |surface - oracle| = {np.abs(got[3][0] - want).max():.2e}, bound {TIGHT:.0e}")
    np.testing.assert_allclose(got[3][0], want, atol=TIGHT, rtol=0)
    sc.close()


# ------------------------------------------------------------------------------------------------ 3. the accumulate rule
def check_accumulate(make_scorer, case=lc.SMALL, n_variants=3):
    """Query sets as variants through accumulate_max, tags in shuffled order: every entry's surface ends as the surface of the
    call that won it (its final tag), the triple is spr_ncc_score_list's driven the same way; then the rule's corners."""
    c, qh, qw, gh, gw = case.shape
    nq, ng = case_counts(case)
    p = lc.prepare(make_scorer, case, nq, ng)
    sc, dev = p.scorer, p.scorer.dev
    rng = np.random.default_rng(77 + n_variants)
    batches = [p.pq] + [sc.prepare_queries(p.plan, dev.astype_storage(dev.to_device(
        rng.random((nq, c, qh, qw), dtype=np.float32)), case.storage)) for _ in range(n_variants - 1)]
    order = {2: [1, 0], 3: [2, 0, 1]}[n_variants]
    every = lc.case_lists(nq, ng, 9)["permutation"]
    bad = np.array([(nq, 0)], dtype=np.int32)
    pairs = np.concatenate([every[:4], bad, every[4:], every[:2], np.array([(-1, -1)], dtype=np.int32)])  # repeats, padding: odd
    is_bad = (pairs[:, 0] < 0) | (pairs[:, 0] >= nq)
    assert len(pairs) % 2 == 1
    pairs_dev = dev.to_device(np.ascontiguousarray(pairs, dtype=np.int32))
    alone = {tag: run_surfaces(p._replace(pq=pq), pairs, case, tag=tag) for pq, tag in zip(batches, order)}
    ref = lc.ListOutputs(sc, len(pairs), START)
    out = SurfOutputs(sc, len(pairs), map_hw(case), START)
    for pq, tag in zip(batches, order):
        sc.lib.check(ref.score(p._replace(pq=pq), pairs_dev, len(pairs), accumulate=True, tag=tag))
        sc.lib.check(out.score(p._replace(pq=pq), pairs_dev, len(pairs), accumulate=True, tag=tag))
    want, got = ref.read(), out.read()
    for k in range(3):
        assert_same_bits(got[k], want[k], f"accumulate: output {k} against spr_ncc_score_list")
    assert len(set(got[2][~is_bad].tolist()) - {-1}) >= 2  # (more than one variant wins somewhere)
    for k in range(len(pairs)):
        if is_bad[k] or got[2][k] < 0:  # skipped, or never above 0: nobody wrote the surface
            assert np.isnan(got[3][k]).all() and (is_bad[k] or got[0][k] == 0.0)
            continue
        assert_same_bits(got[3][k], alone[int(got[2][k])][3][k], f"accumulate: entry {k} holds the map of the call that won it")
    assert_surface_consequences(got[0][~is_bad & (got[2] >= 0)], got[1][~is_bad & (got[2] >= 0)], got[3][~is_bad & (got[2] >= 0)],
                                "accumulate")
    for k in range(3):
        assert (got[k][is_bad] == START[k]).all()
    # a call that replaces nothing leaves every surface bit-identical: the last batch again under a tag above all others ...
    before = got
    sc.lib.check(out.score(p._replace(pq=batches[-1]), pairs_dev, len(pairs), accumulate=True, tag=99))
    after = out.read()
    for k in range(4):
        assert_same_bits(after[k], before[k], f"a call that replaces nothing: output {k}")
    # ... an equal score under a higher tag does not replace, under a lower tag it does: the surfaces are overwritten behind the
    # library's back, so a rewrite shows
    winner_tag = order[-1]
    won_last = ~is_bad & (before[2] == winner_tag)
    assert won_last.any()
    out.overwrite_surfaces(123.0)
    sc.lib.check(out.score(p._replace(pq=batches[-1]), pairs_dev, len(pairs), accumulate=True, tag=winner_tag + 50))
    after = out.read()
    assert (after[3] == 123.0).all() and (after[2] == before[2]).all()
    sc.lib.check(out.score(p._replace(pq=batches[-1]), pairs_dev, len(pairs), accumulate=True, tag=-7))
    after = out.read()
    assert (after[2][won_last] == -7).all() and (after[2][~won_last] == before[2][~won_last]).all()
    assert (after[3][~won_last] == 123.0).all()
    assert_same_bits(after[3][won_last], before[3][won_last], "an equal score under a lower tag rewrites the surface")
    assert_same_bits(after[0], before[0], "scores")
    sc.close()


def check_slicing(make_scorer, monkeypatch, case=lc.SMALL):
    """SPR_NCC_MAX_TILES=1 (read at every launch): a list of several launches gives the bits of one launch."""
    p = lc.prepare(make_scorer, case)
    rng = np.random.default_rng(4)
    every = np.array([(q, g) for q in range(p.nq) for g in range(p.ng)], dtype=np.int32)
    n = {"direct": 5, "fft": 2 * 256 + 37, "fft_pow2": 2 * 256 + 37}[case.method]  # (one tile: 256 pairs, direct: one)
    if case.grid == (192, 96):
        n = 256 + 5
    pairs = every[rng.integers(0, len(every), n)]
    pairs[n // 2] = (-1, 0)
    want = run_surfaces(p, pairs, case, start=SENTINEL)
    monkeypatch.setenv("SPR_NCC_MAX_TILES", "1")
    got = run_surfaces(p, pairs, case, start=SENTINEL)
    monkeypatch.delenv("SPR_NCC_MAX_TILES")
    ok = np.arange(n) != n // 2
    for k in range(4):
        assert_same_bits(got[k], want[k], f"{case.id}, sliced: output {k}")
    assert np.isnan(got[3][n // 2]).all() and all(got[k][n // 2] == SENTINEL[k] for k in range(3))
    assert_surface_consequences(got[0][ok], got[1][ok], got[3][ok], f"{case.id}, sliced")
    p.scorer.close()


# ------------------------------------------------------------------------------------------------ 4. refusals and arguments
def check_arguments(make_scorer, monkeypatch):
    p = lc.prepare(make_scorer, lc.SMALL)
    sc, dev, lib = p.scorer, p.scorer.dev, p.scorer.lib
    pairs = dev.to_device(np.array([(0, 0), (1, 2)], dtype=np.int32))
    hw = map_hw(lc.SMALL)

    def call(prep=p, hw=hw, **kw):
        out = SurfOutputs(sc, 2, hw, SENTINEL)
        a = {"plan": prep.plan.handle, "pq": dev.ptr(prep.pq), "nq": prep.nq, "pg": dev.ptr(prep.pg), "ng": prep.ng,
             "pairs": dev.ptr(pairs), "n": 2, "scores": dev.ptr(out.scores) + 4 * GUARD, "yx": dev.ptr(out.yx) + 4 * GUARD,
             "tags": dev.ptr(out.tags) + 4 * GUARD, "surf": dev.ptr(out.surf) + 4 * GUARD}
        a.update(kw)
        rc = lib.spr_ncc_score_surfaces(a["plan"], a["pq"], a["nq"], a["pg"], a["ng"], a["pairs"], a["n"], a["scores"], a["yx"],
                                        a["tags"], a["surf"], 0, 0, dev.stream())
        return rc, out.read()

    def untouched(got):
        return all((got[k] == SENTINEL[k]).all() for k in range(3)) and np.isnan(got[3]).all()

    rc, got = call()
    assert rc == _lib.SPR_OK and not untouched(got) and not np.isnan(got[3]).any()
    rc, got = call(tags=None)
    assert rc == _lib.SPR_OK and (got[2] == SENTINEL[2]).all() and not np.isnan(got[3]).any()
    for bad in ({"plan": None}, {"pq": None}, {"pg": None}, {"pairs": None}, {"scores": None}, {"yx": None}, {"surf": None},
                {"nq": -1}, {"ng": -1}, {"n": -1}):
        rc, got = call(**bad)
        assert rc == _lib.SPR_ERR_ARG and untouched(got), bad
    rc, got = call(n=0)
    assert rc == _lib.SPR_OK and untouched(got)
    assert lib.spr_ncc_score_surfaces(p.plan.handle, None, 0, None, 0, None, 0, None, None, None, None, 0, 0, dev.stream()) == _lib.SPR_OK
    assert lib.spr_ncc_plan_has_surfaces(None) == 0
    sc.close()
    # plans without the form: the matrix-core method, and the workspace instance of the FFT method
    c, h, w = 4, 32, 16
    rng = np.random.default_rng(8)
    q, g = rng.random((lc.NQ, c, h, w), dtype=np.float32), rng.random((lc.NG, c, h, w), dtype=np.float32)
    monkeypatch.setenv("SPR_NCC_FORCE_BIG", "1")
    big_sc = make_scorer("fft")
    big_plan = big_sc.plan(c, (h, w), (h, w))
    monkeypatch.delenv("SPR_NCC_FORCE_BIG")
    mfma_sc = make_scorer("mfma", storage="bfloat16")
    mfma_plan = mfma_sc.plan(c, (h, w), (h, w), dtype="bfloat16")
    assert big_plan.method == _lib.NCC_FFT and mfma_plan.method == _lib.NCC_MFMA
    for s, plan, storage in ((big_sc, big_plan, "float32"), (mfma_sc, mfma_plan, "bfloat16")):
        assert not plan.has_surfaces and not plan.has_list
        assert lib.spr_ncc_plan_has_surfaces(plan.handle) == 0 == lib.spr_ncc_plan_has_list(plan.handle)
        pq = s.prepare_queries(plan, dev.astype_storage(dev.to_device(q), storage))
        pg = s.prepare_gallery(plan, dev.astype_storage(dev.to_device(g), storage))
        rc, got = call(prep=lc.Prepared(s, plan, pq, lc.NQ, pg, lc.NG), hw=(h - 2 * CROP, w - 2 * CROP))
        assert rc == _lib.SPR_ERR_UNSUPPORTED and untouched(got)
        s.close()


# ------------------------------------------------------------------------------------------------ 5. spr_surface_peaks
PEAK_SIZES = [(1, 1), (1, 37), (5, 3), (28, 12), (124, 60), (128, 64)]
PEAK_COUNTS = [1, 2, 8]


def peak_windows(h, w):
    """None, mid, and one that covers the whole surface from wherever the maximum lies (empty slots)."""
    return [(0, 0), (max(1, h // 5), max(1, w // 5)), (h, w)]


@functools.lru_cache(maxsize=None)
def peak_surfaces(h, w):
    """[7, h, w] float32 in [-1, 1): random; planted equal maxima (two, then four of them, for peak 0 and peak j); the maximum
    in each corner in turn (windows clipped at every edge); all negative."""
    rng = np.random.default_rng(100 * h + w)
    s = rng.uniform(-1.0, 1.0, (7, h, w)).astype(np.float32)
    n = h * w
    flat = s.reshape(7, n)
    flat[1, [n // 3, 2 * n // 3]] = 1.0
    flat[2, [n // 5, n // 2, (3 * n) // 4, n - 1]] = 1.0
    s[3, 0, 0], s[4, 0, w - 1], s[5, h - 1, 0] = 1.0, 1.0, 1.0
    s[5, h - 1, w - 1] = 1.0
    s[6] = -np.abs(s[6]) - np.float32(0.25)
    s.setflags(write=False)
    return s


def expected_surface_peaks(surfaces, n_peaks, ry, rx):
    """The NumPy restatement: (values [n, n_peaks], packed positions [n, n_peaks], psr float64 [n])."""
    n, h, w = surfaces.shape
    values = np.zeros((n, n_peaks), np.float32)
    yx = np.full((n, n_peaks), -1, np.int32)
    psr = np.zeros(n, np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(n):
        left = np.ones((h, w), bool)
        for j in range(n_peaks):
            if not left.any():
                break
            masked = np.where(left, surfaces[k], -np.inf)
            y, x = np.unravel_index(int(np.argmax(masked)), (h, w))  # (the first maximum in row-major order)
            values[k, j], yx[k, j] = surfaces[k, y, x], (y << 16) | x
            window = (np.abs(yy - y) <= ry) & (np.abs(xx - x) <= rx)
            if j == 0:
                side = surfaces[k][~window].astype(np.float64)
                if len(side) >= 2:
                    mu = side.sum() / len(side)
                    sigma = np.sqrt(np.square(side - mu).sum() / len(side))
                    psr[k] = 0.0 if sigma == 0 else (float(values[k, 0]) - mu) / sigma
            left &= ~window
    return values, yx, psr


def run_surface_peaks(scorer, surfaces, n_peaks, ry, rx, with_psr=True, guard=8):
    """spr_surface_peaks into the middle of guarded output buffers; the guard bands must come back untouched."""
    lib, dev = scorer.lib, scorer.dev
    n, h, w = surfaces.shape
    sd = dev.to_device(np.array(surfaces))
    o_v = dev.to_device(np.full(n * n_peaks + 2 * guard, 777.0, np.float32))
    o_yx = dev.to_device(np.full(n * n_peaks + 2 * guard, -777, np.int32))
    o_p = dev.to_device(np.full(n + 2 * guard, 777.0, np.float32))
    lib.check(lib.spr_surface_peaks(dev.ptr(sd), n, h, w, n_peaks, ry, rx, dev.ptr(o_v) + 4 * guard, dev.ptr(o_yx) + 4 * guard,
                                    dev.ptr(o_p) + 4 * guard if with_psr else None, dev.stream()))
    o_v, o_yx, o_p = dev.to_host(o_v), dev.to_host(o_yx), dev.to_host(o_p)
    for buf, poison, m in ((o_v, 777.0, n * n_peaks), (o_yx, -777, n * n_peaks), (o_p, 777.0, n if with_psr else 0)):
        assert (buf[:guard] == poison).all() and (buf[guard + m:] == poison).all()
    return o_v[guard:guard + n * n_peaks].reshape(n, n_peaks), o_yx[guard:guard + n * n_peaks].reshape(n, n_peaks), o_p[guard:guard + n]


def assert_psr(got, want, what):
    """|got - want| <= 2^-22 |want|; the float64 restatement itself holds the figure to far less (it IS the definition, and
    np.sum's pairwise float64 error on < 2^15 values of magnitude <= 1 is below 2^-45 relative to the sums)."""
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= PSR_REL * np.abs(want)).all(), f"{what}: psr {got} against {want}"


def check_surface_peaks(scorer, hw):
    h, w = hw
    surfaces = peak_surfaces(h, w)
    n = h * w
    for n_peaks in PEAK_COUNTS:
        for ry, rx in peak_windows(h, w):
            what = f"{h}x{w}, {n_peaks} peaks, window ({ry}, {rx})"
            want_v, want_yx, want_psr = expected_surface_peaks(surfaces, n_peaks, ry, rx)
            got_v, got_yx, got_psr = run_surface_peaks(scorer, surfaces, n_peaks, ry, rx)
            np.testing.assert_array_equal(got_yx, want_yx, err_msg=what)
            assert_same_bits(got_v, want_v, what)
            assert_psr(got_psr, want_psr, what)
            if (ry, rx) == (h, w) and n_peaks > 1:  # the window covers everything: one peak, the other slots empty, no side lobe
                assert (got_yx[:, 1:] == -1).all() and (got_v[:, 1:] == 0).all() and (got_psr == 0).all()
            if n >= 3:  # the planted ties: the first in row-major order wins
                assert got_yx[1, 0] == (((n // 3) // w) << 16 | (n // 3) % w) and got_v[1, 0] == 1.0
            assert (got_v[6, 0] < 0) and got_yx[6, 0] >= 0  # all negative: the maximum all the same
    if n >= 5:  # peak j among equal maxima: the first of those left, in row-major order
        _, got_yx, _ = run_surface_peaks(scorer, surfaces, 4, 0, 0)
        assert got_yx[2].tolist() == [((i // w) << 16) | (i % w) for i in (n // 5, n // 2, (3 * n) // 4, n - 1)]
    # without the ratio the other two outputs are the same
    got = run_surface_peaks(scorer, surfaces, 2, 1, 1, with_psr=False)
    want = run_surface_peaks(scorer, surfaces, 2, 1, 1)
    np.testing.assert_array_equal(got[1], want[1])
    assert_same_bits(got[0], want[0], "no psr")


def check_surface_peaks_edges(scorer):
    lib, dev = scorer.lib, scorer.dev
    # a constant surface and a surface with one side-lobe pixel give a ratio of exactly 0
    const = np.full((1, 6, 5), 0.3, np.float32)
    v, yx, psr = run_surface_peaks(scorer, const, 2, 1, 1)
    assert psr[0] == 0.0 and yx[0, 0] == 0 and v[0, 0] == np.float32(0.3)
    one = np.array([[[0.5, 0.1, 0.9]]], np.float32)  # the window (0, 1) around x = 2 leaves x = 0 alone
    v, yx, psr = run_surface_peaks(scorer, one, 2, 0, 1)
    assert psr[0] == 0.0 and yx[0].tolist() == [2, 0] and v[0].tolist() == [np.float32(0.9), np.float32(0.5)]
    # arguments
    sd, o_v, o_yx, o_p = dev.zeros((1, 3, 4), np.float32), dev.zeros((8,), np.float32), dev.zeros((8,), np.int32), dev.zeros((1,), np.float32)
    ok = [dev.ptr(sd), 1, 3, 4, 2, 1, 1, dev.ptr(o_v), dev.ptr(o_yx), dev.ptr(o_p), dev.stream()]
    assert lib.spr_surface_peaks(*ok) == 0
    for pos, bad in ((1, -1), (2, 0), (3, 0), (2, 32768), (3, 32768), (4, 0), (4, 9), (5, -1), (6, -1), (0, None), (7, None), (8, None)):
        args = list(ok)
        args[pos] = bad
        assert lib.spr_surface_peaks(*args) == _lib.SPR_ERR_ARG, (pos, bad)
    assert lib.spr_surface_peaks(None, 0, 3, 4, 2, 1, 1, None, None, None, dev.stream()) == 0  # n = 0: nothing to do
    args = list(ok)
    args[5], args[6] = 2 ** 31 - 1, 2 ** 31 - 1  # a window beyond any surface: one peak
    assert lib.spr_surface_peaks(*args) == 0 and dev.to_host(o_yx)[1] == -1


# ------------------------------------------------------------------------------------------------ 6. spr_maps_mean
def check_maps_mean(scorer, shape, guard=8):
    lib, dev = scorer.lib, scorer.dev
    maps = sc_cases.peak_maps(*shape)
    p, c, h, w = shape
    want = np.zeros((p, h, w), np.float32)
    for i in range(p):
        acc = np.zeros((h, w), np.float64)
        for ch in range(c):
            acc += maps[i, ch].astype(np.float64)
        want[i] = (acc / c).astype(np.float32)
    md = dev.to_device(np.array(maps))
    out = dev.to_device(np.full(p * h * w + 2 * guard, 777.0, np.float32))
    lib.check(lib.spr_maps_mean(dev.ptr(md), p, c, h, w, dev.ptr(out) + 4 * guard, dev.stream()))
    out = dev.to_host(out)
    assert (out[:guard] == 777.0).all() and (out[guard + p * h * w:] == 777.0).all()
    got = out[guard:guard + p * h * w].reshape(p, h, w)
    assert_same_bits(got, want, f"spr_maps_mean {shape}")
    score, _ = sc_cases._peak(scorer, maps)
    assert_same_bits(got.reshape(p, -1).max(axis=1), score, f"spr_maps_mean {shape}: the maximum against spr_maps_peak")


def check_maps_mean_arguments(scorer):
    lib, dev = scorer.lib, scorer.dev
    md, out = dev.zeros((1, 2, 3, 4), np.float32), dev.zeros((12,), np.float32)
    ok = [dev.ptr(md), 1, 2, 3, 4, dev.ptr(out), dev.stream()]
    assert lib.spr_maps_mean(*ok) == 0
    for pos, bad in ((1, -1), (2, 0), (3, 0), (4, 0), (0, None), (5, None)):
        args = list(ok)
        args[pos] = bad
        assert lib.spr_maps_mean(*args) == _lib.SPR_ERR_ARG, (pos, bad)
    assert lib.spr_maps_mean(None, 0, 2, 3, 4, None, dev.stream()) == 0


# ------------------------------------------------------------------------------------------------ 7. the Python layer
def check_pair_surfaces(scorer, q=None, g=None, rot=lc.ROT, sc=lc.SCALES, sides=None):
    """``pair_surfaces`` against ``score_pairs``: the triple (and t_hw) exact; every surface has its gallery item's cropped
    shape, its floored maximum is the score and its peak pixel holds the maximum."""
    if q is None:
        q, g = lc.ragged_sets()
    rng = np.random.default_rng(3)
    every = np.array([(a, b) for a in range(len(q)) for b in range(len(g))])
    pairs = np.concatenate([every[rng.permutation(len(every))], every[:4]])
    want = scorer.score_pairs(*(sides or (q, g)), pairs, rotations=rot, scales=sc)
    got = scorer.pair_surfaces(*(sides or (q, g)), pairs, rotations=rot, scales=sc)
    assert len(got) == 5 and len(got[4]) == len(pairs)
    assert_same_bits(got[0], want[0], "pair_surfaces: scores")
    for k in (1, 2, 3):
        np.testing.assert_array_equal(got[k], want[k])
    for k, (a, b) in enumerate(pairs):
        m = got[4][k]
        assert m.dtype == np.float32 and m.shape == (g[b].shape[1] - 2 * CROP, g[b].shape[2] - 2 * CROP)
    return pairs, got


def check_pair_surfaces_list_route(scorer, **kw):
    pairs, got = check_pair_surfaces(scorer, **kw)
    assert (got[0] > 0).any()
    hit = got[1] >= 0
    for k in np.flatnonzero(hit):
        m = got[4][k]
        assert_same_bits(m.max(), got[0][k], f"pair_surfaces: entry {k}, maximum")
        assert_same_bits(m[got[2][k, 0], got[2][k, 1]], m.max(), f"pair_surfaces: entry {k}, the surface at the peak")
    for k in np.flatnonzero(~hit):
        assert not got[4][k].any()
    empty = scorer.pair_surfaces(*lc.ragged_sets(), [])
    assert [a.shape for a in empty[:4]] == [(0,), (0,), (0, 2), (0, 2)] and empty[4] == []


def check_pair_surfaces_matrix_cores(make_scorer):
    """A set one of whose blocks goes to the matrix cores (bf16-stored [C, 32, 16] maps) beside one that takes the list route
    ([C, 40, 20]): on the former the fallback's surface maximum is ``locate``'s score."""
    rng = np.random.default_rng(12)
    bf = lambda items: [synth.from_bfloat16_bits(synth.bfloat16_bits(a)) for a in items]
    q = bf([rng.random((4, 32, 16), dtype=np.float32) for _ in range(3)])
    g = bf([rng.random((4, 32, 16), dtype=np.float32) for _ in range(3)] + [rng.random((4, 40, 20), dtype=np.float32) for _ in range(2)])
    scorer = make_scorer("auto", storage="bfloat16")
    pairs, got = check_pair_surfaces(scorer, q, g, rot=[180], sc=None)
    methods = {p.method for p in scorer._plans.values()}
    assert _lib.NCC_MFMA in methods and _lib.NCC_FFT in methods
    small = np.flatnonzero(pairs[:, 1] < 3)
    score, variant, yx = scorer.locate(q, g, pairs[small], rotations=[180])
    for k, s, v in zip(small, score, variant):
        if got[0][k] > 0:
            assert got[1][k] == v
            assert_same_bits(got[4][k].max(), s, f"matrix-core block, entry {k}: the fallback's maximum against locate")
        else:
            assert not got[4][k].any()
    scorer.close()


def check_retrieve_surfaces(scorer, case):
    """``retrieve(..., surfaces=True)`` on a planted set: everything ``retrieve`` returns is unchanged; the surface is the
    winning variant's map (against the oracle, within TIGHT); the peak fields are spr_surface_peaks of those maps."""
    seed, nq, ng, c, h, w = case
    q, g, m, sim, peak, lead = sc_cases.planted_reference(case, scorer.storage)
    k = ng + 1  # (one slot beyond the gallery: empty)
    plain = similarity.retrieve(q, g, sc_cases._cfg(), k=k, scorer=scorer)
    short = similarity.retrieve(q, g, sc_cases._cfg(), k=k, scorer=scorer, surfaces=True, peaks=3)
    assert plain.surface is None and plain.psr is None and plain.peak_values is None and plain.peak_positions is None
    np.testing.assert_array_equal(short.index, plain.index)
    assert_same_bits(short.score, plain.score, "retrieve: scores")
    for name in ("variant", "peak_yx", "offset"):
        np.testing.assert_array_equal(getattr(short, name), getattr(plain, name))
    assert short.surface.shape == (nq, k) and short.surface.dtype == object
    assert short.psr.shape == (nq, k) and short.psr.dtype == np.float32
    assert short.peak_values.shape == (nq, k, 3) and short.peak_values.dtype == np.float32
    assert short.peak_positions.shape == (nq, k, 3, 2) and short.peak_positions.dtype == np.int32
    empty = short.index < 0
    assert empty[:, -1].all() and not empty[:, :-1].any()
    assert all(s is None for s in short.surface[empty]) and not short.psr[empty].any() and not short.peak_values[empty].any()
    assert (short.peak_positions[empty] == -1).all()
    th, tw = h - 2 * CROP, w - 2 * CROP
    worst = 0.0
    for qi in range(nq):
        for p in range(ng):
            gi = int(short.index[qi, p])
            surf = short.surface[qi, p]
            assert surf.shape == (th, tw) and short.variant[qi, p] == 0
            worst = max(worst, float(np.abs(surf - oracle_surface(q[qi], g[gi])).max()))
            v, yx, psr = run_surface_peaks(scorer, surf[None], 3, th // 2, tw // 2)
            assert_same_bits(short.peak_values[qi, p], v[0], "retrieve: peak values")
            np.testing.assert_array_equal(short.peak_positions[qi, p], similarity._unpack_yx(yx[0]))
            assert_same_bits(short.psr[qi, p], psr[0], "retrieve: psr")
            if gi == m[qi]:  # the planted print
                assert_same_bits(short.peak_values[qi, p, 0], short.score[qi, p], "retrieve: the planted print's first peak")
                np.testing.assert_array_equal(short.peak_positions[qi, p, 0], short.peak_yx[qi, p])
    print(f"\n[retrieve surfaces] {case}: max |surface - oracle mean map| = {worst:.2e}, bound {TIGHT:.0e}")
    assert worst <= TIGHT
    for bad in (0, 9, 2.5, True):
        try:
            similarity.retrieve(q, g, sc_cases._cfg(), k=2, scorer=scorer, surfaces=True, peaks=bad)
        except ValueError as e:
            assert "peaks" in str(e)
        else:
            raise AssertionError(f"peaks = {bad!r} was accepted")


def check_retrieve_surfaces_variants(scorer):
    """With rotations the surface is the winning variant's map: its maximum is the score, at ``peak_yx``; FeatureSets on both
    sides (``retrieve_resident``) and the cascade's shortlist give the same fields."""
    from shoeprint_image_retrieval_amd.features import FeatureSet

    q, g = lc.ragged_sets()
    cfg = sc_cases._cfg(rot=[180], sc=[1.04])
    plain = similarity.retrieve(q, g, cfg, k=3, scorer=scorer)
    short = similarity.retrieve(q, g, cfg, k=3, scorer=scorer, surfaces=True)
    np.testing.assert_array_equal(short.index, plain.index)
    assert_same_bits(short.score, plain.score, "retrieve with variants: scores")
    for name in ("variant", "peak_yx", "offset"):
        np.testing.assert_array_equal(getattr(short, name), getattr(plain, name))
    assert short.peak_values.shape == (len(q), 3, 2)
    assert len(set(short.variant.ravel().tolist())) >= 2  # (more than one variant wins somewhere)
    for qi in range(len(q)):
        for p in range(3):
            surf = short.surface[qi, p]
            assert_same_bits(surf.max(), short.score[qi, p], "retrieve with variants: the surface's maximum")
            assert_same_bits(surf[tuple(short.peak_yx[qi, p])], surf.max(), "retrieve with variants: the surface at the peak")
            assert_same_bits(short.peak_values[qi, p, 0], short.score[qi, p], "retrieve with variants: the first peak")
    res = similarity.retrieve(FeatureSet.from_host(scorer.dev, q), FeatureSet.from_host(scorer.dev, g), cfg, k=3, scorer=scorer,
                              surfaces=True)
    np.testing.assert_array_equal(res.index, short.index)
    assert_same_bits(res.psr, short.psr, "retrieve_resident: psr")
    assert_same_bits(res.peak_values, short.peak_values, "retrieve_resident: peak values")
    np.testing.assert_array_equal(res.peak_positions, short.peak_positions)
    for a, b in zip(res.surface.ravel(), short.surface.ravel()):
        assert_same_bits(a, b, "retrieve_resident: surfaces")
    # the cascade: the located layer's surfaces
    layers, match, _ = lc.cascade_layers()
    cas = similarity.retrieve_cascade(layers, lc._cfg(), 4, scorer=scorer)
    two = cas.shortlist(2, surfaces=True)
    np.testing.assert_array_equal(two.index, cas.shortlist(2).index)
    assert two.surface.shape == (lc.CASCADE_Q, 2) and cas.shortlist(2).surface is None
    for qi in range(lc.CASCADE_Q):
        for p in range(2):
            if two.variant[qi, p] >= 0:
                assert two.surface[qi, p].shape == (60, 28)
                np.testing.assert_array_equal(two.peak_positions[qi, p, 0], two.peak_yx[qi, p])
