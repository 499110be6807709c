"""Checks of spr_ncc_score_list - the pair kernels over a list of (query, gallery) pairs - and of what stands on it
(NccScorer.score_pairs, similarity.retrieve_cascade), shared by the CPU-emulation runner (test_emu_score_list.py, not gpu) and
the MI355X runner (test_gpu_score_list.py, gpu).

The contract (include/shoeprint_mi355x.h) is exact: entry p of a list holds bit for bit what spr_ncc_score_peaks stores in cell
pairs[p] of the dense matrices.  So the list form is compared with the dense form on the same prepared buffers without any
tolerance, every output between guard bands; score_pairs with the cells of score_matrix_located, and the cascade with the full
fused matrix, likewise.  One check compares with the float64 oracle instead of a sibling: within parity_cases.TIGHT, the bound
shortlist_cases.check_locate_planted holds the dense path to on the same data sets.
"""

import functools
from typing import NamedTuple

import numpy as np
import pytest

import shortlist_cases as sc_cases
from oracle import ncc_oracle as oracle
from parity_cases import BIG_SHAPE_CASES, SHAPE_CASES, TIGHT
from shoeprint_image_retrieval_amd import _lib, similarity, synth

GUARD = 64
POISON_F, POISON_I = 777.0, -777
START = (0.0, -1, -1)              # what a caller starts scores / peak_yx / peak_tag at
SENTINEL = (-5.5, -1234, -4321)    # what the outputs of entries that must stay untouched are filled with


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case(NamedTuple):
    method: str
    storage: str
    shape: tuple   # (C, qh, qw, gh, gw)
    grid: tuple    # spr_ncc_plan_fft_size of the plan: (0, 0) for the direct method

    @property
    def id(self):
        return f"{self.method}-{self.storage}-" + "x".join(str(v) for v in self.shape)


# Every workgroup shape of the list form once.  The grid a case runs on is asserted, so a case cannot move to another instance
# unnoticed: 32x16 .. 64x32 one wave per pair, 64x64 and 128x64 four waves, 96x48 three, 192x96 six (two pairs per workgroup;
# 2 queries x 3 items and 3 x 3 items give odd counts that leave a half idle), 256x128 eight.
CASES = [Case("fft", "float32", s, g) for s, g in zip(SHAPE_CASES, [
    (48, 24), (64, 64), (48, 24), (64, 64), (64, 64), (64, 64), (32, 16), (96, 48), (96, 48), (48, 24), (64, 32)])] + [
    Case("fft", "float32", BIG_SHAPE_CASES[0], (192, 96)), Case("fft", "float32", BIG_SHAPE_CASES[3], (192, 96)),
    Case("fft_pow2", "float32", (2, 128, 64, 128, 64), (256, 128)),
    Case("direct", "float32", SHAPE_CASES[0], (0, 0)), Case("direct", "float32", SHAPE_CASES[2], (0, 0)),
    Case("direct", "float32", SHAPE_CASES[4], (0, 0)),
    Case("fft", "float16", SHAPE_CASES[6], (32, 16)), Case("fft", "bfloat16", SHAPE_CASES[9], (48, 24)),
    # the grids no case above lands on
    Case("fft", "float32", (2, 20, 20, 20, 20), (32, 32)), Case("fft", "float32", (2, 80, 40, 80, 40), (128, 64)),
    Case("fft", "float32", (1, 70, 70, 70, 70), (128, 128)),
]
SMALL = Case("fft", "float32", SHAPE_CASES[6], (32, 16))  # the cheapest plan: accumulation, slicing and argument checks
NQ = NG = 3


class Prepared(NamedTuple):
    scorer: object
    plan: object
    pq: object
    nq: int
    pg: object
    ng: int


def prepare(make_scorer, case, nq=NQ, ng=NG, seed=0):
    """A scorer, the case's plan and ``nq`` x ``ng`` seeded ``rng.random`` maps, prepared."""
    c, qh, qw, gh, gw = case.shape
    rng = np.random.default_rng(1000 * seed + sum(case.shape))
    q = rng.random((nq, c, qh, qw), dtype=np.float32)
    g = rng.random((ng, c, gh, gw), dtype=np.float32)
    sc = make_scorer(case.method, storage=case.storage)
    dev = sc.dev
    plan = sc.plan(c, (qh, qw), (gh, gw), dtype=case.storage)
    assert plan.fft_size == case.grid, (case.id, plan.fft_size)
    assert plan.has_list and sc.lib.spr_ncc_plan_has_list(plan.handle) == 1
    pq = sc.prepare_queries(plan, dev.astype_storage(dev.to_device(q), case.storage))
    pg = sc.prepare_gallery(plan, dev.astype_storage(dev.to_device(g), case.storage))
    return Prepared(sc, plan, pq, nq, pg, ng)


class ListOutputs:
    """scores / peak_yx / peak_tag of one list between guard bands of GUARD poisoned elements, started at ``start``."""

    def __init__(self, scorer, n, start=START, with_tags=True):
        self.sc, self.n = scorer, n
        dev = scorer.dev

        def guarded(value, poison, dtype):
            host = np.full(n + 2 * GUARD, poison, dtype=dtype)
            host[GUARD:GUARD + n] = value
            return dev.to_device(host)

        self.scores = guarded(start[0], POISON_F, np.float32)
        self.yx = guarded(start[1], POISON_I, np.int32)
        self.tags = guarded(start[2], POISON_I, np.int32) if with_tags else None

    def score(self, p: Prepared, pairs_dev, n_pairs, accumulate=False, tag=0):
        dev, lib = self.sc.dev, self.sc.lib
        return lib.spr_ncc_score_list(p.plan.handle, dev.ptr(p.pq), p.nq, dev.ptr(p.pg), p.ng, dev.ptr(pairs_dev), n_pairs,
                                      dev.ptr(self.scores) + 4 * GUARD, dev.ptr(self.yx) + 4 * GUARD,
                                      None if self.tags is None else dev.ptr(self.tags) + 4 * GUARD,
                                      1 if accumulate else 0, tag, dev.stream())

    def read(self):
        """(scores, packed positions, tags or None); the guard bands must be as they were."""
        out = []
        for buf, poison in ((self.scores, POISON_F), (self.yx, POISON_I), (self.tags, POISON_I)):
            if buf is None:
                out.append(None)
                continue
            host = np.array(self.sc.dev.to_host(buf))
            assert (host[:GUARD] == poison).all() and (host[GUARD + self.n:] == poison).all(), "written outside the list's outputs"
            out.append(host[GUARD:GUARD + self.n])
        return out


def run_list(p: Prepared, pairs, start=START, with_tags=True, tag=0):
    """One non-accumulating spr_ncc_score_list call over ``pairs`` (host [n, 2])."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    out = ListOutputs(p.scorer, len(pairs), start, with_tags)
    p.scorer.lib.check(out.score(p, p.scorer.dev.to_device(pairs), len(pairs), tag=tag))
    return out.read()


def dense(p: Prepared, with_tags=True, tag=0):
    """The dense form on the same prepared buffers: host (scores, packed positions, tags or None), each [nq, ng]."""
    sc, dev = p.scorer, p.scorer.dev
    s = dev.zeros((p.nq, p.ng), np.float32)
    yx = dev.to_device(np.full((p.nq, p.ng), -1, np.int32))
    tags = dev.to_device(np.full((p.nq, p.ng), -1, np.int32)) if with_tags else None
    sc.score_prepared(p.plan, p.pq, p.nq, p.pg, p.ng, s, p.ng, 0, peaks=yx, tags=tags, tag=tag)
    return np.array(dev.to_host(s)), np.array(dev.to_host(yx)), None if tags is None else np.array(dev.to_host(tags))


def assert_entries(got, want, pairs, what):
    """``got`` (list outputs) against the cells ``pairs`` of ``want`` (dense matrices), bit for bit."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    for k, name in enumerate(("scores", "peak_yx", "peak_tag")):
        if got[k] is None:
            assert want[k] is None
            continue
        cells = want[k][pairs[:, 0], pairs[:, 1]]
        if k == 0:
            np.testing.assert_array_equal(bits(got[k]), bits(cells), err_msg=f"{what}: {name}")
        else:
            np.testing.assert_array_equal(got[k], cells, err_msg=f"{what}: {name}")


def case_lists(nq, ng, seed):
    """The lists every instance is given: all pairs in a seeded permutation, a single pair, an odd count with repeats."""
    rng = np.random.default_rng(seed)
    every = np.array([(q, g) for q in range(nq) for g in range(ng)], dtype=np.int32)
    return {"permutation": every[rng.permutation(len(every))], "single": every[[len(every) // 2]],
            "odd with repeats": every[rng.integers(0, len(every), 7)]}


def check_instance(make_scorer, case):
    """The list form of one instance against the dense form on the same prepared buffers."""
    nq, ng = (2, 3) if case.shape == BIG_SHAPE_CASES[3] else (NQ, NG)
    p = prepare(make_scorer, case, nq, ng)
    want = dense(p, tag=3)
    assert (want[0] > 0).any()  # (random positive maps: the scores are not all floored away)
    for name, pairs in case_lists(nq, ng, sum(case.shape)).items():
        assert_entries(run_list(p, pairs, tag=3), want, pairs, f"{case.id}, {name}")
    # without a tag vector
    pairs = case_lists(nq, ng, 5)["odd with repeats"]
    assert_entries(run_list(p, pairs, with_tags=False, tag=3), (want[0], want[1], None), pairs, f"{case.id}, no tags")
    # entries that name no item, interleaved: their outputs keep what they held, their neighbours are right
    bad = [(-1, 0), (nq, 0), (0, -1), (0, ng)]
    valid = case_lists(nq, ng, 6)["permutation"][:5]
    mixed = np.array([bad[0], valid[0], bad[1], bad[2], valid[1], valid[2], bad[3], valid[3], valid[4]], dtype=np.int32)
    is_bad = np.array([tuple(e) in bad for e in mixed.tolist()])
    got = run_list(p, mixed, start=SENTINEL, tag=3)
    for k in range(3):
        assert (got[k][is_bad] == SENTINEL[k]).all(), f"{case.id}: output {k} of a skipped entry was written"
    assert_entries([v[~is_bad] for v in got], want, mixed[~is_bad], f"{case.id}, neighbours of skipped entries")
    # a list of skipped entries only (a six-wave workgroup both of whose pairs are skipped returns)
    got = run_list(p, np.array(bad, dtype=np.int32), start=SENTINEL)
    for k in range(3):
        assert (got[k] == SENTINEL[k]).all()
    p.scorer.close()


def check_accumulate(make_scorer, case=SMALL):
    """Three query batches as variants through accumulate_max, tags in the order 2, 0, 1, on outputs started at 0 / -1 / -1:
    the dense form driven the same way, with the tag vector and without it."""
    c, qh, qw, gh, gw = case.shape
    p = prepare(make_scorer, case)
    sc, dev = p.scorer, p.scorer.dev
    rng = np.random.default_rng(77)
    batches = [p.pq] + [sc.prepare_queries(p.plan, dev.astype_storage(dev.to_device(
        rng.random((p.nq, c, qh, qw), dtype=np.float32)), case.storage)) for _ in range(2)]
    batches.append(p.pq)  # (the first batch once more under a lower tag: equal scores, the lower tag must win)
    order = [2, 0, 1, 1]
    pairs = case_lists(p.nq, p.ng, 9)["permutation"]
    pairs_dev = dev.to_device(np.ascontiguousarray(pairs, dtype=np.int32))
    for with_tags in (True, False):
        s = dev.zeros((p.nq, p.ng), np.float32)
        yx = dev.to_device(np.full((p.nq, p.ng), -1, np.int32))
        tags = dev.to_device(np.full((p.nq, p.ng), -1, np.int32)) if with_tags else None
        out = ListOutputs(sc, len(pairs), START, with_tags)
        for pq, tag in zip(batches, order):
            sc.score_prepared(p.plan, pq, p.nq, p.pg, p.ng, s, p.ng, 0, accumulate_max=True, peaks=yx, tags=tags, tag=tag)
            sc.lib.check(out.score(p._replace(pq=pq), pairs_dev, len(pairs), accumulate=True, tag=tag))
        want = (np.array(dev.to_host(s)), np.array(dev.to_host(yx)), None if tags is None else np.array(dev.to_host(tags)))
        if with_tags:
            assert len(set(want[2].ravel().tolist()) - {-1}) >= 2  # (more than one batch wins somewhere)
        assert_entries(out.read(), want, pairs, f"accumulate, tags {with_tags}")
    sc.close()


def check_slicing(make_scorer, monkeypatch, case=SMALL):
    """SPR_NCC_MAX_TILES=1 (read at every launch): a list of several launches gives the bits of one launch."""
    p = prepare(make_scorer, case)
    rng = np.random.default_rng(4)
    every = np.array([(q, g) for q in range(p.nq) for g in range(p.ng)], dtype=np.int32)
    n = {"direct": 5, "fft": 2 * 256 + 37, "fft_pow2": 2 * 256 + 37}[case.method]  # (one tile: 256 pairs, direct: one)
    if case.grid == (192, 96):
        n = 256 + 5
    pairs = every[rng.integers(0, len(every), n)]
    pairs[n // 2] = (-1, 0)
    want = run_list(p, pairs, start=SENTINEL)
    monkeypatch.setenv("SPR_NCC_MAX_TILES", "1")
    got = run_list(p, pairs, start=SENTINEL)
    monkeypatch.delenv("SPR_NCC_MAX_TILES")
    ref = dense(p)
    ok = np.arange(n) != n // 2
    assert_entries([v[ok] for v in got], ref, pairs[ok], f"{case.id}, sliced")
    for k in range(3):
        np.testing.assert_array_equal(got[k].view(np.int32), want[k].view(np.int32))
        assert got[k][n // 2] == SENTINEL[k]
    p.scorer.close()


def check_arguments(make_scorer, monkeypatch):
    """Error codes of the entry point; plans without the form."""
    p = prepare(make_scorer, SMALL)
    sc, dev, lib = p.scorer, p.scorer.dev, p.scorer.lib
    pairs = dev.to_device(np.array([(0, 0), (1, 2)], dtype=np.int32))

    def call(prep=p, out=None, **kw):
        out = out or ListOutputs(sc, 2, SENTINEL)
        a = {"plan": prep.plan.handle, "pq": dev.ptr(prep.pq), "nq": prep.nq, "pg": dev.ptr(prep.pg), "ng": prep.ng,
             "pairs": dev.ptr(pairs), "n": 2, "scores": dev.ptr(out.scores) + 4 * GUARD, "yx": dev.ptr(out.yx) + 4 * GUARD,
             "tags": dev.ptr(out.tags) + 4 * GUARD}
        a.update(kw)
        rc = lib.spr_ncc_score_list(a["plan"], a["pq"], a["nq"], a["pg"], a["ng"], a["pairs"], a["n"], a["scores"], a["yx"],
                                    a["tags"], 0, 0, dev.stream())
        return rc, out.read()

    def untouched(got):
        return all((got[k] == SENTINEL[k]).all() for k in range(3))

    rc, got = call()
    assert rc == _lib.SPR_OK and not untouched(got)
    rc, got = call(tags=None)
    assert rc == _lib.SPR_OK and (got[2] == SENTINEL[2]).all()
    for bad in ({"plan": None}, {"pq": None}, {"pg": None}, {"pairs": None}, {"scores": None}, {"yx": None}, {"nq": -1},
                {"ng": -1}, {"n": -1}):
        rc, got = call(**bad)
        assert rc == _lib.SPR_ERR_ARG and untouched(got), bad
    rc, got = call(n=0)
    assert rc == _lib.SPR_OK and untouched(got)
    assert lib.spr_ncc_score_list(p.plan.handle, None, 0, None, 0, None, 0, None, None, None, 0, 0, dev.stream()) == _lib.SPR_OK
    assert lib.spr_ncc_plan_has_list(None) == 0
    sc.close()
    # plans without the form: the matrix-core method, and the workspace instance of the FFT method
    c, h, w = 4, 32, 16
    rng = np.random.default_rng(8)
    q, g = rng.random((NQ, c, h, w), dtype=np.float32), rng.random((NG, c, h, w), dtype=np.float32)
    monkeypatch.setenv("SPR_NCC_FORCE_BIG", "1")
    big_sc = make_scorer("fft")
    big_plan = big_sc.plan(c, (h, w), (h, w))
    monkeypatch.delenv("SPR_NCC_FORCE_BIG")
    mfma_sc = make_scorer("mfma", storage="bfloat16")
    mfma_plan = mfma_sc.plan(c, (h, w), (h, w), dtype="bfloat16")
    assert big_plan.method == _lib.NCC_FFT and mfma_plan.method == _lib.NCC_MFMA  # (workspace mode: whatever the grid)
    for s, plan, storage in ((big_sc, big_plan, "float32"), (mfma_sc, mfma_plan, "bfloat16")):
        assert not plan.has_list and lib.spr_ncc_plan_has_list(plan.handle) == 0
        pq = s.prepare_queries(plan, dev.astype_storage(dev.to_device(q), storage))
        pg = s.prepare_gallery(plan, dev.astype_storage(dev.to_device(g), storage))
        rc, got = call(prep=Prepared(s, plan, pq, NQ, pg, NG))
        assert rc == _lib.SPR_ERR_UNSUPPORTED and untouched(got)
        s.close()


# ------------------------------------------------------------------------------------------------ against the oracle
def check_planted_against_oracle(scorer, case):
    """score_pairs of all pairs of a planted data set within TIGHT of max(0, oracle.get_similarity)."""
    seed, nq, ng, c, h, w = case
    q, g, m, sim, peak, lead = sc_cases.planted_reference(case, scorer.storage)
    pairs = [(qi, gi) for qi in range(nq) for gi in range(ng)]
    scores, variant, yx, t_hw = scorer.score_pairs(q, g, pairs)
    want = np.maximum(sim, 0.0).ravel()
    print(f"\n[score_pairs] {case}: max |score - max(0, oracle)| = {np.abs(scores - want).max():.2e}, bound {TIGHT:.0e}")
    np.testing.assert_allclose(scores, want, atol=TIGHT, rtol=0)
    for qi in range(nq):  # the planted shift of every true match
        dy, dx = synth.query_shift(seed, qi)
        assert tuple(yx[qi * ng + m[qi]]) == ((h - 4) // 2 + dy, (w - 4) // 2 + dx)


# ------------------------------------------------------------------------------------------------ score_pairs
ROT, SCALES = [3, 180], [1.04]


@functools.lru_cache(maxsize=None)
def ragged_sets():
    """Two query shapes, two gallery shapes (read-only)."""
    q = [synth.query_features(1236, i, i, 5, hh, ww) for i, (hh, ww) in enumerate([(18, 12), (16, 14), (18, 12)])]
    g = [synth.gallery_features(1236, i, 5, hh, ww) for i, (hh, ww) in enumerate([(18, 12), (20, 12), (18, 12), (20, 12), (18, 12)])]
    for a in q + g:
        a.setflags(write=False)
    return q, g


def check_score_pairs(scorer, q=None, g=None, pairs=None, rot=ROT, sc=SCALES, sides=None):
    """``score_pairs`` against the cells of ``score_matrix_located``, bit for bit; ``sides`` = what is handed to score_pairs
    (default: the host lists)."""
    if q is None:
        q, g = ragged_sets()
    nq, ng = len(q), len(g)
    if pairs is None:
        rng = np.random.default_rng(3)
        every = np.array([(a, b) for a in range(nq) for b in range(ng)])
        pairs = np.concatenate([every[rng.permutation(len(every))], every[:4]])  # every pair, some twice
    pairs = np.asarray(pairs).reshape(-1, 2)
    scores, variant, yx, t_hw_all = scorer._score_matrix_located(q, g, rot, sc)
    got = scorer.score_pairs(*(sides or (q, g)), pairs, rotations=rot, scales=sc)
    assert [a.dtype for a in got] == [np.float32, np.int32, np.int32, np.int32]
    assert got[0].shape == got[1].shape == (len(pairs),) and got[2].shape == got[3].shape == (len(pairs), 2)
    qs, gs = pairs[:, 0], pairs[:, 1]
    np.testing.assert_array_equal(bits(got[0]), bits(scores[qs, gs]))
    np.testing.assert_array_equal(got[1], variant[qs, gs])
    np.testing.assert_array_equal(got[2], yx[qs, gs])
    hit = variant[qs, gs] >= 0
    assert hit.any() and ((scores[qs, gs] > 0) == hit).all()
    np.testing.assert_array_equal(got[3][hit], t_hw_all[qs[hit], variant[qs, gs][hit]])
    assert not got[3][~hit].any()
    return got


def check_score_pairs_surface(scorer):
    q, g = ragged_sets()
    with pytest.raises(IndexError):
        scorer.score_pairs(q, g, [(0, 0), (len(q), 0)])
    with pytest.raises(IndexError):
        scorer.score_pairs(q, g, [(0, -1)])
    empty = scorer.score_pairs(q, g, [], rotations=ROT, scales=SCALES)
    assert [a.shape for a in empty] == [(0,), (0,), (0, 2), (0, 2)]
    assert [a.dtype for a in empty] == [np.float32, np.int32, np.int32, np.int32]
    # a few pairs of one shape class: the other classes are not visited (their plans are never made)
    check_score_pairs(scorer, pairs=[(1, 1), (1, 3)])


# ------------------------------------------------------------------------------------------------ the cascade
CASCADE_SEED, CASCADE_Q, CASCADE_G = 31, 5, 12


def _cfg(rot=None, sc=None):
    return {"comparison": {"n_processes": 1, "rotations": rot, "scales": sc}}


@functools.lru_cache(maxsize=None)
def cascade_layers():
    """Two "layers" of the same items: fine [4, 64, 32] and coarse [6, 32, 16], same seed, same matches (read-only).  With
    noise 12 the coarse oracle ranks of the matches are 1, 5, 6, 4, 1."""
    fine = synth.dataset(CASCADE_SEED, CASCADE_Q, CASCADE_G, 4, 64, 32, signal=1, noise=12)
    coarse = synth.dataset(CASCADE_SEED, CASCADE_Q, CASCADE_G, 6, 32, 16, signal=1, noise=12)
    assert list(fine[2]) == list(coarse[2])
    coarse_ranks = oracle.compare_maps(coarse[0], coarse[1], coarse[2], _cfg())
    return [(fine[0], fine[1]), (coarse[0], coarse[1])], [int(v) for v in fine[2]], [int(r) for r in coarse_ranks]


def check_cascade_full_depth(scorer, depth):
    """Identity 1: with depth >= G the cascade is the ranking of the full fused matrix."""
    layers, match, _ = cascade_layers()
    dev = scorer.dev
    full = scorer.multi_layer_score_matrix_device(layers)
    want_ranks = scorer.ranks_of_device(full, match)
    full_host = np.array(dev.to_host(full))
    want_s, want_i = sc_cases.expected_topk(full_host, depth)
    top_s, top_i = scorer.topk_device(full, depth)
    np.testing.assert_array_equal(np.array(dev.to_host(top_i)), want_i)  # (the device top-G of the full matrix is that order)
    c = similarity.retrieve_cascade(layers, _cfg(), depth, scorer=scorer)
    assert c.index.shape == c.score.shape == c.variant.shape == (CASCADE_Q, depth) and c.peak_yx.shape == c.offset.shape == (CASCADE_Q, depth, 2)
    assert c.index.dtype == np.int32 and c.score.dtype == np.float32
    np.testing.assert_array_equal(c.index, want_i)
    np.testing.assert_array_equal(bits(c.score), bits(want_s))
    np.testing.assert_array_equal(bits(c.score), bits(np.array(dev.to_host(top_s))))
    np.testing.assert_array_equal(c.ranks(match), want_ranks)
    np.testing.assert_array_equal(bits(np.array(dev.to_host(c.coarse))), bits(scorer.score_matrix(*layers[1])))


def check_cascade_short_depth(scorer, depth=3):
    """Identity 2: with depth < G every candidate's fused score is its cell of the full fused matrix, the candidates are the
    top-M of the coarse matrix, and a query whose match is no candidate has its coarse rank."""
    layers, match, oracle_ranks = cascade_layers()
    inside = [r <= depth for r in oracle_ranks]
    assert any(inside) and not all(inside), oracle_ranks  # (from the oracle: both kinds of query occur)
    dev = scorer.dev
    full = np.array(dev.to_host(scorer.multi_layer_score_matrix_device(layers)))
    coarse = scorer.score_matrix(*layers[1])
    coarse_ranks = scorer.ranks(coarse, match)
    np.testing.assert_array_equal(coarse_ranks, oracle_ranks)
    _, cand = sc_cases.expected_topk(coarse, depth)
    c = similarity.retrieve_cascade(layers, _cfg(), depth, scorer=scorer)
    assert c.index.shape == (CASCADE_Q, depth)
    for q in range(CASCADE_Q):
        assert sorted(c.index[q]) == sorted(cand[q])
        np.testing.assert_array_equal(bits(c.score[q]), bits(full[q, c.index[q]]))
    _, want_i = sc_cases.expected_topk(full, CASCADE_G)
    for q in range(CASCADE_Q):  # re-ranked in the ranker's order: the candidates in the order the full ranking has them
        order = [g for g in want_i[q] if g in set(cand[q].tolist())]
        assert c.index[q].tolist() == order
    ranks = c.ranks(match)
    for q in range(CASCADE_Q):
        if match[q] in c.index[q]:
            assert ranks[q] == c.index[q].tolist().index(match[q]) + 1 <= depth and inside[q]
        else:
            assert ranks[q] == coarse_ranks[q] > depth and not inside[q]
    return c


def check_cascade_located(scorer):
    """The located fields are score_pairs of the located layer, laid out like Shortlist's; the shortlist view."""
    layers, match, _ = cascade_layers()
    for locate_layer, rot in ((None, None), (1, None), (0, [180])):
        c = similarity.retrieve_cascade(layers, _cfg(rot=rot), 4, locate_layer=locate_layer, scorer=scorer)
        qs, ps = np.nonzero(c.index >= 0)
        assert len(qs) == CASCADE_Q * 4
        pairs = np.stack([qs, c.index[qs, ps]], axis=1)
        _, variant, yx, t_hw = scorer.score_pairs(*layers[locate_layer or 0], pairs, rotations=rot)
        assert (variant >= 0).all()
        np.testing.assert_array_equal(c.variant[qs, ps], variant)
        np.testing.assert_array_equal(c.peak_yx[qs, ps], yx)
        np.testing.assert_array_equal(c.offset[qs, ps], yx - t_hw // 2)
        short = c.shortlist(2)
        assert isinstance(short, similarity.Shortlist) and short.index.shape == (CASCADE_Q, 2) and short.offset.shape == (CASCADE_Q, 2, 2)
        np.testing.assert_array_equal(short.index, c.index[:, :2])
        np.testing.assert_array_equal(bits(short.score), bits(c.score[:, :2]))
        np.testing.assert_array_equal(short.offset, c.offset[:, :2])
    # the true match of a query whose match is a candidate lies where it was planted, on the fine layer
    c = similarity.retrieve_cascade(layers, _cfg(), 4, scorer=scorer)
    q = 0
    p = c.index[q].tolist().index(match[q])
    assert tuple(c.offset[q, p]) == synth.query_shift(CASCADE_SEED, q)


def check_cascade_errors(scorer):
    layers, match, _ = cascade_layers()
    for depth in (0, 257, -1, 2.5):
        with pytest.raises(ValueError, match="depth"):
            similarity.retrieve_cascade(layers, _cfg(), depth, scorer=scorer)
    with pytest.raises(ValueError, match="two feature layers"):
        similarity.retrieve_cascade(layers[:1], _cfg(), 3, scorer=scorer)
    with pytest.raises(ValueError, match="two feature layers"):
        similarity.retrieve_cascade([], _cfg(), 3, scorer=scorer)
    with pytest.raises(ValueError, match="coarse"):
        similarity.retrieve_cascade(layers, _cfg(), 3, coarse=2, scorer=scorer)
    c = similarity.retrieve_cascade(layers, _cfg(), 3, scorer=scorer)
    with pytest.raises(IndexError):
        c.ranks([0, 2, CASCADE_G, 6, 8])
    with pytest.raises(ValueError):
        c.shortlist(4)
