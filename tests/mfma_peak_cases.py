"""Checks of the matrix-core pair kernels' peak form (csrc/ncc_mfma_peaks.hip: spr_ncc_score_peaks on a plan of "mfma" or
"mfma_f32" that was asked with spr_ncc_plan_enable_peaks) and of its host mirror (NccScorer(matrix_core_peaks=True),
[mi355x] matrix_core_peaks), shared by the CPU-emulation runner (test_emu_mfma_peaks.py, not gpu) and the MI355X runner
(test_gpu_mfma_peaks.py, gpu).  Inputs, oracles and rules are those of mfma_map_cases.py, peak_cases.py and shortlist_cases.py.

The contract (include/shoeprint_mi355x.h) is exact: scores bit for bit those of spr_ncc_score (peak_cases.score_peaks checks
that on every call made here), the position the first maximum of the kernel's float32 channel sums in row-major order, and
never a position outside the ih x iw map - the frame of positions of both instances is 28 x 12 whatever the map
(assert_inside, applied to every position this file reads).

1. check_default_refuses / check_opt_in: the form is opt-in per plan.
2. check_planted: mfma_map_cases.PEAK_CASES - 67 templates (a full 64-query block and a block of three) against one
   single-channel item per planted position, every good matched pair names the planted pixel.
3. check_ties: twelve (nine) exactly equal maxima in different tiles and tile groups; the first in row-major order is named.
4. check_instance: one multi-channel pair with dead channels per case of MAP_CASES + WIDE_CASES.
5. check_accumulate_rule / check_edges: the rules of the peak_cases helpers of those names on the storage type of the plan.
6. Host level: score_matrix_located, retrieve, locate and the call counts with the flag on and off, the config key.

Bounds: positions are compared exactly where the float64 oracle on the values as stored names the pixel beyond doubt (planted
peaks with mfma_map_cases.MARGIN, leads above POSITION_LEAD); scores against the oracle within TIGHT for the 16-bit forms and
within the contract TOL for "mfma_f32" (mfma_map_cases.py says why its scheme passes TIGHT on some shapes).
"""

import functools

import numpy as np

import mfma_map_cases as mm
import ncc_map_cases as mc
import peak_cases as pc
import shortlist_cases as sc_cases
from oracle import ncc_oracle as oracle
from parity_cases import TIGHT, TOL
from shortlist_cases import POSITION_LEAD
from shoeprint_image_retrieval_amd import _lib, similarity, synth

# (method, storage) of the host-level checks; "auto" takes bfloat16 maps inside the frame to the matrix-core method
HOST_SCORERS = [("mfma", "bfloat16"), ("mfma_f32", "float32"), ("auto", "bfloat16")]
PLANTED = sc_cases.PLANTED_CASES[0]  # 4 x 6 items, 5 channels, 20 x 14 (cropped 16 x 10: the general instance)


def score_bound(form_or_storage):
    return TOL if form_or_storage in ("f32", "float32") else TIGHT


def assert_inside(yx, ih, iw, label):
    """No position outside the map: yx [..., 2] holds (-1, -1) or a pixel of the ih x iw map."""
    yx = np.asarray(yx).reshape(-1, 2)
    none = (yx == -1).all(axis=1)
    ok = none | ((yx[:, 0] >= 0) & (yx[:, 0] < ih) & (yx[:, 1] >= 0) & (yx[:, 1] < iw))
    assert ok.all(), f"{label}: positions outside the {ih} x {iw} map: {sorted({tuple(v) for v in yx[~ok]})[:20]}"


def peaks_on(make_scorer):
    """make_scorer(method) -> a crop-0 scorer whose plans are asked for the peak form."""
    return lambda method: make_scorer(method, crop=0, matrix_core_peaks=True)


# ------------------------------------------------------------------------------------------------ 1. opt-in
def _small_pair(sc, plan, dtype):
    q = np.random.default_rng(3).standard_normal((2, 1, 9, 7), dtype=np.float32)
    g = np.random.default_rng(4).standard_normal((3, 1, 28, 12), dtype=np.float32)
    return pc.prepare(sc, plan, mm._to_storage(q, dtype)[0], mm._to_storage(g, dtype)[0])


def check_default_refuses(make_scorer):
    """A matrix-core plan that was not asked answers as before the form existed: has_peaks 0, SPR_ERR_UNSUPPORTED, no launch."""
    for method, dtype in (("mfma", "bfloat16"), ("mfma_f32", "float32")):
        sc = make_scorer(method, crop=0)
        plan = sc.plan(1, (9, 7), (28, 12), dtype=mm._NP_DTYPE[dtype])
        assert plan.method == similarity._METHODS[method]
        assert not plan.has_peaks and sc.lib.spr_ncc_plan_has_peaks(plan.handle) == 0
        pq, pg = _small_pair(sc, plan, dtype)
        m = pc.PeakMatrices(sc, 2, 3)
        assert m.score(plan, pq, pg) == _lib.SPR_ERR_UNSUPPORTED
        s, packed, tags = m.read()
        assert not s.any() and (packed == -1).all() and (tags == -1).all()
        sc.close()


def check_opt_in(make_scorer):
    for method, dtype in (("mfma", "bfloat16"), ("mfma_f32", "float32")):
        sc = make_scorer(method, crop=0)
        lib = sc.lib
        plan = sc.plan(1, (9, 7), (28, 12), dtype=mm._NP_DTYPE[dtype])
        sizes = (plan.query_item_bytes, plan.gallery_item_bytes)
        assert lib.spr_ncc_plan_has_peaks(plan.handle) == 0
        assert lib.spr_ncc_plan_enable_peaks(plan.handle) == 0
        assert lib.spr_ncc_plan_has_peaks(plan.handle) == 1 and lib.spr_ncc_plan_method(plan.handle) == plan.method
        assert lib.spr_ncc_plan_enable_peaks(plan.handle) == 0 and lib.spr_ncc_plan_has_peaks(plan.handle) == 1  # asked twice
        assert (lib.spr_ncc_query_bytes(plan.handle, 1), lib.spr_ncc_gallery_bytes(plan.handle, 1)) == sizes
        pq, pg = _small_pair(sc, plan, dtype)
        scores, yx, tags = pc.score_peaks(sc, plan, pq, 2, pg, 3, tag=6)  # (bit-equal to spr_ncc_score inside)
        assert_inside(yx, 28, 12, method)
        sc.close()
        on = make_scorer(method, crop=0, matrix_core_peaks=True)
        assert on.matrix_core_peaks and on.plan(1, (9, 7), (28, 12), dtype=mm._NP_DTYPE[dtype]).has_peaks
        on.close()
    # an FFT plan: SPR_OK, nothing changes
    sc = make_scorer("fft", crop=0)
    plan = sc.plan(1, (9, 7), (28, 12))
    pq, pg = _small_pair(sc, plan, "float32")
    before = pc.score_peaks(sc, plan, pq, 2, pg, 3)
    grid, sizes = plan.fft_size, (plan.query_item_bytes, plan.gallery_item_bytes)
    assert sc.lib.spr_ncc_plan_has_peaks(plan.handle) == 1
    assert sc.lib.spr_ncc_plan_enable_peaks(plan.handle) == 0
    assert sc.lib.spr_ncc_plan_has_peaks(plan.handle) == 1 and sc.lib.spr_ncc_plan_method(plan.handle) == _lib.NCC_FFT
    rows, cols = _lib.C.c_int32(), _lib.C.c_int32()
    sc.lib.check(sc.lib.spr_ncc_plan_fft_size(plan.handle, _lib.C.byref(rows), _lib.C.byref(cols)))
    assert (rows.value, cols.value) == grid
    assert (sc.lib.spr_ncc_query_bytes(plan.handle, 1), sc.lib.spr_ncc_gallery_bytes(plan.handle, 1)) == sizes
    after = pc.score_peaks(sc, plan, pq, 2, pg, 3)
    np.testing.assert_array_equal(pc.bits(after[0]), pc.bits(before[0]))
    np.testing.assert_array_equal(after[1], before[1])
    assert sc.lib.spr_ncc_plan_enable_peaks(None) == _lib.SPR_ERR_ARG
    sc.close()


# ------------------------------------------------------------------------------------------------ 2. planted peaks
def check_planted(make_scorer, case, monkeypatch, every_position):
    """mfma_map_cases.PEAK_CASES through spr_ncc_score_peaks: every good matched pair's peak is the planted pixel."""
    stride = 1 if every_position else case.emu_stride
    mcase = case.map_case()
    templates, items, _, _, pos, owner, want, good = mm._peak_inputs(case.t, case.i, mcase.dtype, stride)
    sc, plan = mm.make_plan(peaks_on(make_scorer), mcase, monkeypatch)
    assert plan.has_peaks
    nq, ng = mm.N_TEMPLATES, len(pos)
    pq, pg = pc.prepare(sc, plan, templates[:, None], items[:, None])
    scores, yx, _ = pc.score_peaks(sc, plan, pq, nq, pg, ng)
    if case.launches > 1:
        per = -(-ng // case.launches)
        assert -(-ng // per) == case.launches
        monkeypatch.setenv("SPR_NCC_MAX_TILES", str(per))
        sliced = pc.score_peaks(sc, plan, pq, nq, pg, ng)
        monkeypatch.delenv("SPR_NCC_MAX_TILES")
        np.testing.assert_array_equal(pc.bits(sliced[0]), pc.bits(scores), err_msg=case.id)
        np.testing.assert_array_equal(sliced[1], yx, err_msg=case.id)
    sc.close()
    assert_inside(yx, *case.i, case.id)
    off = [k for k in np.flatnonzero(good) if tuple(yx[owner[k], k]) != pos[k]]
    print(f"[mfma peak form] {case.id}: {ng} positions, {int(good.sum())} good, {len(off)} off")
    if off:
        lines = [f"query {owner[k]} (block {owner[k] // 64} wave {owner[k] % 64 // 16} lane {owner[k] % 16}) item {k} planted at "
                 f"{pos[k]}: got {tuple(yx[owner[k], k])}" for k in off[:25]]
        raise AssertionError(
            f"{case.id}: {len(off)} planted peaks off: planted rows {sorted({pos[k][0] for k in off})}, planted columns "
            f"{sorted({pos[k][1] for k in off})}, query slots (wave, lane) "
            f"{sorted({(int(owner[k]) % 64 // 16, int(owner[k]) % 16) for k in off})}\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------ 3. ties
TIE_CASES = [((7, 4), (4, 3)), ((5, 3), (3, 3))]  # (template, tiling): 28 x 12 = the frame; 15 x 9 leaves spare positions


@functools.lru_cache(maxsize=None)
def tie_inputs(t, tiling):
    """An integer template with zero sum (entries in [-4, 4], the last one adjusted) and the map that tiles it: every value
    is exact in bfloat16 and float16, every aligned window is the template itself, the map's mean is exactly 0.  From the
    float64 oracle alone: the maxima are the aligned centres (th // 2 + th * a, tw // 2 + tw * b), equal within 1e-12, and every
    other pixel lies more than 0.1 below them."""
    (th, tw), (ny, nx) = t, tiling
    rng = np.random.default_rng([31, th, tw])
    tpl = rng.integers(-4, 5, size=(th, tw)).astype(np.float32)
    tpl[-1, -1] -= tpl.sum()
    assert tpl.sum() == 0 and np.abs(tpl).max() <= 16 and tpl.std() > 0
    item = np.tile(tpl, (ny, nx))
    want = oracle.ncc_maps(tpl[None], item[None], precise=True)[0]
    centres = sorted((th // 2 + th * a, tw // 2 + tw * b) for a in range(ny) for b in range(nx))
    order = np.argsort(-want.ravel(), kind="stable")
    top = want.ravel()[order]
    n = len(centres)
    assert sorted((int(p) // item.shape[1], int(p) % item.shape[1]) for p in order[:n]) == centres
    assert top[0] - top[n - 1] <= 1e-12 and top[n] < top[0] - 0.1, (top[0], top[n - 1], top[n])
    for a in (tpl, item):
        a.flags.writeable = False
    return tpl, item, centres


def check_ties(make_scorer, t, tiling, form, monkeypatch):
    tpl, item, centres = tie_inputs(t, tiling)
    ih, iw = item.shape
    case = mm.MapCase(t, (ih, iw), form, channels=1)
    assert not case.tuned
    sc, plan = mm.make_plan(peaks_on(make_scorer), case, monkeypatch)
    pq, pg = pc.prepare(sc, plan, mm._to_storage(tpl[None, None], case.dtype)[0], mm._to_storage(item[None, None], case.dtype)[0])
    scores, yx, _ = pc.score_peaks(sc, plan, pq, 1, pg, 1)
    own = np.array(sc.dev.to_host(sc.ncc_maps_device(plan, pq, pg)))[0]  # one channel: the map is the channel sum
    sc.close()
    first = centres[0]
    assert first == (t[0] // 2, t[1] // 2)
    print(f"[mfma peak form] ties {case.id}: score {scores[0, 0]:.7f}, peak {tuple(yx[0, 0])}, "
          f"{int((own == own.max()).sum())} equal maxima in the plan's own map")
    assert_inside(yx, ih, iw, case.id)
    assert abs(float(scores[0, 0]) - 1.0) <= score_bound(form)
    assert tuple(yx[0, 0]) == first, (case.id, tuple(yx[0, 0]))
    assert np.unravel_index(int(own.argmax()), own.shape) == first  # (np.argmax: the first maximum in row-major order)


# ------------------------------------------------------------------------------------------------ 4. every instance
INSTANCE_CASES = mm.MAP_CASES + mm.WIDE_CASES


def check_instance(make_scorer, case, monkeypatch):
    """peak_cases.check_instance on the matrix-core cases: one multi-channel pair with dead channels; the named pixel holds
    the oracle's maximum (on the values as stored) within POSITION_LEAD."""
    q, g, want = mm.map_inputs(case)
    sc, plan = mm.make_plan(peaks_on(make_scorer), case, monkeypatch)
    assert plan.has_peaks
    pq, pg = pc.prepare(sc, plan, q[None], g[None])
    scores, yx, tags = pc.score_peaks(sc, plan, pq, 1, pg, 1, tag=4)
    sc.close()
    tol = score_bound(case.form)
    summed = want.sum(axis=0)
    top = float(summed.max())
    y, x = (int(v) for v in yx[0, 0])
    print(f"[mfma peak form] {case.id}: score {scores[0, 0]:.7f}, peak ({y}, {x}), oracle max {top:.7f}"
          f"{'' if y < 0 else f', oracle at peak {summed[y, x]:.7f}'}")
    assert_inside(yx, *case.i, case.id)
    if top < -tol:
        assert scores[0, 0] == 0 and (y, x) == (-1, -1) and tags[0, 0] == -1
        return
    if top > tol:
        assert scores[0, 0] > 0
    if scores[0, 0] > 0:
        assert tags[0, 0] == 4
        assert summed[y, x] >= top - POSITION_LEAD, (case.id, (y, x), float(summed[y, x]), top)
        assert abs(float(scores[0, 0]) - top / case.channels) <= tol


# ------------------------------------------------------------------------------------------------ 5. accumulate, edges
RULE_SCORERS = [("mfma", "bfloat16"), ("mfma_f32", "float32")]
RULE_SHAPE = ((5, 5), (16, 12))


@functools.lru_cache(maxsize=None)
def stored_sweep(dtype):
    """ncc_map_cases._sweep_inputs of the (5, 5)-on-(16, 12) set as the plan stores it: (templates, items) in the storage
    type, the planted positions, and which matched pairs are good by the float64 oracle on the stored values."""
    t, i = RULE_SHAPE
    templates, items, pos, _, good = mc._sweep_inputs(t, i)
    if dtype == "float32":
        return templates, items, pos, good
    (ts, tf), (its, itf) = mm._to_storage(np.array(templates), dtype), mm._to_storage(np.array(items), dtype)
    good = np.zeros(len(pos), dtype=bool)
    for q in range(mc.N_TEMPLATES):
        maps = oracle.ncc_maps(np.broadcast_to(tf[q], (len(pos),) + t).copy(), itf, precise=True)
        for k in range(q, len(pos), mc.N_TEMPLATES):
            flat = maps[k].ravel()
            planted = pos[k][0] * i[1] + pos[k][1]
            good[k] = flat.argmax() == planted and flat[planted] - np.delete(flat, planted).max() >= mc.MARGIN
    assert good.mean() >= mc.GOOD_SHARE
    for a in (ts, its, good):
        a.flags.writeable = False
    return ts, its, pos, good


def _rule_plan(make_scorer, method, dtype):
    t, i = RULE_SHAPE
    sc = peaks_on(make_scorer)(method)
    plan = sc.plan(1, t, i, dtype=mm._NP_DTYPE[dtype])
    assert plan.method == similarity._METHODS[method] and plan.has_peaks
    return sc, plan


def check_accumulate_rule(make_scorer, method, dtype):
    """peak_cases.check_accumulate_rule on a matrix-core plan: two query batches A, B against the same items through
    accumulate_max, in both orders of the calls and of the tags, with and without a tag matrix."""
    templates, items, pos, good = stored_sweep(dtype)
    sc, plan = _rule_plan(make_scorer, method, dtype)
    nq, ng = len(templates), len(items)
    pq_a, pg = pc.prepare(sc, plan, templates[:, None], items[:, None])
    pq_b = sc.prepare_queries(plan, sc.dev.to_device(np.ascontiguousarray(np.roll(templates, 1, axis=0)[:, None])))
    s_a, yx_a, _ = pc.score_peaks(sc, plan, pq_a, nq, pg, ng)
    s_b, yx_b, _ = pc.score_peaks(sc, plan, pq_b, nq, pg, ng)
    assert (s_b > s_a).any() and (s_b < s_a).any()  # both a strictly better and a worse second batch occur
    assert_inside(np.concatenate([yx_a, yx_b]), *RULE_SHAPE[1], method)

    def run(calls, with_tags=True):
        m = pc.PeakMatrices(sc, nq, ng, with_tags)
        for pq, tag in calls:
            sc.lib.check(m.score(plan, pq, pg, accumulate=True, tag=tag))
        s, packed, tags = m.read()
        return s, pc.unpack(packed), tags

    for tags_in in ((5, 2), (2, 5)):  # the same batch twice: equal scores, the lower tag stays whichever call brought it
        s, yx, tags = run([(pq_a, tags_in[0]), (pq_a, tags_in[1])])
        np.testing.assert_array_equal(pc.bits(s), pc.bits(s_a))
        np.testing.assert_array_equal(yx, yx_a)
        np.testing.assert_array_equal(tags, np.where(s_a > 0, 2, -1))
    for first, second in (((pq_a, s_a, yx_a, 1), (pq_b, s_b, yx_b, 2)), ((pq_b, s_b, yx_b, 2), (pq_a, s_a, yx_a, 1))):
        s, yx, tags = run([(first[0], first[3]), (second[0], second[3])])
        take = second[1] > first[1]
        np.testing.assert_array_equal(pc.bits(s), pc.bits(np.where(take, second[1], first[1])))
        np.testing.assert_array_equal(yx, np.where(take[..., None], second[2], first[2]))
        np.testing.assert_array_equal(tags, np.where(s > 0, np.where(take, second[3], first[3]), -1))
        s2, yx2, none = run([(first[0], first[3]), (second[0], second[3])], with_tags=False)
        assert none is None
        np.testing.assert_array_equal(pc.bits(s2), pc.bits(s))
        np.testing.assert_array_equal(yx2, yx)
    sc.close()


def check_edges(make_scorer, monkeypatch, method, dtype, n_items=75):
    """peak_cases.check_edges on a matrix-core plan: an odd query count, no tag matrix, all-constant queries, one gallery item
    per launch (SPR_NCC_MAX_TILES=1) and the argument checks of spr_ncc_score_peaks, inside guarded wider matrices.  The
    emulation takes the first n_items = 30 items (each a launch of its own in the sliced run), the MI355X all 75."""
    t, i = RULE_SHAPE
    templates, items, pos, good = stored_sweep(dtype)
    items, pos, good = items[:n_items], pos[:n_items], good[:n_items]
    constant = mm._to_storage(np.full((2,) + t, 0.75, np.float32), dtype)[0]  # (0.75 is exact in every storage type)
    queries = np.concatenate([templates, constant])[:, None]  # 5 queries, the last two constant
    mm.set_env(monkeypatch, ())
    sc, plan = _rule_plan(make_scorer, method, dtype)
    nq, ng = len(queries), len(items)
    assert nq % 2 == 1 and ng >= 3
    pq, pg = pc.prepare(sc, plan, queries, items[:, None])
    scores, yx, tags = pc.score_peaks(sc, plan, pq, nq, pg, ng, tag=9)
    assert not scores[3:].any() and (yx[3:] == -1).all() and (tags[3:] == -1).all()
    assert_inside(yx, *i, method)
    for k in np.flatnonzero(good):
        assert tuple(yx[k % mc.N_TEMPLATES, k]) == pos[k]
    no_tag = pc.score_peaks(sc, plan, pq, nq, pg, ng, with_tags=False)
    assert no_tag[2] is None
    np.testing.assert_array_equal(pc.bits(no_tag[0]), pc.bits(scores))
    np.testing.assert_array_equal(no_tag[1], yx)
    monkeypatch.setenv("SPR_NCC_MAX_TILES", "1")  # one gallery item per launch: ng launches
    sliced = pc.score_peaks(sc, plan, pq, nq, pg, ng, tag=9)
    monkeypatch.delenv("SPR_NCC_MAX_TILES")
    np.testing.assert_array_equal(pc.bits(sliced[0]), pc.bits(scores))
    np.testing.assert_array_equal(sliced[1], yx)
    np.testing.assert_array_equal(sliced[2], tags)
    m = pc.PeakMatrices(sc, nq, ng)
    lib, dev = sc.lib, sc.dev
    ok = [plan.handle, dev.ptr(pq), nq, dev.ptr(pg), ng, dev.ptr(m.scores) + 4 * pc.GUARD, dev.ptr(m.yx) + 4 * pc.GUARD, None, m.ld,
          pc.COL0, 0, 0, dev.stream()]
    for at, bad in ((0, None), (1, None), (3, None), (5, None), (6, None), (2, -1), (4, -1), (8, ng), (9, -1), (2, 65536)):
        args = list(ok)
        args[at] = bad
        assert lib.spr_ncc_score_peaks(*args) == _lib.SPR_ERR_ARG, (at, bad)
    args = list(ok)
    args[2] = 0
    assert lib.spr_ncc_score_peaks(*args) == 0
    m.read()  # nothing written by any of them
    sc.close()


# ------------------------------------------------------------------------------------------------ 6. host level
def check_planted_matrix(scorer):
    """peak_cases.check_planted_matrix with the score bound of the scorer's storage type."""
    seed, nq, ng, c, h, w = PLANTED
    q, g, m, sim, peak, lead = sc_cases.planted_reference(PLANTED, scorer.storage)
    ih, iw = h - 4, w - 4
    scores, variant, yx = scorer.score_matrix_located(q, g)
    assert scores.dtype == np.float32 and variant.dtype == np.int32 and yx.dtype == np.int32
    assert scores.shape == variant.shape == (nq, ng) and yx.shape == (nq, ng, 2)
    np.testing.assert_array_equal(pc.bits(scores), pc.bits(scorer.score_matrix(q, g)))
    tol = score_bound(scorer.storage)
    print(f"[mfma peak form] matrix {PLANTED}, {scorer.storage}: max |score - oracle| = "
          f"{np.abs(scores - np.maximum(sim, 0.0)).max():.2e}, bound {tol:.2e}")
    np.testing.assert_allclose(scores, np.maximum(sim, 0.0), atol=tol, rtol=0)
    assert_inside(yx, ih, iw, "planted matrix")
    hit = scores > 0
    assert (variant[hit] == 0).all() and (variant[~hit] == -1).all() and (yx[~hit] == -1).all()
    sure = (lead > POSITION_LEAD) & hit
    print(f"[mfma peak form] matrix {PLANTED}: {int(sure.sum())} of {nq * ng} pairs compared")
    assert 2 * sure.sum() >= nq * ng
    np.testing.assert_array_equal(yx[sure], peak[sure])
    pairs = [(qi, gi) for qi in range(nq) for gi in range(ng)]
    _, l_variant, l_yx = scorer.locate(q, g, pairs)
    np.testing.assert_array_equal(l_yx.reshape(nq, ng, 2)[sure], yx[sure])
    for qi in range(nq):
        dy, dx = synth.query_shift(seed, qi)
        assert tuple(yx[qi, m[qi]]) == (ih // 2 + dy, iw // 2 + dx)


def check_ragged(scorer):
    """peak_cases.check_ragged with the ragged set as the scorer stores it (the oracle sees the stored values)."""
    rq, rg = (sc_cases._rounded(items, scorer.storage) for items in pc.ragged_set())
    scores, variant, yx = scorer.score_matrix_located(rq, rg)
    np.testing.assert_array_equal(pc.bits(scores), pc.bits(scorer.score_matrix(rq, rg)))
    assert all(p.has_peaks for p in scorer._plans.values())
    pairs = [(qi, gi) for qi in range(len(rq)) for gi in range(len(rg))]
    _, l_variant, l_yx = scorer.locate(rq, rg, pairs)
    compared = 0
    for k, (qi, gi) in enumerate(pairs):
        summed = oracle.ncc_maps(rq[qi][:, 2:-2, 2:-2], rg[gi][:, 2:-2, 2:-2], precise=True).sum(axis=0)
        assert_inside(yx[qi, gi], *summed.shape, f"ragged pair {(qi, gi)}")
        top = np.sort(summed.ravel())[::-1]
        if top[0] - top[1] > POSITION_LEAD and top[0] > score_bound(scorer.storage):
            compared += 1
            assert variant[qi, gi] == l_variant[k] == 0 and tuple(yx[qi, gi]) == tuple(l_yx[k]), (qi, gi)
            assert tuple(yx[qi, gi]) == np.unravel_index(int(summed.argmax()), summed.shape)
    assert 2 * compared >= len(pairs)


def check_located_variants(scorer):
    """peak_cases.check_located_variants on the queries as the scorer stores them.  The score is held to the oracle for float32
    storage only: a 16-bit scorer stores every variant as the device resampler's float32 result rounded once more, which the
    host oracle does not restate bit for bit - there the scores are held bit-equal to score_matrix, the variant and the
    position to the oracle's choice (leads of 0.19 and more, shortlist_cases.check_locate_variants) and to locate."""
    import os

    from parity_cases import GOLDEN

    z = np.load(os.path.join(GOLDEN, "variants.npz"))
    nq, ng, c, h, w, seed = (int(v) for v in z["shape"])
    q, g, m = synth.dataset(seed, nq, ng, c, h, w)
    q, g = sc_cases._rounded(q, scorer.storage), sc_cases._rounded(g, scorer.storage)
    for rot, sc in pc.VARIANT_SETTINGS:
        lists = oracle.transform_variants(q, rot, sc)
        required = {}
        for qi in range(nq):
            sims = np.array([float(oracle.get_similarity(v[qi], g[m[qi]], precise=True)) for v in lists])
            best = int(np.argmax(sims))
            seen = lambda v: v[qi][:, 2:-2, 2:-2]
            other = [sims[k] for k, v in enumerate(lists)
                     if not (seen(v).shape == seen(lists[best]).shape and np.array_equal(seen(v), seen(lists[best])))]
            if sims[best] - max(other) > POSITION_LEAD:
                required[qi] = (best, sims[best])
        assert 2 * len(required) >= nq, (rot, sc, len(required))  # from the oracle alone
        scores, variant, yx = scorer.score_matrix_located(q, g, rotations=rot, scales=sc)
        np.testing.assert_array_equal(pc.bits(scores), pc.bits(scorer.score_matrix(q, g, rotations=rot, scales=sc)))
        assert all(p.has_peaks for p in scorer._plans.values())
        assert ((variant >= 0) == (scores > 0)).all() and variant.max() < len(lists)
        assert_inside(yx, h - 4, w - 4, f"variants {rot} {sc}")
        for qi, (best, sim) in required.items():
            assert variant[qi, m[qi]] == best, (rot, sc, qi, variant[qi, m[qi]])
            if scorer.storage == "float32":
                assert abs(scores[qi, m[qi]] - sim) <= score_bound(scorer.storage)
        pairs = [(qi, m[qi]) for qi in required]
        _, l_variant, l_yx = scorer.locate(q, g, pairs, rotations=rot, scales=sc)
        for k, (qi, gi) in enumerate(pairs):
            assert l_variant[k] == variant[qi, gi] and tuple(l_yx[k]) == tuple(yx[qi, gi]), (rot, sc, qi)


def check_second_pass_counts(make_scorer, method, storage, monkeypatch):
    """spr_ncc_maps calls of retrieve and score_matrix_located: none with the flag on, Q * k * V and Q * G * V without it."""
    q, g, m, sim, peak, lead = sc_cases.planted_reference(PLANTED, storage)
    nq, ng = len(q), len(g)
    rot = [-15, 180]
    on = make_scorer(method, storage=storage, matrix_core_peaks=True)
    pc.check_no_second_pass(on, monkeypatch)  # retrieve: no call, the planted positions, k = the whole gallery
    calls = pc.count_maps_calls(monkeypatch, on.lib)
    similarity.retrieve_with_scores(q, g, sc_cases._cfg(rot=rot), k=2, scorer=on)
    s_on, v_on, yx_on = on.score_matrix_located(q, g, rotations=rot)
    assert not calls, f"{len(calls)} spr_ncc_maps calls with the flag on"
    assert all(p.has_peaks for p in on._plans.values())
    off = make_scorer(method, storage=storage)
    assert not off.matrix_core_peaks
    similarity.retrieve(q, g, sc_cases._cfg(), k=3, scorer=off)
    assert not any(p.has_peaks for p in off._plans.values())
    assert len(calls) == nq * 3 * 1, len(calls)
    del calls[:]
    similarity.retrieve(q, g, sc_cases._cfg(rot=rot), k=2, scorer=off)
    assert len(calls) == nq * 2 * (1 + len(rot)), len(calls)
    del calls[:]
    s_off, v_off, yx_off = off.score_matrix_located(q, g, rotations=rot)
    assert len(calls) == nq * ng * (1 + len(rot)), len(calls)
    # both routes: the same scores bit for bit, and the same variant wherever it is beyond doubt on both
    np.testing.assert_array_equal(pc.bits(s_on), pc.bits(s_off))
    assert ((v_on >= 0) == (s_on > 0)).all()
    on.close()
    off.close()


def check_config_key(make_from_config):
    """[mi355x] matrix_core_peaks reaches the scorer and is part of the scorer cache's key; off by default; a bool."""
    import pytest

    from shoeprint_image_retrieval_amd.config import MI355X_DEFAULTS, normalise

    assert MI355X_DEFAULTS["matrix_core_peaks"] is False and normalise({})["mi355x"]["matrix_core_peaks"] is False
    with pytest.raises(ValueError, match="matrix_core_peaks"):
        normalise({"mi355x": {"matrix_core_peaks": 1}})
    base = {"ncc_method": "mfma", "dtype": "bfloat16"}
    cfg = normalise({"comparison": {"n_processes": 1, "rotations": "", "scales": ""}, "mi355x": dict(base, matrix_core_peaks=True)})
    sc = make_from_config(cfg)
    assert sc.matrix_core_peaks and sc is make_from_config(cfg)
    plain = make_from_config(normalise({"comparison": {"n_processes": 1, "rotations": "", "scales": ""}, "mi355x": dict(base)}))
    assert plain is not sc and not plain.matrix_core_peaks
    assert sc.plan(5, (20, 14), (20, 14), dtype="bfloat16").has_peaks
    assert not plain.plan(5, (20, 14), (20, 14), dtype="bfloat16").has_peaks
