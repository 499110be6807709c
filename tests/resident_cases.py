"""Checks of the device-resident route - spr_items_gather and spr_block_scatter (csrc/resident.hip), features.FeatureSet /
DeviceImages, Model.get_multiple_feature_maps_device, the scorer's surface on resident sets, the loader's DeviceImages -
shared by the CPU-emulation runner (test_emu_resident.py, not gpu) and the MI355X runner (test_gpu_resident.py, gpu).

Everything here is exact: the gather is a copy or a round-to-nearest-even conversion (compared as bits with the backend's own
``astype_storage``), the scatter a copy or a maximum, and the resident route runs the launches of the host-list route on the
bytes of the host-list route, so its results are compared as bits with that route's.
"""

import contextlib
import functools
import io

import numpy as np
import pytest

import peak_cases as pc
from shoeprint_image_retrieval_amd import _lib, similarity
from shoeprint_image_retrieval_amd.features import DeviceImages, FeatureSet

GUARD = 64     # bytes of poison on either side of every buffer the two kernels write
POISON = 0xA5
N_SRC = 7
# the sizes the kernels take different paths at: one element, below a 16-byte vector, an odd size (2-byte destinations then
# start items on odd dwords and the source phase changes from item to item), a multiple of 4 (the aligned path), and more than
# one tile of 1024 vectors with an odd tail
ITEM_ELEMS = [1, 3, 105, 1028, 8203]
INDEXES = {0: [], 1: [3], 5: [6, 4, 4, 1, 0]}  # (descending, with a repeat)
STORAGES = ["float32", "float16", "bfloat16"]
CODES = {"float32": _lib.F32, "float16": _lib.F16, "bfloat16": _lib.BF16}
SPECIAL = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,     # bfloat16 ties: to even downwards / upwards
                    -(1 + 2.0 ** -8), 2.0 ** -24, 3 * 2.0 ** -25, 6.0e-8, 3.0e-5, -4.0e-6,  # float16 subnormals, a tie among them
                    65504.0, 65520.0, -65520.0, 65519.0,  # the largest float16, the first value that rounds to inf
                    -0.0, 0.0, np.inf, -np.inf, 3.3e38, 1.0e-40], dtype=np.float32)


def raw_bytes(dev, buf) -> np.ndarray:
    """The bytes of a device buffer of any storage type (a bfloat16 tensor has no numpy form)."""
    if dev.name == "hip":
        import torch

        return dev.to_host(buf.contiguous().view(torch.uint8).reshape(-1))
    return np.ascontiguousarray(buf).view(np.uint8).reshape(-1).copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. gather
@functools.lru_cache(maxsize=None)
def gather_source(item_elems):
    """[7, item_elems] float32: SPECIAL spread over the items (as many of them as the set has room for), the rest normal
    values over twelve binades.  Read-only."""
    rng = np.random.default_rng(item_elems)
    src = (rng.standard_normal((N_SRC, item_elems)) * 2.0 ** rng.integers(-8, 4, (N_SRC, item_elems))).astype(np.float32)
    flat = src.reshape(-1)
    at = np.arange(len(SPECIAL)) * max(1, len(flat) // len(SPECIAL)) % len(flat)
    flat[at] = SPECIAL[:len(at)]
    src.setflags(write=False)
    return src


def _guarded(dev, nbytes):
    return dev.to_device(np.full(nbytes + 2 * GUARD, POISON, dtype=np.uint8))


def _inside(dev, buf, nbytes):
    host = raw_bytes(dev, buf)
    assert (host[:GUARD] == POISON).all() and (host[GUARD + nbytes:] == POISON).all(), "written outside the destination"
    return host[GUARD:GUARD + nbytes]


def check_gather(scorer, item_elems, storage, index):
    lib, dev = scorer.lib, scorer.dev
    src = gather_source(item_elems)
    n = len(index)
    size = 4 if storage == "float32" else 2
    src_dev = dev.to_device(np.array(src))
    idx_dev = dev.to_device(np.asarray(index + [0], dtype=np.int32))  # (never empty: the call takes a pointer)
    out = _guarded(dev, n * item_elems * size)
    lib.check(lib.spr_items_gather(dev.ptr(src_dev), item_elems, dev.ptr(idx_dev), n, dev.ptr(out) + GUARD, CODES[storage],
                                   dev.stream()))
    got = _inside(dev, out, n * item_elems * size)
    np.testing.assert_array_equal(bits(dev.to_host(src_dev)), bits(src))  # the source is only read
    if n == 0:
        return
    want = raw_bytes(dev, dev.astype_storage(dev.to_device(np.ascontiguousarray(src[index])), storage))
    if storage == "float32":
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        return
    got16, want16 = got.view(np.uint16), want.view(np.uint16)
    value = src[index].reshape(-1)
    # what the conversion must do at the special values, from the formats alone
    if storage == "bfloat16":
        for v, b in ((1 + 2.0 ** -8, 0x3F80), (1 + 3 * 2.0 ** -8, 0x3F82), (-0.0, 0x8000), (np.inf, 0x7F80), (-np.inf, 0xFF80)):
            hit = bits(value) == bits(np.float32(v))
            assert (got16[hit] == b).all(), (v, got16[hit])
    else:
        for v, b in ((65504.0, 0x7BFF), (65520.0, 0x7C00), (-65520.0, 0xFC00), (65519.0, 0x7BFF), (2.0 ** -24, 0x0001),
                     (3 * 2.0 ** -25, 0x0002), (-0.0, 0x8000), (np.inf, 0x7C00), (-np.inf, 0xFC00), (3.3e38, 0x7C00), (1.0e-40, 0)):
            hit = bits(value) == bits(np.float32(v))
            assert (got16[hit] == b).all(), (v, got16[hit])
    np.testing.assert_array_equal(got16, want16)


def check_gather_grid_stride(scorer):
    """More (item, tile) pairs than the launch has workgroups, one element per item: the form NccScorer.cells_device uses."""
    lib, dev = scorer.lib, scorer.dev
    src = np.arange(1000, 1000 + 611, dtype=np.int32)  # 4-byte words of any kind travel as float32 -> float32
    index = np.random.default_rng(5).integers(0, len(src), 4200).astype(np.int32)
    out = _guarded(dev, 4 * len(index))
    src_dev, idx_dev = dev.to_device(src), dev.to_device(index)
    lib.check(lib.spr_items_gather(dev.ptr(src_dev), 1, dev.ptr(idx_dev), len(index), dev.ptr(out) + GUARD, _lib.F32, dev.stream()))
    np.testing.assert_array_equal(_inside(dev, out, 4 * len(index)).view(np.int32), src[index])
    mat = dev.to_device(np.arange(35, dtype=np.int32).reshape(5, 7) - 3)
    np.testing.assert_array_equal(scorer.cells_device(mat, 7, [4, 0, 2, 2], [6, 0, 3, 3]), [31, -3, 14, 14])
    assert scorer.cells_device(mat, 7, [], []).shape == (0,)


def check_gather_arguments(scorer):
    lib, dev = scorer.lib, scorer.dev
    src, idx = dev.to_device(np.zeros((3, 8), np.float32)), dev.to_device(np.array([2, 0], np.int32))
    out = _guarded(dev, 2 * 8 * 4)
    ok = [dev.ptr(src), 8, dev.ptr(idx), 2, dev.ptr(out) + GUARD, _lib.F32, dev.stream()]
    assert lib.spr_items_gather(*ok) == 0
    for at, bad in ((0, None), (2, None), (4, None), (1, -1), (3, -1), (5, 3), (5, -1), (4, dev.ptr(out) + GUARD + 2), (0, dev.ptr(src) + 2)):
        args = list(ok)
        args[at] = bad
        out = _guarded(dev, 2 * 8 * 4)
        if at != 4:
            args[4] = dev.ptr(out) + GUARD
        assert lib.spr_items_gather(*args) == _lib.SPR_ERR_ARG, (at, bad)
        assert b"spr_items_gather" in lib.spr_last_error()
        _inside(dev, out, 0)  # nothing was written
    assert lib.spr_items_gather(None, 8, None, 0, None, _lib.BF16, dev.stream()) == 0  # no items: nothing to do
    assert lib.spr_items_gather(None, 0, None, 5, None, _lib.F16, dev.stream()) == 0
    # a 2-byte destination needs 2-byte alignment only
    out = _guarded(dev, 2 * 8 * 2 + 2)
    assert lib.spr_items_gather(dev.ptr(src), 8, dev.ptr(idx), 2, dev.ptr(out) + GUARD + 2, _lib.F16, dev.stream()) == 0
    assert not _inside(dev, out, 2 * 8 * 2 + 2)[2:].any() and (_inside(dev, out, 2 * 8 * 2 + 2)[:2] == POISON).all()


# ------------------------------------------------------------------------------------------------ 2. scatter
ROWS, COLS, LD, SRC_LD = [4, 0, 2], [6, 1, 3, 0], 9, 6


def _scatter(scorer, dst_host, src_host, mode, rows=ROWS, cols=COLS, nr=None, nc=None):
    """spr_block_scatter into a [5, 7] matrix held with row pitch 9 between guard bands; returns the [5, 9] words after it."""
    lib, dev = scorer.lib, scorer.dev
    wide = np.full((5, LD), 0x5A5A5A5A, dtype=np.uint32)
    wide[:, :7] = dst_host.view(np.uint32)
    buf = np.full(5 * LD * 4 + 2 * GUARD, POISON, dtype=np.uint8)
    buf[GUARD:GUARD + 5 * LD * 4] = wide.view(np.uint8).reshape(-1)
    dst = dev.to_device(buf)
    src = dev.to_device(np.ascontiguousarray(src_host))
    r, c = dev.to_device(np.asarray(rows, np.int32)), dev.to_device(np.asarray(cols, np.int32))
    lib.check(lib.spr_block_scatter(dev.ptr(dst) + GUARD, LD, dev.ptr(src), SRC_LD, dev.ptr(r), len(rows) if nr is None else nr,
                                    dev.ptr(c), len(cols) if nc is None else nc, mode, dev.stream()))
    np.testing.assert_array_equal(dev.to_host(src).view(np.uint32), np.ascontiguousarray(src_host).view(np.uint32))
    after = _inside(dev, dst, 5 * LD * 4).view(np.uint32).reshape(5, LD)
    assert (after[:, 7:] == 0x5A5A5A5A).all(), "the pitch columns were written"
    return after[:, :7]


def check_scatter(scorer):
    rng = np.random.default_rng(11)
    # copy mode, int32 with negatives and -1
    dst = rng.integers(-1000, 1000, (5, 7)).astype(np.int32)
    src = rng.integers(-2 ** 31, 2 ** 31 - 1, (3, SRC_LD)).astype(np.int32)
    src[0, 0], src[1, 2], src[2, 3] = -1, -1, 0
    want = dst.copy()
    want[np.ix_(ROWS, COLS)] = src[:, :4]
    np.testing.assert_array_equal(_scatter(scorer, dst, src, 0).view(np.int32), want)
    # max mode: below, equal to and above what is there
    dst = rng.uniform(0.0, 1.0, (5, 7)).astype(np.float32)
    src = rng.uniform(0.0, 1.0, (3, SRC_LD)).astype(np.float32)
    block = dst[np.ix_(ROWS, COLS)]
    src[0, :4] = block[0]                                        # equal
    src[1, :4] = np.nextafter(block[1], np.float32(2.0))          # one ulp above
    src[2, :2], src[2, 2:4] = np.nextafter(block[2, :2], np.float32(-1.0)), block[2, 2:4] * 0.5  # below
    src[:, 4:] = 9.0  # (beyond nc: never read as data)
    want = dst.copy()
    want[np.ix_(ROWS, COLS)] = np.maximum(block, src[:, :4])
    assert (src[:, :4] > block).any() and (src[:, :4] < block).any() and (src[:, :4] == block).any()
    np.testing.assert_array_equal(_scatter(scorer, dst, src, 1), bits(want))
    # nothing to do
    for nr, nc in ((0, 4), (3, 0), (0, 0)):
        for mode in (0, 1):
            np.testing.assert_array_equal(_scatter(scorer, dst, src, mode, nr=nr, nc=nc), bits(dst))


def check_scatter_arguments(scorer):
    lib, dev = scorer.lib, scorer.dev
    dst, src = dev.zeros((5, LD), np.float32), dev.zeros((3, SRC_LD), np.float32)
    r, c = dev.to_device(np.asarray(ROWS, np.int32)), dev.to_device(np.asarray(COLS, np.int32))
    ok = [dev.ptr(dst), LD, dev.ptr(src), SRC_LD, dev.ptr(r), 3, dev.ptr(c), 4, 1, dev.stream()]
    assert lib.spr_block_scatter(*ok) == 0
    for at, bad in ((0, None), (2, None), (4, None), (6, None), (5, -1), (7, -1), (8, 2), (8, -1), (1, 3), (3, 3)):
        args = list(ok)
        args[at] = bad
        assert lib.spr_block_scatter(*args) == _lib.SPR_ERR_ARG, (at, bad)
        assert b"spr_block_scatter" in lib.spr_last_error()
    assert lib.spr_block_scatter(None, 0, None, 0, None, 0, None, 0, 0, dev.stream()) == 0
    assert not dev.to_host(dst).any()


# ------------------------------------------------------------------------------------------------ 3. FeatureSet
def check_feature_set(scorer):
    dev = scorer.dev
    rq, rg = pc.ragged_set()
    for items in (rq, rg, rg[::-1], []):
        fs = FeatureSet.from_host(dev, items)
        back = fs.to_host_list()
        assert len(fs) == len(back) == len(items) and fs.nbytes == sum(a.nbytes for a in items)
        for a, b in zip(items, back):
            assert b.dtype == np.float32 and b.shape == a.shape and b.flags["C_CONTIGUOUS"]
            np.testing.assert_array_equal(bits(a), bits(b))
        want = similarity._group_by_shape(items)
        assert [shape for shape, _, _ in fs.classes] == list(want)  # order of first appearance
        assert [list(idx) for _, idx, _ in fs.classes] == list(want.values())
        assert fs.groups() == want and list(fs.groups()) == list(want)
        for used in ([len(items) - 1, 0], list(range(1, len(items)))):
            used = sorted(set(used)) if items else []
            assert list(fs.groups(used).items()) == list(similarity._group_by_shape(items, used).items())
    fs = FeatureSet.from_host(dev, rg)
    np.testing.assert_array_equal(bits(dev.to_host(fs.stack(scorer.lib, [3, 0]))), bits(np.stack([rg[3], rg[0]])))
    with pytest.raises(ValueError, match="share a shape"):
        fs.stack(scorer.lib, [0, 1])
    with pytest.raises(ValueError, match=r"\[C, h, w\]"):
        FeatureSet.from_host(dev, [np.zeros((4, 4), np.float32)])
    # a set assembled on the device may hold a class's items in any order
    mixed = FeatureSet(dev, 3, [((6, 18, 12), [2, 0], dev.to_device(np.stack([rq[2], rq[0]]))), ((6, 16, 14), [1], dev.to_device(rq[1][None]))])
    for a, b in zip(rq, mixed.to_host_list()):
        np.testing.assert_array_equal(bits(a), bits(b))
    assert mixed.groups() == similarity._group_by_shape(rq)
    for bad in ([((6, 18, 12), [0, 0], dev.zeros((2, 6, 18, 12)))], [((6, 18, 12), [0], dev.zeros((2, 6, 18, 12)))],
                [((6, 18, 12), [0], dev.zeros((1, 6, 18, 12)))]):
        with pytest.raises(ValueError):
            FeatureSet(dev, 2, bad)


# ------------------------------------------------------------------------------------------------ 4. scoring
METHODS = [("fft", "float32"), ("direct", "float32"), ("mfma", "bfloat16"), ("mfma_f32", "float32")]
SIDES = ["both", "queries", "gallery"]
ROT, SCALE = [180], [0.9]
MATCH = [0, 2, 3]  # the true matches of the ragged set (check_retrieve_surface)
PAIRS = [(0, 0), (2, 3), (0, 1), (2, 0), (1, 4)]
K = 3


def cfg():
    return {"comparison": {"n_processes": 1, "rotations": ROT, "scales": SCALE}}


def budget_scorer(make_scorer, method, storage):
    """A scorer whose budget splits the two-item gallery class of the ragged set into two chunks (check_call_counts' rule)."""
    rq, _ = pc.ragged_set()
    sc = make_scorer(method, storage=storage)
    shapes = {vs for q in rq[:2] for vs in (q.shape[1:], (int(q.shape[1] * SCALE[0]), int(q.shape[2] * SCALE[0])))}
    assert len(shapes) == 4
    budget = 4 * max(sc.plan(6, vs, (18, 12), dtype=storage).gallery_item_bytes for vs in shapes) + 17
    sc.close()
    sc = make_scorer(method, storage=storage, max_prepared_bytes=budget)
    assert min(sc.gallery_chunk_items(sc.plan(6, vs, (18, 12), dtype=storage), 2, share=4) for vs in shapes) == 1
    return sc


def surface(sc, q, g, only_matrix=False):
    """Every function of the drop-in surface on (q, g): a dict of named arrays (``only_matrix``: score_matrix alone)."""
    out = {}
    out["score_matrix"] = sc.score_matrix(q, g, rotations=ROT, scales=SCALE)
    if only_matrix:
        return out
    out["located.scores"], out["located.variant"], out["located.yx"] = sc.score_matrix_located(q, g, rotations=ROT, scales=SCALE)
    out["locate.score"], out["locate.variant"], out["locate.yx"] = sc.locate(q, g, PAIRS, rotations=ROT, scales=SCALE)
    short = similarity.retrieve(q, g, cfg(), k=K, scorer=sc)
    for name in ("index", "score", "variant", "peak_yx", "offset"):
        out["retrieve." + name] = getattr(short, name)
    plain = similarity.retrieve(q, g, cfg(), k=K, locate=False, scorer=sc)
    assert plain.variant is None and plain.peak_yx is None and plain.offset is None
    out["retrieve_plain.index"], out["retrieve_plain.score"] = plain.index, plain.score
    scores, short2 = similarity.retrieve_with_scores(q, g, cfg(), K, scorer=sc)
    out["with_scores.scores"], out["with_scores.index"] = scores, short2.index
    out["compare_maps"] = similarity.compare_maps(q, g, MATCH, cfg(), scorer=sc)
    pre = np.linspace(0.0, 1.0, len(q) * len(g), dtype=np.float32).reshape(len(q), len(g))
    acc = pre.copy()
    assert sc.score_matrix(q, g, accumulate_into=acc, rotations=ROT, scales=SCALE) is acc
    np.testing.assert_array_equal(bits(acc), bits(np.maximum(pre, out["score_matrix"])))
    assert (pre > out["score_matrix"]).any() and (pre < out["score_matrix"]).any()
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape, name
        if x.dtype == np.float32:
            np.testing.assert_array_equal(bits(x), bits(y), err_msg=name)
        else:
            np.testing.assert_array_equal(x, y, err_msg=name)


_HOST_RESULTS = {}


def host_results(make_scorer, method, storage, only_matrix=False):
    """The host-list results of one method, computed once and shared by its cases: read-only."""
    key = (method, storage, only_matrix)
    if key not in _HOST_RESULTS:
        sc = budget_scorer(make_scorer, method, storage)
        _HOST_RESULTS[key] = surface(sc, *pc.ragged_set(), only_matrix=only_matrix)
        sc.close()
    return _HOST_RESULTS[key]


def check_surface(make_scorer, method, storage, sides, only_matrix=False):
    """``only_matrix``: score_matrix alone (the emulation of the matrix-core pair kernels takes seconds per launch; the
    MI355X runner checks the whole surface for every method)."""
    want = host_results(make_scorer, method, storage, only_matrix)
    assert (want["score_matrix"] > 0).all() and (only_matrix or (want["located.variant"] > 0).any())
    sc = budget_scorer(make_scorer, method, storage)
    rq, rg = pc.ragged_set()
    q = FeatureSet.from_host(sc.dev, rq) if sides in ("both", "queries") else rq
    g = FeatureSet.from_host(sc.dev, rg) if sides in ("both", "gallery") else rg
    same(surface(sc, q, g, only_matrix), want)
    if sides == "both" and not only_matrix:
        # the device forms themselves
        s_dev = sc.score_matrix_device(q, g, rotations=ROT, scales=SCALE)
        np.testing.assert_array_equal(bits(sc.dev.to_host(s_dev)), bits(want["score_matrix"]))
        s_dev, v_dev, p_dev, t_hw = sc.score_matrix_device(q, g, rotations=ROT, scales=SCALE, located=True)
        np.testing.assert_array_equal(bits(sc.dev.to_host(s_dev)), bits(want["located.scores"]))
        np.testing.assert_array_equal(sc.dev.to_host(v_dev), want["located.variant"])
        np.testing.assert_array_equal(pc.unpack(sc.dev.to_host(p_dev)), want["located.yx"])
        assert t_hw.shape == (len(rq), 3, 2) and t_hw.dtype == np.int32
        # without variants the query classes are gathered and cast in one pass
        np.testing.assert_array_equal(bits(sc.score_matrix(q, g)), bits(sc.score_matrix(rq, rg)))
    sc.close()


def check_resident_call_counts(make_scorer, monkeypatch):
    """The resident walk is the host-list walk: the same expansions, preparations and launches, call for call, and the
    closed-form counts of peak_cases.check_call_counts (5 chunks x 4 variant shapes, 5 chunks x 2 classes x 3 variants)."""
    sc = budget_scorer(make_scorer, "fft", "float32")
    rq, rg = pc.ragged_set()
    n = pc.count_calls(monkeypatch, sc.lib)
    runs = []
    for q, g in ((rq, rg), (FeatureSet.from_host(sc.dev, rq), FeatureSet.from_host(sc.dev, rg))):
        per = []
        for call in (lambda: sc.score_matrix(q, g, rotations=ROT, scales=SCALE),
                     lambda: sc.score_matrix_located(q, g, rotations=ROT, scales=SCALE),
                     lambda: sc.locate(q, g, PAIRS[:4], rotations=ROT, scales=SCALE)):
            before = dict(n)
            call()
            per.append({k: n[k] - before[k] for k in n})
        runs.append(per)
    assert runs[0] == runs[1], runs
    assert runs[0][0]["spr_ncc_prepare_gallery"] == 5 * 4 and runs[0][0]["spr_ncc_score"] == 5 * 2 * 3
    sc.close()


# ------------------------------------------------------------------------------------------------ 5. nothing crosses
class Traffic:
    """Wraps the transfers of a backend and records what they carry."""

    def __init__(self, monkeypatch, dev):
        self.down, self.up, self.stacks = [], [], 0
        to_host, to_device, stack = dev.to_host, dev.to_device, dev.stack_to_device

        def down(buf):
            host = to_host(buf)
            self.down.append(tuple(host.shape))
            return host

        def up(array):
            self.up.append((np.asarray(array).dtype, int(np.asarray(array).size)))
            return to_device(array)

        def stacked(items):
            self.stacks += 1
            return stack(items)

        monkeypatch.setattr(dev, "to_host", down, raising=False)
        monkeypatch.setattr(dev, "to_device", up, raising=False)
        monkeypatch.setattr(dev, "stack_to_device", stacked, raising=False)

    def take(self):
        down, up, stacks = self.down, self.up, self.stacks
        self.down, self.up, self.stacks = [], [], 0
        return down, up, stacks


def check_nothing_crosses(make_scorer, monkeypatch, method, storage):
    sc = budget_scorer(make_scorer, method, storage)
    rq, rg = pc.ragged_set()
    nq, ng = len(rq), len(rg)
    smallest = min(a.size for a in rq + rg)
    q, g = FeatureSet.from_host(sc.dev, rq), FeatureSet.from_host(sc.dev, rg)
    fused = sc.plan(6, (18, 12), (18, 12), dtype=storage).has_peaks
    traffic = Traffic(monkeypatch, sc.dev)
    matrix, vector = (nq, ng), (nq,)
    per_pair = lambda shape: len(shape) in (1, 2) and shape[0] <= nq * ng and (len(shape) == 1 or shape[1] == 2)
    shortlisted = lambda shape: shape in ((nq, K), (nq * K,)) or per_pair(shape)
    calls = {
        "compare_maps": (lambda: similarity.compare_maps(q, g, MATCH, cfg(), scorer=sc), lambda s: s == vector),
        "retrieve": (lambda: similarity.retrieve(q, g, cfg(), k=K, scorer=sc), shortlisted),
        "retrieve_plain": (lambda: similarity.retrieve(q, g, cfg(), k=K, locate=False, scorer=sc), lambda s: s == (nq, K)),
        "retrieve_with_scores": (lambda: similarity.retrieve_with_scores(q, g, cfg(), K, scorer=sc), lambda s: s == matrix or shortlisted(s)),
        "score_matrix": (lambda: sc.score_matrix(q, g, rotations=ROT, scales=SCALE), lambda s: s == matrix),
        "score_matrix_located": (lambda: sc.score_matrix_located(q, g, rotations=ROT, scales=SCALE), lambda s: s == matrix or per_pair(s)),
        "locate": (lambda: sc.locate(q, g, PAIRS, rotations=ROT, scales=SCALE), per_pair),
        "score_matrix_device": (lambda: sc.score_matrix_device(q, g, rotations=ROT, scales=SCALE), lambda s: False),
    }
    for name, (call, allowed) in calls.items():
        call()
        down, up, stacks = traffic.take()
        assert stacks == 0, (name, "stack_to_device was called")
        assert not [u for u in up if u[0] == np.float32 and u[1] >= smallest], (name, up)
        assert all(int(np.prod(s)) < smallest for s in down), (name, down)  # no call carries a whole feature item
        assert all(allowed(s) for s in down), (name, down)
        if name == "compare_maps":
            assert down == [vector]
        if name == "score_matrix":
            assert down == [matrix]
        if name == "retrieve" and fused:
            assert all(s in ((nq, K), (nq * K,)) for s in down), down
    sc.close()


# ------------------------------------------------------------------------------------------------ 6. extractor
def extractor_images(rgb):
    from shoeprint_image_retrieval_amd import synth

    sizes = [(37, 51), (24, 20), (37, 51), (37, 51), (24, 20)]  # three of one class (a full batch of 2 and a partial one), two of another
    grey = [synth.shoeprint_image(31, i, h, w) for i, (h, w) in enumerate(sizes)]
    if not rgb:
        return grey
    return [np.ascontiguousarray(np.stack([a, 255 - a, np.roll(a, 5, axis=1)], axis=-1)) for a in grey[:3]]


def check_extractor(device, lib, rgb):
    """VGG16 features[:2] (a shallow block: the emulated convolutions behind it cost seconds per image), batch_size 2."""
    import extractor_cases

    m = extractor_cases.make_model(2, device, lib, batch_size=2)
    images = extractor_images(rgb)
    with contextlib.redirect_stderr(io.StringIO()) as host_err:
        want = m.get_multiple_feature_maps(images)
    for source in (images, DeviceImages.from_host(device, images)):
        with contextlib.redirect_stderr(io.StringIO()) as err:
            fs = m.get_multiple_feature_maps_device(source)
        assert isinstance(fs, FeatureSet) and len(fs) == len(images)
        assert err.getvalue() == host_err.getvalue() and "features" in err.getvalue()  # the same progress lines
        got = fs.to_host_list()
        for a, b in zip(want, got):
            assert a.shape == b.shape and b.dtype == np.float32 and b.flags["C_CONTIGUOUS"]
            np.testing.assert_array_equal(bits(a), bits(b))
        assert list(fs.groups()) == list(similarity._group_by_shape(want))
    back = DeviceImages.from_host(device, images).to_host_list()
    assert all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(back, images))
    with pytest.raises(ValueError, match="grey"):
        m.get_multiple_feature_maps_device([np.zeros((4, 4, 2), np.uint8)])
    with pytest.raises(ValueError, match="out is"):
        m.extract_device(device.to_device(np.stack(images[:1])), in_channels=3 if rgb else 1, out=device.zeros((1, 2, 3, 4)))
    m.close()


def check_extractor_shared_feature_shape(device, lib):
    """Image classes whose features share a shape lie in one feature class: behind the first max-pool (features[:5]) a
    25 x 21 image gives what a 24 x 20 one gives, 12 x 10.  Items keep the caller's order."""
    import extractor_cases
    from shoeprint_image_retrieval_amd import synth

    m = extractor_cases.make_model(5, device, lib, batch_size=2)
    images = [synth.shoeprint_image(32, 0, 24, 20), synth.shoeprint_image(32, 1, 25, 21), synth.shoeprint_image(32, 2, 24, 20)]
    with contextlib.redirect_stderr(io.StringIO()):
        want = m.get_multiple_feature_maps(images)
        fs = m.get_multiple_feature_maps_device(images, progress=False)
    assert want[0].shape == want[1].shape and len(fs.classes) == 1 and list(fs.classes[0][1]) == [0, 2, 1]
    for a, b in zip(want, fs.to_host_list()):
        np.testing.assert_array_equal(bits(a), bits(b))
    m.close()


# ------------------------------------------------------------------------------------------------ 7. loader
def check_loader(config, resizer):
    """Every step of the Dataloader with device_resize + device_resident against the keys-off loader: DeviceImages whose
    to_host_list() is the Pillow list byte for byte, the same matches and blocks."""
    from shoeprint_image_retrieval_amd.dataloader import Dataloader

    on = dict(config, mi355x=dict(config.get("mi355x", {}), device_resize=True, device_resident=True))
    with contextlib.redirect_stdout(io.StringIO()):
        plain, device = Dataloader(config), Dataloader(on, resizer=resizer)
    assert device.scales == plain.scales and device.blocks == plain.blocks and device.clusters == plain.clusters
    steps = 0
    for (q0, g0, m0, b0), (q1, g1, m1, b1) in zip(plain, device):
        assert (m0, b0) == (m1, b1)
        for want, got in ((q0, q1), (g0, g1)):
            assert isinstance(got, DeviceImages) and len(got) == len(want)
            assert [s for s, _, _ in got.classes] == list(dict.fromkeys(tuple(a.shape) for a in want))  # first appearance
            back = got.to_host_list()
            for a, b in zip(want, back):
                a8 = np.ascontiguousarray(a, dtype=np.uint8)
                assert b.dtype == np.uint8 and a8.shape == b.shape and a8.tobytes() == b.tobytes()
        steps += 1
    assert steps == plain.num_clusters
    with pytest.raises(StopIteration):
        next(device)
    # device_resident without device_resize changes nothing about the loader: lists, as ever
    with contextlib.redirect_stdout(io.StringIO()):
        lists = Dataloader(dict(config, mi355x=dict(device_resident=True)))
    assert isinstance(next(lists)[0], list)
    return device


# ------------------------------------------------------------------------------------------------ 9. config
def check_config():
    from shoeprint_image_retrieval_amd.config import MI355X_DEFAULTS, normalise

    assert MI355X_DEFAULTS["device_resident"] is False and MI355X_DEFAULTS["max_feature_gib"] == 64
    extra = normalise({})["mi355x"]
    assert extra["device_resident"] is False and extra["max_feature_gib"] == 64
    extra = normalise({"mi355x": {"device_resident": True, "max_feature_gib": 0}})["mi355x"]
    assert extra["device_resident"] is True and extra["max_feature_gib"] == 0
    assert normalise({"mi355x": {"max_feature_gib": 1.5}})["mi355x"]["max_feature_gib"] == 1.5
    for bad in (1, 0, "true", None):
        with pytest.raises(ValueError, match="device_resident"):
            normalise({"mi355x": {"device_resident": bad}})
    for bad in (-1, -0.5, "64", True, None):
        with pytest.raises(ValueError, match="max_feature_gib"):
            normalise({"mi355x": {"max_feature_gib": bad}})
