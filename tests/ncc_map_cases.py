"""Every-pixel and planted-peak checks of the FFT NCC kernels, shared by the CPU-emulation runner (test_emu_ncc_maps.py, not
gpu) and the MI355X runner (test_gpu_ncc_maps.py, gpu).

A score is the maximum over pixels of the channel sum, so a wrong pixel below the maximum never reaches a score test.  Two
kinds of check close that gap for every kernel instance of kEntries (csrc/ncc_fft.hip) and both of its variants:

A. check_maps: all C x ih x iw values of spr_ncc_maps against the float64 oracle on exactly the values the kernel is given;
B. check_sweep: one gallery item per planted position (every row at three columns, every column at three rows), scored
   through spr_ncc_score - the accumulators, the lane / wave / workgroup maximum and the 1/sigma slot order, which the maps
   branch does not exercise.  A failure names the planted rows and columns of the pairs that are off.

Scorers are made with crop=0: the shapes below are the kernels' own (cropped) sizes.
"""

import functools
from typing import NamedTuple

import numpy as np

from oracle import ncc_oracle as oracle
from parity_cases import TIGHT
from shoeprint_image_retrieval_amd import _lib, synth

# Largest errors, the bound being TIGHT = 5e-6 everywhere (each check prints its own figure):
#   CPU emulation: maps 2.0e-7 per pixel (5x5 on 127x61, 192x96 four-wave), sweep scores 6.0e-7 (5x5 on 16x12)
#   MI355X:        not measured yet - no run of test_gpu_ncc_maps.py has been made on the hardware

INSTANCES = ("32x16", "32x32", "48x24", "64x32", "64x64", "96x48", "128x64", "128x128", "192x96/6", "192x96/4", "256x128",
             "384x192")  # the twelve entries of kEntries; 192x96 exists on six waves (ncc_pair6.hip) and on four


class MapCase(NamedTuple):
    t: tuple            # template (th, tw)
    i: tuple            # search map (ih, iw)
    inst: str           # the kernel instance the plan must take (its grid is asserted through plan.fft_size)
    channels: int = 3
    method: str = "fft"
    env: tuple = ()     # ((name, value), ...) set while the scorer and its plan are made and run
    dtype: str = "float32"
    direct: bool = True  # does method="direct" accept the shape (it refuses maps beyond its LDS / strip limits)

    @property
    def grid(self):
        return tuple(int(v) for v in self.inst.split("/")[0].split("x"))

    @property
    def id(self):
        tag = f"{self.t[0]}x{self.t[1]}-on-{self.i[0]}x{self.i[1]}@{self.inst.replace('/', '-')}"
        if self.method != "fft":
            tag += "," + self.method
        if self.dtype != "float32":
            tag += "," + self.dtype
        return tag + "".join(f",{k[8:]}={v}" for k, v in self.env)


_FOUR = (("SPR_NCC_SIX", "0"),)
_BIG = (("SPR_NCC_FORCE_BIG", "1"),)
_SIX_SHAPES = [((124, 60), (124, 60)),  # the headline shape (conv3_3 of a 512 x 256 print): the prep's slot-order 1/sigma path
               ((9, 7), (126, 64)),     # every row and column the six-wave kernel owns; two-sweep 1/sigma (tables beyond LDS)
               ((93, 37), (106, 48))]

# One case per kernel instance and variant (tuned: kept outputs and row rounds within KW_A x RR_A, see fill_geometry).
BASE_CASES = [
    MapCase((8, 6), (16, 8), "32x16"),            # tuned
    MapCase((9, 5), (16, 12), "32x16"),           # general
    MapCase((7, 9), (20, 24), "32x32"),
    MapCase((28, 12), (28, 12), "48x24"),         # tuned: the cropped ResNet layer3 / conv5_3 shape
    MapCase((26, 13), (29, 11), "48x24"),
    MapCase((10, 6), (40, 20), "48x24"),          # general
    MapCase((40, 18), (40, 18), "64x32"),         # general
    MapCase((12, 6), (56, 28), "64x32"),          # general
    MapCase((9, 5), (50, 14), "64x32"),           # one kept output, two row rounds
    MapCase((36, 36), (36, 36), "64x64"),
    MapCase((12, 27), (13, 26), "64x64"),         # template wider than tall, and larger than the map
    MapCase((9, 9), (56, 56), "64x64"),
    MapCase((60, 28), (60, 28), "96x48"),
    MapCase((9, 7), (90, 44), "96x48"),
    MapCase((70, 30), (70, 30), "128x64"),
    MapCase((9, 7), (120, 60), "128x64"),
    MapCase((66, 46), (66, 46), "128x128"),
    MapCase((9, 9), (120, 90), "128x128"),   # over 64 columns: the plain table scan, not the blocked one
    *[MapCase(t, i, "192x96/6") for t, i in _SIX_SHAPES],
    MapCase((86, 46), (116, 66), "192x96/4"),
    MapCase((9, 7), (126, 80), "192x96/4"),  # over 64 columns
    *[MapCase(t, i, "192x96/4", env=_FOUR) for t, i in _SIX_SHAPES],
    # a search map whose two float64 tables exceed LDS: this grid with its working set in the global workspace, reached
    # without any override (its column pass once stored nothing: E = 12 registers on TG = 16 lanes is a single
    # sub-transform set, and group_fft called the storing sink only per set of a multi-set transform)
    MapCase((9, 7), (140, 92), "192x96/4", direct=False),
    MapCase((96, 66), (96, 66), "256x128"),
    MapCase((9, 7), (180, 120), "256x128", direct=False),
    MapCase((200, 100), (200, 100), "384x192", channels=1, direct=False),
    MapCase((200, 124), (200, 124), "384x192", channels=1, direct=False),  # over 108 columns: the other accumulator layout
]

# method="fft_pow2" on every case whose grid then changes
POW2_CASES = [
    MapCase((28, 12), (28, 12), "64x32", method="fft_pow2"),
    MapCase((26, 13), (29, 11), "64x32", method="fft_pow2"),
    MapCase((60, 28), (60, 28), "128x64", method="fft_pow2"),
    MapCase((9, 7), (90, 44), "128x64", method="fft_pow2"),
    *[MapCase(t, i, "256x128", method="fft_pow2") for t, i in _SIX_SHAPES],
    MapCase((86, 46), (116, 66), "256x128", method="fft_pow2"),
    MapCase((9, 7), (126, 80), "256x128", method="fft_pow2"),
]

# 16-bit storage: the oracle runs on the rounded values
STORAGE_CASES = [MapCase(t, i, inst, dtype=d) for t, i, inst in (((124, 60), (124, 60), "192x96/6"), ((9, 7), (90, 44), "96x48"))
                 for d in ("bfloat16", "float16")]

# Variant boundaries: same template and rows, iw = EW * KW_A (the last width of the tuned variant) and one more (general).
# Rows are chosen within the tuned variant's row rounds, templates so that the pair stays on its grid.
BOUNDARY_PAIRS = [
    (MapCase((3, 3), (12, 8), "32x16"), MapCase((3, 3), (12, 9), "32x16")),
    (MapCase((7, 9), (20, 16), "32x32"), MapCase((7, 9), (20, 17), "32x32")),
    (MapCase((5, 5), (32, 12), "48x24"), MapCase((5, 5), (32, 13), "48x24")),
    (MapCase((9, 18), (30, 16), "64x32"), MapCase((9, 18), (30, 17), "64x32")),
    (MapCase((9, 9), (40, 32), "64x64"), MapCase((9, 9), (40, 33), "64x64")),
    (MapCase((9, 7), (70, 30), "96x48"), MapCase((9, 7), (70, 31), "96x48")),
    (MapCase((9, 34), (62, 32), "128x64"), MapCase((9, 34), (62, 33), "128x64")),
    (MapCase((9, 9), (60, 64), "128x128"), MapCase((9, 9), (60, 65), "128x128")),
    (MapCase((5, 5), (127, 60), "192x96/4"), MapCase((5, 5), (127, 61), "192x96/4")),
    (MapCase((9, 7), (126, 64), "256x128", method="fft_pow2"), MapCase((9, 7), (126, 65), "256x128", method="fft_pow2")),
]

# SPR_NCC_FORCE_BIG=1: the working set in the plan's global workspace on shapes that also fit LDS.  (lds, big): the maps of
# `big` must equal those of `lds` bit for bit where both run the same instance; the six-wave kernel has no workspace mode,
# so the headline shape is compared with its four-wave run.
FORCE_BIG_CASES = [
    (MapCase((28, 12), (28, 12), "48x24"), MapCase((28, 12), (28, 12), "48x24", env=_BIG)),
    (MapCase((36, 36), (36, 36), "64x64"), MapCase((36, 36), (36, 36), "64x64", env=_BIG)),
    (MapCase((60, 28), (60, 28), "96x48"), MapCase((60, 28), (60, 28), "96x48", env=_BIG)),
    (MapCase((124, 60), (124, 60), "192x96/4", env=_FOUR), MapCase((124, 60), (124, 60), "192x96/4", env=_BIG)),
]

ALL_CASES = BASE_CASES + POW2_CASES + STORAGE_CASES + [c for pair in BOUNDARY_PAIRS + FORCE_BIG_CASES for c in pair]


def for_emu(cases):
    return [c for c in cases if getattr(c, "emu", True)]  # (only a sweep is too slow for the emulation)


# ------------------------------------------------------------------------------------------------- A. every pixel
@functools.lru_cache(maxsize=None)
def _inputs(t, i, channels, dtype):
    """(query, gallery) as the kernel stores them, their float32 values, and the oracle maps - computed once per shape and
    storage type, shared by every run of that shape, read-only."""
    rng = np.random.default_rng([17, *t, *i])
    q = rng.standard_normal((channels, *t), dtype=np.float32)
    g = rng.standard_normal((channels, *i), dtype=np.float32)
    if channels > 1:
        g[1] = 0.0       # dead gallery channel: flag set, 1/sigma = 0
    if channels > 2:
        q[2] = 0.75      # constant non-zero query channel: a zero template after centring
    if dtype == "bfloat16":
        q, g = synth.bfloat16_bits(q), synth.bfloat16_bits(g)
        qf, gf = synth.from_bfloat16_bits(q), synth.from_bfloat16_bits(g)
    elif dtype == "float16":
        q, g = q.astype(np.float16), g.astype(np.float16)
        qf, gf = q.astype(np.float32), g.astype(np.float32)
    else:
        qf, gf = q, g
    want = oracle.ncc_maps(qf, gf, precise=True)
    for a in (q, g, want):
        a.flags.writeable = False
    return q, g, want


def _set_env(monkeypatch, case):
    for name in ("SPR_NCC_SIX", "SPR_NCC_FORCE_BIG"):
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env:
        monkeypatch.setenv(name, value)


def make_plan(make_scorer, case, monkeypatch, method=None):
    """A fresh scorer and the case's plan (the mode is fixed when the plan is created), with the grid asserted."""
    _set_env(monkeypatch, case)
    sc = make_scorer(method or case.method)
    dtype = {"float32": np.float32, "float16": np.float16, "bfloat16": "bfloat16"}[case.dtype]
    plan = sc.plan(case.channels, case.t, case.i, dtype=dtype)
    if method is None:
        assert plan.method == _lib.NCC_FFT and plan.fft_size == case.grid, (case.id, plan.fft_size)
    return sc, plan


def run_maps(make_scorer, case, monkeypatch, method=None):
    """The kernel's maps of the case and their largest error against the oracle."""
    q, g, want = _inputs(case.t, case.i, case.channels, case.dtype)
    sc, plan = make_plan(make_scorer, case, monkeypatch, method)
    dev = sc.dev
    pq = sc.prepare_queries(plan, dev.to_device(q[None]))
    pg = sc.prepare_gallery(plan, dev.to_device(g[None]))
    got = dev.to_host(sc.ncc_maps_device(plan, pq, pg))
    sc.close()
    assert got.shape == want.shape and got.dtype == np.float32
    return got, want, plan


def assert_maps(got, want, label, tol=TIGHT):
    err = np.abs(got.astype(np.float64) - want)
    err[~np.isfinite(err)] = np.inf
    worst = float(err.max())
    print(f"[ncc maps] {label}: max |err| = {worst:.3g}")
    if not worst <= tol:
        bad = np.argwhere(~(err <= tol))
        c, y, x = (int(v) for v in np.unravel_index(int(err.argmax()), err.shape))
        raise AssertionError(
            f"{label}: {len(bad)} of {err.size} pixels beyond {tol:g}; worst {worst:.3g} at channel {c} row {y} column {x} "
            f"(got {got[c, y, x]!r}, want {want[c, y, x]!r}); rows {sorted({int(b[1]) for b in bad})[:40]}, "
            f"columns {sorted({int(b[2]) for b in bad})[:40]}, channels {sorted({int(b[0]) for b in bad})}")
    return worst


def check_maps(make_scorer, case, monkeypatch):
    got, want, plan = run_maps(make_scorer, case, monkeypatch)
    if case.channels > 2:
        assert not got[1].any() and not got[2].any(), f"{case.id}: dead channels must give exact zeros"
    assert_maps(got, want, case.id)
    return got, plan


def check_direct(make_scorer, case, monkeypatch):
    """method="direct" on the same inputs, where its plan accepts the shape; the table says where it does not."""
    try:
        got, want, plan = run_maps(make_scorer, case, monkeypatch, method="direct")
    except _lib.SprError as e:
        assert e.code == _lib.SPR_ERR_UNSUPPORTED and not case.direct, f"{case.id}: direct refused ({e})"
        return
    assert case.direct, f"{case.id}: the table expects the direct method to refuse this shape"
    assert plan.method == _lib.NCC_DIRECT
    assert_maps(got, want, case.id + ",direct")


def check_boundary_pair(make_scorer, pair, monkeypatch):
    tuned, general = pair
    assert tuned.t == general.t and tuned.i[0] == general.i[0] and tuned.i[1] + 1 == general.i[1] and tuned.inst == general.inst
    _, plan_t = check_maps(make_scorer, tuned, monkeypatch)
    _, plan_g = check_maps(make_scorer, general, monkeypatch)
    # the 1/sigma slice grows with the kept outputs: a pair that no longer flips the variant fails here
    assert plan_g.gallery_item_bytes > plan_t.gallery_item_bytes, (tuned.id, plan_t.gallery_item_bytes, plan_g.gallery_item_bytes)


def check_force_big(make_scorer, pair, monkeypatch):
    lds, big = pair
    got_big, plan_big = check_maps(make_scorer, big, monkeypatch)
    got_lds, plan_lds = check_maps(make_scorer, lds, monkeypatch)
    if plan_big.fft_size == plan_lds.fft_size:
        np.testing.assert_array_equal(got_big, got_lds, err_msg=big.id)


def check_case_table(make_scorer, monkeypatch, cases):
    """Every case lands on the grid it names, and together the cases reach each of the twelve instances.  The ABI does not
    say which 192 x 96 kernel a plan took; the six-wave prepared layouts differ in size from the four-wave ones, so a
    six-wave case whose sizes do not change under SPR_NCC_SIX=0 is not on the six-wave kernel."""
    reached = set()
    for case in cases:
        sc, plan = make_plan(make_scorer, case, monkeypatch)
        if case.inst == "192x96/6":
            assert not case.env and case.i[0] <= 126 and case.i[1] <= 64, case.id
            sc4, plan4 = make_plan(make_scorer, case._replace(env=_FOUR), monkeypatch)
            assert plan4.fft_size == plan.fft_size, case.id
            assert (plan4.query_item_bytes, plan4.gallery_item_bytes) != (plan.query_item_bytes, plan.gallery_item_bytes), case.id
            sc4.close()
        elif case.inst == "192x96/4":
            assert case.env or case.i[0] > 126 or case.i[1] > 64, case.id
        sc.close()
        reached.add(case.inst)
    assert reached == set(INSTANCES), sorted(set(INSTANCES) - reached)


# ------------------------------------------------------------------------------------------------- B. planted peaks
class SweepCase(NamedTuple):
    t: tuple
    i: tuple
    inst: str
    positions: int
    env: tuple = ()
    emu: bool = True

    @property
    def grid(self):
        return tuple(int(v) for v in self.inst.split("/")[0].split("x"))

    @property
    def id(self):
        return f"{self.t[0]}x{self.t[1]}-on-{self.i[0]}x{self.i[1]}@{self.inst.replace('/', '-')}" + \
            "".join(f",{k[8:]}={v}" for k, v in self.env)


SWEEP_CASES = [
    SweepCase((5, 5), (16, 12), "32x16", 75),
    SweepCase((9, 9), (56, 56), "64x64", 327),
    SweepCase((9, 7), (90, 44), "96x48", 393),
    SweepCase((9, 7), (126, 64), "192x96/6", 561),
    SweepCase((9, 7), (126, 80), "192x96/4", 609),
    SweepCase((9, 7), (180, 120), "256x128", 891, emu=False),
    SweepCase((9, 7), (90, 44), "96x48", 393, env=_BIG),
]
N_TEMPLATES = 3   # an odd query count leaves the second half of the last six-wave workgroup idle
MARGIN = 1e-3     # a good pair's planted pixel beats every other pixel of its oracle map by this much
GOOD_SHARE = 0.85


def sweep_positions(ih, iw):
    pos = {(y, x) for y in range(ih) for x in (0, iw // 2, iw - 1)} | {(y, x) for y in (0, ih // 2, ih - 1) for x in range(iw)}
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def _sweep_inputs(t, i):
    """Templates, one gallery item per planted position, the oracle's [3, n] scores, and which matched pairs are good -
    computed once per shape, shared by every run of that shape, read-only.  The conditions on the inputs are asserted
    here, from the oracle alone."""
    (th, tw), (ih, iw) = t, i
    rng = np.random.default_rng([23, th, tw, ih, iw])
    templates = rng.standard_normal((N_TEMPLATES, th, tw), dtype=np.float32)
    pos = sweep_positions(ih, iw)
    items = (0.05 * rng.standard_normal((len(pos), ih, iw))).astype(np.float32)
    for k, (y, x) in enumerate(pos):
        y0, x0 = y - th // 2, x - tw // 2   # the template's corner when its 'same'-mode centre lies on (y, x)
        ya, yb, xa, xb = max(y0, 0), min(y0 + th, ih), max(x0, 0), min(x0 + tw, iw)
        items[k, ya:yb, xa:xb] += templates[k % N_TEMPLATES, ya - y0:yb - y0, xa - x0:xb - x0]
    want = np.empty((N_TEMPLATES, len(pos)))
    good = np.zeros(len(pos), dtype=bool)
    for q in range(N_TEMPLATES):
        maps = oracle.ncc_maps(np.broadcast_to(templates[q], items.shape[:1] + t).copy(), items, precise=True)
        want[q] = np.maximum(maps.reshape(len(pos), -1).max(axis=1), 0.0)
        for k in range(q, len(pos), N_TEMPLATES):
            flat = maps[k].ravel()
            planted = pos[k][0] * iw + pos[k][1]
            good[k] = flat.argmax() == planted and flat[planted] - np.delete(flat, planted).max() >= MARGIN
    label = f"{th}x{tw} on {ih}x{iw}"
    assert good.mean() >= GOOD_SHARE, f"{label}: only {good.mean():.3f} of the planted peaks are the oracle's clear maximum"
    rows = {pos[k][0] for k in np.flatnonzero(good)}
    cols = {pos[k][1] for k in np.flatnonzero(good)}
    assert rows == set(range(ih)) and cols == set(range(iw)), f"{label}: good pairs miss rows / columns"
    for a in (templates, items, want, good):
        a.flags.writeable = False
    return templates, items, pos, want, good


def check_sweep(make_scorer, case, monkeypatch, tol=TIGHT):
    templates, items, pos, want, good = _sweep_inputs(case.t, case.i)
    assert len(pos) == case.positions
    _set_env(monkeypatch, case)
    sc = make_scorer("fft")
    assert sc.plan(1, case.t, case.i).fft_size == case.grid, case.id
    got = sc.score_matrix([a[None] for a in templates], [a[None] for a in items])
    sc.close()
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want)
    err[~np.isfinite(err)] = np.inf
    worst = float(err.max())
    print(f"[ncc sweep] {case.id}: {len(pos)} positions, {int(good.sum())} good, max |err| = {worst:.3g}")
    if not worst <= tol:
        bad = np.argwhere(~(err <= tol))
        matched = [(int(q), int(k)) for q, k in bad if k % N_TEMPLATES == q]
        lines = [f"query {q} item {k} planted at row {pos[k][0]} column {pos[k][1]}"
                 f"{'' if k % N_TEMPLATES == q else ' (of another template)'}: got {got[q, k]:.7f} want {want[q, k]:.7f}"
                 for q, k in sorted(((int(q), int(k)) for q, k in bad), key=lambda qk: -err[qk])[:25]]
        raise AssertionError(
            f"{case.id}: {len(bad)} of {err.size} scores beyond {tol:g}, worst {worst:.3g}; matched pairs off: planted rows "
            f"{sorted({pos[k][0] for _, k in matched})}, planted columns {sorted({pos[k][1] for _, k in matched})}\n" + "\n".join(lines))
    return worst
