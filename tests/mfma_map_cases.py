"""Every-pixel, planted-peak and guard-band checks of the matrix-core NCC scorer (csrc/ncc_mfma.hip: methods "mfma" and
"mfma_f32"), shared by the CPU-emulation runner (test_emu_mfma_maps.py, not gpu) and the MI355X runner
(test_gpu_mfma_maps.py, gpu).

A score is the maximum over positions of a channel sum, so a wrong pixel below the maximum never reaches a score test, and
the one pair of half-normal features that parity_cases / mfma_f32_cases look at per pixel is held to 1e-4 ... 2e-3 only.

A. check_maps: all C x ih x iw values of spr_ncc_maps against the float64 oracle on exactly the values the kernel is given
   (the rounded ones for 16-bit storage) - the four forms of the method (bfloat16 exact, bfloat16 split, float16, float32 as
   hi + lo), both instances (MCfg<28, 12> and MCfg<28, 12, 30, 8>), both gallery preparation kernels, maps riding on offsets.
B. check_peaks: one gallery item per planted position of the frame (position p carries template p % 67), 67 templates (a full 64-query block and a block of three
   with idle waves), the whole 67 x N matrix of spr_ncc_score - the maximum over 21 tiles x 16 positions, the query slots of a
   wave and the correction matrix of the exact form, which the maps branch does not exercise.  A failure names the planted
   rows and columns and the query slots (wave, lane) of the matched pairs that are off.
C. check_guarded: every scorer method through the raw C ABI with the inputs, both prepared buffers, a score matrix with
   ld > n_gallery and col0 > 0, the maps of one pair and the ranks between random bands, the interiors pre-filled with three
   different bytes: bands and padding columns untouched, outputs bit-identical whatever the fill (the running maximum
   swallows NaN, so a NaN fill alone cannot show a read of bytes the preparation never wrote).

Bounds.  16-bit forms: TIGHT (5e-6) against the oracle.  "mfma_f32": the kernel is held to TIGHT against restate_f32 - the
scheme itself in numpy (both maps centred in float32 about the float64-summed mean as the prep kernels do, each split into
hi + lo bfloat16, hi*hi + hi*lo + lo*hi exact in float64, minus mean(t_hi + t_lo) * S1, over the oracle's own float64 window
statistics) - which bounds the kernel's float32 accumulation and catches a dropped or mis-weighted product, and to the
contract TOL (1e-4) against the oracle.  How far the scheme itself is from the oracle is printed per case: with one live
tap row or a handful of taps the 2^-17 per operand of hi + lo does not average out, and the figure passes 5e-6.

Scorers of A and B are made with crop=0: the shapes are the kernels' own (cropped) sizes.  C uses the default crop of 2.
"""

import functools
from typing import NamedTuple

import numpy as np

import ncc_map_cases as nm
from layer_cases import run_guarded
from ncc_map_cases import assert_maps
from oracle import ncc_oracle as oracle
from parity_cases import TIGHT, TOL
from shoeprint_image_retrieval_amd import _lib, synth
from shoeprint_image_retrieval_amd.similarity import _METHODS

# Largest errors measured (each check prints its own figure).  emulation = the CPU twin of the kernels (k-ordered float32
# accumulation); MI355X = the gfx950 build on the hardware.  MI355X: NOT MEASURED YET - no run of test_gpu_mfma_maps.py has been
# made on the hardware; every figure below is the emulation's.
#   A. maps, max |kernel - oracle| per pixel (bound TIGHT = 5e-6)          emulation      MI355X
#      bf16 exact: 1.2e-7 (3x3 on 28x12), 17 channels 8.9e-8, offsets 100 / 1000 2.2e-8        not measured
#      bf16 split: 2.2e-6 (3x3 on 28x12; 1.6e-6 5x5 on 9x7, 1.5e-6 9x7 on 28x12), offsets 7.9e-7   not measured
#      float16:    1.8e-7 (3x3 on 28x12), offset 100 1.1e-8                                   not measured
#      mfma_f32, |kernel - restatement| (bound TIGHT): 2.5e-7 (28x12 on 28x12), offsets 1.2e-7   not measured
#      mfma_f32, |kernel - oracle| (bound TOL = 1e-4): 6.0e-6 (3x3 on 28x12), 7.4e-6 at offset 1000   not measured
#   mfma_f32, |restatement - oracle| per shape, 3 channels (a property of the scheme and of the inputs, not of the hardware):
#      28x12 on 28x12 7.5e-7 (17 channels 1.1e-6)   30x16 on 28x12 5.8e-7   29x13 on 28x12 7.4e-7   9x7 on 28x12 2.9e-6 (17 ch. 2.3e-6)
#      3x3 on 28x12 6.1e-6   1x1 on 28x12 0   28x12 on 17x5 5.4e-7   5x5 on 9x7 3.2e-6   30x16 on 5x3 7.9e-7   2x16 on 28x1 1.8e-6
#      28x12 on 28x12 at offset 100 8.1e-7, at offset 1000 7.4e-6 - of which 7.2e-6 is one ulp (6.1e-5) between the float32 mean
#      numpy's pairwise sum gives the oracle and the correctly rounded one of the kernels' float64 sum, 1.3e-6 the hi + lo split
#   B. planted peaks, max |score - oracle| (bound TIGHT)         emulation (every 7th position)      MI355X (all positions)
#      9x7 on 28x12: bf16 exact 2.0e-7, bf16 split 2.2e-6, float16 3.2e-7                              not measured
#      9x7 on 28x12 mfma_f32: restatement 5.0e-7 (TIGHT), oracle 4.3e-6 (TOL), scheme 4.2e-6            not measured
#      28x12 on 28x12 bf16 exact 3.4e-7, 30x16 on 28x12 float16 4.9e-7, 9x7 on 17x5 bf16 exact 2.5e-7   not measured
#      every planted peak good (48 of 48; 29 of 29 on 17x5)
#   C. guard bands, emulation: bands and padding untouched, outputs bit-identical across the fills, scores within 1.6e-6 of the
#      oracle (mfma_f32; the others 6.4e-7 and below).  MI355X: not measured.

ENV_NAMES = ("SPR_NCC_MFMA_EXACT", "SPR_MFMA_PREP", "SPR_MFMA_F32_MEAN", "SPR_NCC_MAX_TILES", "SPR_NCC_FORCE_BIG", "SPR_NCC_SIX")

# form -> (method asked for, storage type, environment while the plan is made)
FORMS = {
    "bf16-exact": ("mfma", "bfloat16", (("SPR_NCC_MFMA_EXACT", "1"),)),
    "bf16-split": ("mfma", "bfloat16", (("SPR_NCC_MFMA_EXACT", "0"),)),
    "f16": ("mfma", "float16", ()),          # half-precision maps: the exact form only
    "f32": ("mfma_f32", "float32", ()),
}
_NP_DTYPE = {"float32": np.float32, "float16": np.float16, "bfloat16": "bfloat16"}
TUNED = ((28, 12), (28, 12))  # template and map of MCfg<28, 12>; every other shape runs MCfg<28, 12, 30, 8>
NPOS = 28 * 12                # the frame of positions of both instances


def _align(n, a=256):
    return (n + a - 1) // a * a


def _pad16(c):
    return (c + 15) // 16 * 16


class MapCase(NamedTuple):
    t: tuple            # template (th, tw)
    i: tuple            # search map (ih, iw)
    form: str
    channels: int = 3
    prep: str = ""      # SPR_MFMA_PREP: "1" the wave kernel (default), "0" the table kernel
    offset: float = 0.0

    @property
    def tuned(self):
        return (self.t, self.i) == TUNED

    @property
    def method(self):
        return FORMS[self.form][0]

    @property
    def dtype(self):
        return FORMS[self.form][1]

    @property
    def env(self):
        return FORMS[self.form][2] + ((("SPR_MFMA_PREP", self.prep),) if self.prep else ())

    @property
    def id(self):
        tag = f"{self.t[0]}x{self.t[1]}-on-{self.i[0]}x{self.i[1]},{self.form},{self.channels}ch"
        if self.prep:
            tag += f",prep={self.prep}"
        if self.offset:
            tag += f",offset={self.offset:g}"
        return tag


def expected_item_bytes(case):
    """(query, gallery) bytes of one prepared item, from the layouts ncc_mfma.hip documents: template rows of FH x 16 taps
    (FH = 28 tuned, 30 general; two planes for float32 maps) and {a, a * mean} per channel, the exact form's
    U[position][16-padded channel] behind them; per gallery channel b, b * S and the pixel words of the 336 positions, the exact
    form's V and the channel means behind them.  The instance shows in the query size, the form in both."""
    fh = 28 if case.tuned else 30
    rows, c, cp = fh * 16 * 2, case.channels, _pad16(case.channels)
    exact = case.form in ("bf16-exact", "f16")
    if case.form == "f32":
        qb = c * (2 * rows + 8)
    else:
        qb = c * (rows + 8) + (4 * NPOS * cp if exact else 0)
    gb = c * 3 * 4 * NPOS + (4 * (NPOS + 1) * cp if exact else 0)
    return _align(qb), _align(gb)


_GENERAL_SHAPES = [((30, 16), (28, 12)),   # the largest template
                   ((29, 13), (28, 12)),
                   ((9, 7), (28, 12)),
                   ((3, 3), (28, 12)),
                   ((1, 1), (28, 12)),
                   ((28, 12), (17, 5)),    # a map smaller than the frame: the spare positions must not leak
                   ((5, 5), (9, 7)),
                   ((30, 16), (5, 3)),     # a template larger than the map
                   ((2, 16), (28, 1))]
_ON_FRAME = [TUNED, ((9, 7), (28, 12))]  # 17 channels (the exact form pads U / V to 16) and both prep kernels on these

MAP_CASES = [MapCase(t, i, form) for form in FORMS for t, i in [TUNED] + _GENERAL_SHAPES]
WIDE_CASES = [MapCase(t, i, form, channels=17) for form in FORMS for t, i in _ON_FRAME]
PREP_CASES = [MapCase(t, i, form, prep=p) for form in FORMS for t, i in _ON_FRAME for p in ("1", "0")]
# maps riding on an offset; float16 keeps 11 bits, so 1000 is for bfloat16 (whose exact shift it exercises) and float32
OFFSET_CASES = [MapCase(*TUNED, form, offset=o) for form in FORMS for o in (100.0, 1000.0) if o <= 100.0 or form != "f16"]
ALL_MAP_CASES = MAP_CASES + WIDE_CASES + PREP_CASES + OFFSET_CASES


def set_env(monkeypatch, env):
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)


def make_plan(make_scorer, case, monkeypatch):
    """A fresh scorer and the case's plan (the form is fixed when the plan is created); the method, the instance and the
    form are asserted through the plan's method and item sizes."""
    set_env(monkeypatch, case.env)
    sc = make_scorer(case.method)
    plan = sc.plan(case.channels, case.t, case.i, dtype=_NP_DTYPE[case.dtype])
    want = _lib.NCC_MFMA_F32 if case.form == "f32" else _lib.NCC_MFMA
    assert plan.method == want, (case.id, plan.method)
    # (the instance is a matter of the shape alone; one channel's sizes round to the same multiple of 256 on both instances,
    # so the three-channel plan of the same shape is asked as well)
    for probe in {case, case._replace(channels=3)}:
        p = sc.plan(probe.channels, probe.t, probe.i, dtype=_NP_DTYPE[probe.dtype])
        assert (p.query_item_bytes, p.gallery_item_bytes) == expected_item_bytes(probe), \
            (probe.id, p.query_item_bytes, p.gallery_item_bytes, expected_item_bytes(probe))
    return sc, plan


def check_case_table(make_scorer, monkeypatch, cases):
    """Every case lands on the method, instance and form it names, and together the cases reach both instances in all
    four forms.  The tuned and the general instance must differ in their prepared query size - or the assertion of
    make_plan could not tell them apart."""
    reached = set()
    for case in cases:
        sc, plan = make_plan(make_scorer, case, monkeypatch)
        sc.close()
        probe = case._replace(channels=3)
        other = probe._replace(t=(9, 7)) if case.tuned else probe._replace(t=TUNED[0], i=TUNED[1])
        assert expected_item_bytes(other)[0] != expected_item_bytes(probe)[0], case.id
        reached.add((case.form, case.tuned))
    assert reached == {(form, tuned) for form in FORMS for tuned in (True, False)}, sorted(reached)


# ------------------------------------------------------------------------------------------------- A. every pixel
def _to_storage(a, dtype):
    """(the array as the kernel stores it, its float32 values)"""
    if dtype == "bfloat16":
        bits = synth.bfloat16_bits(a)
        return bits, synth.from_bfloat16_bits(bits)
    if dtype == "float16":
        h = a.astype(np.float16)
        return h, h.astype(np.float32)
    return a, a


@functools.lru_cache(maxsize=None)
def _offset_inputs(t, i, channels, dtype, offset):
    """As ncc_map_cases._inputs (standard-normal maps, a dead gallery channel, a constant non-zero query channel), riding on
    an offset - computed once per shape and storage type, read-only."""
    rng = np.random.default_rng([19, *t, *i, int(offset)])
    q = rng.standard_normal((channels, *t), dtype=np.float32) + np.float32(offset)
    g = rng.standard_normal((channels, *i), dtype=np.float32) + np.float32(offset)
    g[1] = 0.0
    q[2] = 0.75
    (q, qf), (g, gf) = _to_storage(q, dtype), _to_storage(g, dtype)
    want = oracle.ncc_maps(qf, gf, precise=True)
    for a in (q, g, want):
        a.flags.writeable = False
    return q, g, want


def map_inputs(case):
    if case.offset:
        return _offset_inputs(case.t, case.i, case.channels, case.dtype, case.offset)
    return nm._inputs(case.t, case.i, case.channels, case.dtype)


def _bf16(x):
    return synth.from_bfloat16_bits(synth.bfloat16_bits(np.ascontiguousarray(x, dtype=np.float32)))


def _hi_lo(x0):
    """A float32 array as two bfloat16 numbers (round to nearest even, the remainder rounded again), as float64."""
    hi = _bf16(x0)
    lo = _bf16(x0 - hi)  # (exact in float32)
    return hi.astype(np.float64), lo.astype(np.float64)


def _centre_f32(x):
    """Centred in float32 about the mean summed in float64 (ncc_prep_common.h: load_centred)."""
    mean = x.astype(np.float64).mean(axis=(-2, -1), keepdims=True).astype(np.float32)
    return (x - mean).astype(np.float32)


def _windows(img, th, tw):
    """[..., ih, iw, th, tw]: the pixels 'same' mode lays the taps on at every position (zeros outside the map)."""
    pad = [(0, 0)] * (img.ndim - 2) + [(th // 2, th - th // 2 - 1), (tw // 2, tw - tw // 2 - 1)]
    return np.lib.stride_tricks.sliding_window_view(np.pad(img, pad), (th, tw), axis=(-2, -1))


def _statistics(i0, t0):
    """The oracle's float64 statistics: window sums S1, clamped variances, template energies."""
    th, tw = t0.shape[-2:]
    s1, s2 = oracle._window_sums(i0, th, tw)
    var = s2 - np.square(s1) / float(th * tw)
    var[var < 0] = 0
    energy = np.square(t0).sum(axis=(-2, -1), dtype=np.float64)
    return s1, var, energy


def restate_f32(q, g):
    """The scheme of "mfma_f32" on [C, th, tw] against [C, ih, iw] float32 maps, products exact (see the module docstring)."""
    t0, i0 = _centre_f32(np.asarray(q)), _centre_f32(np.asarray(g))
    th, tw = t0.shape[-2:]
    (t_hi, t_lo), (i_hi, i_lo) = _hi_lo(t0), _hi_lo(i0)
    num = np.einsum("cyxuv,cuv->cyx", _windows(i_hi, th, tw), t_hi) + np.einsum("cyxuv,cuv->cyx", _windows(i_lo, th, tw), t_hi) \
        + np.einsum("cyxuv,cuv->cyx", _windows(i_hi, th, tw), t_lo)
    s1, var, energy = _statistics(i0, t0)
    resid = (t_hi + t_lo).sum(axis=(-2, -1)) / float(th * tw)
    num = num - resid[:, None, None] * s1
    with np.errstate(divide="ignore", invalid="ignore"):
        out = num / np.sqrt(var * energy[:, None, None])
    out[~np.isfinite(out)] = 0
    return out


def run_maps(make_scorer, case, monkeypatch):
    q, g, want = map_inputs(case)
    sc, plan = make_plan(make_scorer, case, monkeypatch)
    dev = sc.dev
    pq = sc.prepare_queries(plan, dev.to_device(q[None]))
    pg = sc.prepare_gallery(plan, dev.to_device(g[None]))
    got = dev.to_host(sc.ncc_maps_device(plan, pq, pg))
    sc.close()
    assert got.shape == want.shape and got.dtype == np.float32
    return got, want


def check_maps(make_scorer, case, monkeypatch):
    """Every pixel of the case; returns the largest errors {against the oracle, (f32) the restatement, the scheme's own}."""
    got, want = run_maps(make_scorer, case, monkeypatch)
    assert not got[1].any() and not got[2].any(), f"{case.id}: dead channels must give exact zeros"
    if case.form != "f32":
        return {"oracle": assert_maps(got, want, case.id)}
    q, g, _ = map_inputs(case)
    rest = restate_f32(q, g)
    gap = float(np.abs(rest - want).max())
    print(f"[mfma maps] {case.id}: max |restatement - oracle| = {gap:.3g}")
    return {"scheme": gap,
            "restatement": assert_maps(got, rest, case.id + " against the restatement"),
            "oracle": assert_maps(got, want, case.id + " against the oracle", tol=TOL)}


# ------------------------------------------------------------------------------------------------- B. planted peaks
N_TEMPLATES = 67  # one full 64-query block and a last block of three queries: idle lanes, three idle waves
MARGIN, GOOD_SHARE = nm.MARGIN, nm.GOOD_SHARE


class PeakCase(NamedTuple):
    t: tuple
    i: tuple
    form: str
    emu_stride: int = 7  # the emulation plants every n-th position (row-major): coprime to and below the map's width, so that
                         # every row and every column is still hit (7 on 12 columns, 3 on 5)
    launches: int = 1    # > 1: SPR_NCC_MAX_TILES for that many launches over the gallery, bit-identical to one launch

    @property
    def id(self):
        return f"{self.t[0]}x{self.t[1]}-on-{self.i[0]}x{self.i[1]},{self.form}" + (f",{self.launches}-launches" if self.launches > 1 else "")

    def map_case(self):
        return MapCase(self.t, self.i, self.form, channels=1)


PEAK_CASES = [
    PeakCase((9, 7), (28, 12), "bf16-exact"),
    PeakCase((9, 7), (28, 12), "bf16-split"),
    PeakCase((9, 7), (28, 12), "f16"),
    PeakCase((9, 7), (28, 12), "f32"),
    PeakCase(*TUNED, "bf16-exact"),
    PeakCase((30, 16), (28, 12), "f16"),
    PeakCase((9, 7), (17, 5), "bf16-exact", emu_stride=3),
    PeakCase((9, 7), (28, 12), "bf16-exact", launches=3),
]


@functools.lru_cache(maxsize=None)
def _peak_inputs(t, i, dtype, stride):
    """67 templates and one single-channel gallery item per planted position p = y * iw + x (0.05 * noise plus template
    p % 67 laid so that its 'same'-mode centre falls on the position: the construction of ncc_map_cases._sweep_inputs; the
    item of a position is the same whatever the stride, and a stride of 7 still reaches both query blocks), as stored; the
    oracle's [67, N] scores on the stored values; which matched pairs are good.  The conditions on the inputs are asserted
    here, from the oracle alone.  Computed once per shape, storage type and stride, read-only."""
    (th, tw), (ih, iw) = t, i
    rng = np.random.default_rng([29, th, tw, ih, iw])
    templates = rng.standard_normal((N_TEMPLATES, th, tw), dtype=np.float32)
    noise = (0.05 * rng.standard_normal((ih * iw, ih, iw))).astype(np.float32)  # (the same item at a position whatever the stride)
    pos = [(p // iw, p % iw) for p in range(0, ih * iw, stride)]
    owner = np.arange(0, ih * iw, stride) % N_TEMPLATES  # the template each item carries
    items = noise[::stride].copy()
    for k, (y, x) in enumerate(pos):
        y0, x0 = y - th // 2, x - tw // 2   # the template's corner when its 'same'-mode centre lies on (y, x)
        ya, yb, xa, xb = max(y0, 0), min(y0 + th, ih), max(x0, 0), min(x0 + tw, iw)
        items[k, ya:yb, xa:xb] += templates[owner[k], ya - y0:yb - y0, xa - x0:xb - x0]
    (templates, tf), (items, itf) = _to_storage(templates, dtype), _to_storage(items, dtype)
    n = len(pos)
    want = np.empty((N_TEMPLATES, n))
    good = np.zeros(n, dtype=bool)
    for q in range(N_TEMPLATES):
        maps = oracle.ncc_maps(np.broadcast_to(tf[q], (n,) + t).copy(), itf, precise=True)
        want[q] = np.maximum(maps.reshape(n, -1).max(axis=1), 0.0)
        for k in np.flatnonzero(owner == q):
            flat = maps[k].ravel()
            planted = pos[k][0] * iw + pos[k][1]
            good[k] = flat.argmax() == planted and flat[planted] - np.delete(flat, planted).max() >= MARGIN
    label = f"{th}x{tw} on {ih}x{iw}, {dtype}, every {stride}. position"
    assert good.mean() >= GOOD_SHARE, f"{label}: only {good.mean():.3f} of the planted peaks are the oracle's clear maximum"
    rows = {pos[k][0] for k in np.flatnonzero(good)}
    cols = {pos[k][1] for k in np.flatnonzero(good)}
    assert rows == set(range(ih)) and cols == set(range(iw)), f"{label}: good pairs miss rows / columns"
    for a in (templates, items, tf, itf, owner, want, good):
        a.flags.writeable = False
    return templates, items, tf, itf, pos, owner, want, good


@functools.lru_cache(maxsize=None)
def _peak_restatement(t, i, stride):
    """restate_f32 for every (template, item) pair of the float32 peak inputs: [67, N] scores."""
    _, _, tf, itf, _, _, _, _ = _peak_inputs(t, i, "float32", stride)
    th, tw = t
    t0, i0 = _centre_f32(tf), _centre_f32(itf)
    (t_hi, t_lo), (i_hi, i_lo) = _hi_lo(t0), _hi_lo(i0)
    w_hi = _windows(i_hi, th, tw)
    num = np.tensordot(t_hi, w_hi, axes=([1, 2], [3, 4])) + np.tensordot(t_lo, w_hi, axes=([1, 2], [3, 4])) \
        + np.tensordot(t_hi, _windows(i_lo, th, tw), axes=([1, 2], [3, 4]))          # [67, N, ih, iw]
    s1, var, energy = _statistics(i0, t0)                                          # [N, ih, iw], [67]
    resid = (t_hi + t_lo).sum(axis=(-2, -1)) / float(th * tw)
    num = num - resid[:, None, None, None] * s1[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = num / np.sqrt(var[None] * energy[:, None, None, None])
    out[~np.isfinite(out)] = 0
    rest = np.maximum(out.reshape(N_TEMPLATES, len(itf), -1).max(axis=2), 0.0)
    rest.flags.writeable = False
    return rest


def _assert_scores(case, got, want, pos, owner, tol, what):
    err = np.abs(got.astype(np.float64) - want)
    err[~np.isfinite(err)] = np.inf
    worst = float(err.max())
    print(f"[mfma peaks] {case.id}: {len(pos)} positions, max |score - {what}| = {worst:.3g}")
    if not worst <= tol:
        bad = [(int(q), int(k)) for q, k in np.argwhere(~(err <= tol))]
        matched = [(q, k) for q, k in bad if owner[k] == q]
        lines = [f"query {q} (block {q // 64} wave {q % 64 // 16} lane {q % 16}) item {k} planted at row {pos[k][0]} column {pos[k][1]}"
                 f"{'' if owner[k] == q else ' (of another template)'}: got {got[q, k]:.7f} want {want[q, k]:.7f}"
                 for q, k in sorted(bad, key=lambda qk: -err[qk])[:25]]
        raise AssertionError(
            f"{case.id} against the {what}: {len(bad)} of {err.size} scores beyond {tol:g}, worst {worst:.3g}; matched pairs "
            f"off: planted rows {sorted({pos[k][0] for _, k in matched})}, planted columns {sorted({pos[k][1] for _, k in matched})}, "
            f"query slots (wave, lane) {sorted({(q % 64 // 16, q % 16) for q, _ in matched})}\n" + "\n".join(lines))
    return worst


def check_peaks(make_scorer, case, monkeypatch, every_position):
    stride = 1 if every_position else case.emu_stride
    mcase = case.map_case()
    templates, items, _, _, pos, owner, want, good = _peak_inputs(case.t, case.i, mcase.dtype, stride)
    sc, plan = make_plan(make_scorer, mcase, monkeypatch)
    dev = sc.dev
    qd, gd = dev.to_device(templates[:, None]), dev.to_device(items[:, None])

    def run():
        return dev.to_host(sc.scores_device(qd, gd, scores=dev.zeros((N_TEMPLATES, len(pos)), np.float32), plan=plan))

    got = run()
    if case.launches > 1:
        per = -(-len(pos) // case.launches)
        assert -(-len(pos) // per) == case.launches
        monkeypatch.setenv("SPR_NCC_MAX_TILES", str(per))
        sliced = run()
        monkeypatch.delenv("SPR_NCC_MAX_TILES")
        np.testing.assert_array_equal(sliced, got, err_msg=case.id)
    sc.close()
    assert got.shape == want.shape and got.dtype == np.float32
    print(f"[mfma peaks] {case.id}: {int(good.sum())} of {len(pos)} planted peaks good")
    if case.form != "f32":
        return {"oracle": _assert_scores(case, got, want, pos, owner, TIGHT, "oracle")}
    rest = _peak_restatement(case.t, case.i, stride)
    gap = float(np.abs(rest - want).max())
    print(f"[mfma peaks] {case.id}: max |restatement - oracle| = {gap:.3g}")
    return {"scheme": gap, "restatement": _assert_scores(case, got, rest, pos, owner, TIGHT, "restatement"),
            "oracle": _assert_scores(case, got, want, pos, owner, TOL, "oracle")}


# ------------------------------------------------------------------------------------------------- C. guard bands
class GuardCase(NamedTuple):
    method: str
    q_hw: tuple          # raw sizes: the scorer crops 2 pixels per edge
    g_hw: tuple
    dtype: str = "float32"
    channels: int = 2
    nq: int = 3
    ng: int = 5
    env: tuple = ()
    gpu_only: bool = False

    @property
    def id(self):
        tag = f"{self.method},{self.q_hw[0]}x{self.q_hw[1]}-on-{self.g_hw[0]}x{self.g_hw[1]},{self.dtype},{self.channels}ch,{self.nq}x{self.ng}"
        return tag + "".join(f",{k[8:]}={v}" for k, v in self.env)


GUARD_CASES = [
    GuardCase("fft", (12, 10), (20, 12)),
    GuardCase("fft", (32, 16), (32, 16)),
    GuardCase("fft", (30, 17), (33, 15), "float16", channels=3),          # 3 x 33 x 15: an odd element count per item
    GuardCase("fft", (44, 22), (44, 22), "bfloat16"),
    GuardCase("fft", (128, 64), (128, 64), channels=1, nq=3, ng=2),       # the six-wave kernel, an odd query count
    GuardCase("fft_pow2", (32, 16), (32, 16)),
    GuardCase("direct", (20, 12), (20, 12)),
    GuardCase("direct", (13, 9), (20, 16), "float16", channels=1),        # 13 x 9: odd
    GuardCase("mfma", (32, 16), (32, 16), "bfloat16", nq=5, ng=3),
    GuardCase("mfma", (32, 16), (32, 16), "bfloat16", nq=70, ng=3),       # a second block of six queries
    GuardCase("mfma", (33, 16), (32, 16), "float16"),
    GuardCase("mfma", (12, 9), (32, 16), "bfloat16", channels=3),
    GuardCase("mfma", (31, 15), (21, 9), "bfloat16", channels=3),         # 3 x 31 x 15 and 3 x 21 x 9: odd on both sides
    GuardCase("mfma", (32, 16), (21, 9), "bfloat16", env=(("SPR_NCC_MFMA_EXACT", "0"),)),
    GuardCase("mfma_f32", (32, 16), (32, 16)),
    GuardCase("mfma_f32", (34, 17), (32, 16)),
    GuardCase("fft", (32, 16), (32, 16), env=(("SPR_NCC_FORCE_BIG", "1"),), gpu_only=True),
]
FILLS = ((0xFF, 99), (0x7F, 99), (0x00, 99), (0xFF, 7))  # (interior byte, band seed): three fills, one more band


def for_emu(cases):
    return [c for c in cases if not c.gpu_only]


@functools.lru_cache(maxsize=None)
def _guard_inputs(case):
    """Half-normal synthetic features as the other score tests use them (their bound on these shapes is TIGHT), as stored,
    with the oracle's scores on the stored values."""
    c = case.channels
    g = np.stack([np.maximum(synth.gallery_features(83, k, c, *case.g_hw), 0) for k in range(case.ng)])
    if case.q_hw == case.g_hw:
        q = np.stack([np.maximum(synth.query_features(83, k, k % case.ng, c, *case.q_hw), 0) for k in range(case.nq)])
    else:
        q = np.stack([np.maximum(synth.gallery_features(89, 10 + k, c, *case.q_hw), 0) for k in range(case.nq)])
    (q, qf), (g, gf) = _to_storage(q, case.dtype), _to_storage(g, case.dtype)
    want = oracle.similarity_matrix(list(qf), list(gf), precise=True)
    match = (np.arange(case.nq) % case.ng).astype(np.int32)
    for a in (q, g, want, match):
        a.flags.writeable = False
    return q, g, want, match


def check_guarded(make_scorer, case, monkeypatch):
    """The five scorer calls of the C ABI on buffers of exactly the sizes the ABI names, between random bands."""
    q, g, want, match = _guard_inputs(case)
    set_env(monkeypatch, case.env)
    sc = make_scorer(case.method, crop=2)
    plan = sc.plan(case.channels, case.q_hw, case.g_hw, dtype=_NP_DTYPE[case.dtype])
    # (a plan of "fft_pow2" reports the FFT method; its grid is the power of two)
    assert plan.method == {"fft_pow2": _lib.NCC_FFT}.get(case.method, _METHODS[case.method]), (case.id, plan.method)
    if case.method == "fft_pow2":
        assert all(v & (v - 1) == 0 for v in plan.fft_size), (case.id, plan.fft_size)
    lib, dev, nq, ng = sc.lib, sc.dev, case.nq, case.ng
    ld, col0 = ng + 3, 2
    ih, iw = case.g_hw[0] - 4, case.g_hw[1] - 4
    sizes = [q.nbytes, g.nbytes, match.nbytes, lib.spr_ncc_query_bytes(plan.handle, nq), lib.spr_ncc_gallery_bytes(plan.handle, ng),
             4 * nq * ld, 4 * case.channels * ih * iw, 4 * nq]
    assert sizes[3] == nq * plan.query_item_bytes and sizes[4] == ng * plan.gallery_item_bytes

    def launch(b):
        for dst, src in zip(b[:3], (q, g, match)):
            dst[:] = dev.to_device(np.ascontiguousarray(src).reshape(-1).view(np.uint8))
        p = [dev.ptr(x) for x in b]
        s = dev.stream()
        lib.check(lib.spr_ncc_prepare_queries(plan.handle, p[0], nq, p[3], s))
        lib.check(lib.spr_ncc_prepare_gallery(plan.handle, p[1], ng, p[4], s))
        lib.check(lib.spr_ncc_score(plan.handle, p[3], nq, p[4], ng, p[5], ld, col0, 0, s))
        # the maps of the last query against the last item: the ends of both prepared buffers
        lib.check(lib.spr_ncc_maps(plan.handle, p[3] + (nq - 1) * plan.query_item_bytes, p[4] + (ng - 1) * plan.gallery_item_bytes,
                                   p[6], s))
        lib.check(lib.spr_rank_true_match(p[5] + 4 * col0, ld, nq, ng, p[2], p[7], s))

    runs = []
    for fill, seed in FILLS:
        out = run_guarded(dev, sizes, launch, fill=fill, seed=seed)  # asserts the bands
        for k, src in enumerate((q, g, match)):
            assert out[k].tobytes() == np.ascontiguousarray(src).tobytes(), f"{case.id}: input buffer {k} was written"
        rows = out[5].reshape(nq, 4 * ld)
        padding = np.concatenate([rows[:, :4 * col0], rows[:, 4 * (col0 + ng):]], axis=1)
        assert (padding == fill).all(), f"{case.id}, fill {fill:#x}: padding columns of the score matrix were written"
        runs.append((rows[:, 4 * col0: 4 * (col0 + ng)].copy().view(np.float32),
                     out[6].copy().view(np.float32).reshape(case.channels, ih, iw), out[7].copy().view(np.int32)))
    for (fill, seed), run in zip(FILLS[1:], runs[1:]):
        for name, a, b in zip(("scores", "maps", "ranks"), run, runs[0]):
            assert a.tobytes() == b.tobytes(), \
                f"{case.id}: {name} differ between fill {FILLS[0][0]:#x} / band seed {FILLS[0][1]} and fill {fill:#x} / band seed " \
                f"{seed}: {int((a.view(np.int32) != b.view(np.int32)).sum())} of {a.size} values (a read of bytes nobody wrote)"
    scores, maps, ranks = runs[0]
    err = float(np.abs(scores.astype(np.float64) - want).max()) if np.isfinite(scores).all() else np.inf
    print(f"[mfma guard] {case.id}: max |score - oracle| = {err:.3g}")
    np.testing.assert_allclose(scores, want, atol=TIGHT, rtol=0, err_msg=case.id)
    np.testing.assert_array_equal(ranks, oracle.ranks_from_matrix(scores, match), err_msg=case.id)
    assert np.isfinite(maps).all(), case.id
    # the maps are those of the scored pair: their channel mean peaks at its score
    peak = max(float(maps.astype(np.float64).sum(axis=0).max()) / case.channels, 0.0)
    assert abs(peak - want[nq - 1, ng - 1]) <= TIGHT, (case.id, peak, want[nq - 1, ng - 1])
    sc.close()
