"""Cases for the per-channel paths of the six-wave pair kernel (csrc/ncc_pair6.hip), shared by the CPU-emulation runner
(test_emu_pair6_paths.py, not gpu) and the MI355X runner (test_gpu_pair6_paths.py, gpu).

Every case is a set of [C,128,64] float32 maps - the only shape class the kernel serves - scored pair by pair against the
float64 oracle at parity_cases.TIGHT.  What the cases walk through:

* the live-channel list: its length (C = 1, 2, 3: the clamped look-ahead to the next channel and the one after), channels
  that are constant on either side in every position of the list, and the empty list (score exactly 0);
* the Nyquist column, which travels apart from the rest of the spectrum through its own two-buffer LDS path: maps with a
  column-alternating component put energy there, so a wrong product or a wrong buffer parity moves the score;
* the workgroup tiling: an odd query count (the second half of the last workgroup idles), gallery counts on both sides of a
  workgroup's second-item slot and of a 16-item tile;
* the four forms of the kernel: plain, accumulate, peaks, per-channel maps.

The emulation scores of the parent of the commit that added these cases lie in golden/pair6_paths_parent.npz: the kernel's
arithmetic is meant to stay what it was, bit for bit.

Largest errors, the bound being TIGHT = 5e-6 (each check prints its own figure): scores 1.5e-8 under emulation and on an
MI355X alike, per-channel maps 4.5e-8 (nyquist-both).
"""

import functools
import os
from typing import NamedTuple

import numpy as np

import peak_cases as pc
from oracle import ncc_oracle as oracle
from parity_cases import GOLDEN, TIGHT
from shortlist_cases import POSITION_LEAD

H, W, CROP = 128, 64, 2
GOLDEN_FILE = os.path.join(GOLDEN, "pair6_paths_parent.npz")
PREFILL_STEP = 1e-3  # the accumulate form's score block before the call: the oracle's scores, this much off


class PathCase(NamedTuple):
    name: str
    channels: int
    nq: int
    ng: int
    dead_q: tuple = ()   # (query, channel) made constant
    dead_g: tuple = ()   # (gallery item, channel) made constant
    nyquist: str = ""    # "q", "g", "qg": who gets the column-alternating component
    forms: bool = False  # also run the accumulate, peaks and maps forms
    emu: bool = True

    @property
    def seed(self):
        return [29, self.channels, self.nq, self.ng, sum(map(ord, self.name))]


def _all(n, channels):
    return tuple((i, c) for i in range(n) for c in channels)


CASES = [
    # live-channel counts
    PathCase("live1", 1, 2, 1),
    PathCase("live2", 2, 2, 1),
    PathCase("live3", 3, 2, 1, forms=True),
    # dead-channel patterns, C = 6 (the second query stays fully live where only the query side is touched: the two halves
    # of a workgroup then walk different lists)
    PathCase("dead-query-only", 6, 2, 1, dead_q=((0, 1), (0, 4))),
    PathCase("dead-gallery-only", 6, 2, 1, dead_g=((0, 2), (0, 3))),
    PathCase("dead-both", 6, 2, 1, dead_q=((0, 1), (1, 3), (1, 4)), dead_g=((0, 3), (0, 5))),
    PathCase("dead-first", 6, 2, 1, dead_g=((0, 0),)),
    PathCase("dead-last", 6, 2, 1, dead_q=_all(2, (5,))),
    PathCase("dead-every-second", 6, 2, 1, dead_g=((0, 1), (0, 3), (0, 5)), forms=True),
    PathCase("dead-all", 6, 2, 1, dead_q=_all(1, range(6)), dead_g=_all(1, range(6)), forms=True),
    # query and gallery counts
    PathCase("counts-3x3", 2, 3, 3, forms=True),
    PathCase("counts-3x17", 2, 3, 17, emu=False),
    # energy at the horizontal Nyquist frequency
    PathCase("nyquist-query", 2, 2, 1, nyquist="q"),
    PathCase("nyquist-gallery", 2, 2, 1, nyquist="g"),
    PathCase("nyquist-both", 3, 2, 1, nyquist="qg", forms=True),
]
EMU_CASES = [c for c in CASES if c.emu]
IDS = lambda cases: [c.name for c in cases]  # noqa: E731


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(queries [nq,C,128,64], gallery [ng,C,128,64], oracle score matrix float64 [nq,ng]) - computed once, read-only."""
    rng = np.random.default_rng(case.seed)
    q = rng.standard_normal((case.nq, case.channels, H, W), dtype=np.float32)
    g = rng.standard_normal((case.ng, case.channels, H, W), dtype=np.float32)
    stripes = np.where(np.arange(W) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if "q" in case.nyquist:
        q += (1.5 * rng.standard_normal((case.nq, case.channels, H, 1), dtype=np.float32)) * stripes
    if "g" in case.nyquist:
        g += (1.5 * rng.standard_normal((case.ng, case.channels, H, 1), dtype=np.float32)) * stripes
    for k, (i, c) in enumerate(case.dead_q):
        q[i, c] = 0.0 if k % 2 == 0 else 0.75   # all zero, or constant and zero only after centring
    for k, (i, c) in enumerate(case.dead_g):
        g[i, c] = 0.0 if k % 2 == 0 else 0.75
    want = np.asarray(oracle.similarity_matrix(list(q), list(g), precise=True), dtype=np.float64)
    for a in (q, g, want):
        a.flags.writeable = False
    return q, g, want


def no_live_channel(case):
    """[nq, ng] bool: pairs whose every channel is constant on one side or the other."""
    dead_q = np.zeros((case.nq, case.channels), bool)
    dead_g = np.zeros((case.ng, case.channels), bool)
    for i, c in case.dead_q:
        dead_q[i, c] = True
    for i, c in case.dead_g:
        dead_g[i, c] = True
    return (dead_q[:, None, :] | dead_g[None, :, :]).all(axis=2)


def make(make_scorer, case):
    q, g, want = inputs(case)
    sc = make_scorer("fft")
    plan = sc.plan(case.channels, (H, W), (H, W))
    assert plan.fft_size == (192, 96) and plan.crop == CROP, (case.name, plan.fft_size)
    pq, pg = pc.prepare(sc, plan, q, g)
    return sc, plan, pq, pg


def check_plain(make_scorer, case):
    """spr_ncc_score of every pair against the oracle; returns the float32 score matrix."""
    q, g, want = inputs(case)
    sc, plan, pq, pg = make(make_scorer, case)
    got = pc.plain_scores(sc, plan, pq, case.nq, pg, case.ng)
    sc.close()
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - np.maximum(want, 0.0))
    err[~np.isfinite(err)] = np.inf
    print(f"[pair6 paths] {case.name}: max |score - oracle| = {err.max():.3g}")
    assert err.max() <= TIGHT, (case.name, np.argwhere(~(err <= TIGHT)).tolist(), got.tolist(), want.tolist())
    none = no_live_channel(case)
    assert (got[none] == 0.0).all(), f"{case.name}: a pair without a live channel scores exactly 0"
    return got


def check_forms(make_scorer, case):
    """The accumulate, peaks and maps forms on the case's inputs, against the plain form and the oracle."""
    q, g, want = inputs(case)
    sc, plan, pq, pg = make(make_scorer, case)
    dev, nq, ng = sc.dev, case.nq, case.ng
    plain = pc.plain_scores(sc, plan, pq, nq, pg, ng)
    # accumulate = 1 over a pre-filled block: the larger of the two, bit for bit
    # (pre-filled from the oracle, PREFILL_STEP = 200 x TIGHT above and below it in turn: the call raises every other score)
    sign = np.where((np.arange(nq)[:, None] + np.arange(ng)[None, :]) % 2 == 0, -1.0, 1.0)
    before = (np.maximum(want, 0.0) + sign * PREFILL_STEP).astype(np.float32)
    block = dev.to_device(before)
    sc.score_prepared(plan, pq, nq, pg, ng, block, ng, 0, accumulate_max=True)
    np.testing.assert_array_equal(pc.bits(np.array(dev.to_host(block))), pc.bits(np.maximum(plain, before)))
    assert ((plain > before) == (sign < 0)).all() or no_live_channel(case).any(), case.name
    # peaks: the plain scores bit for bit (asserted inside, between guard bands), the position on the oracle's maximum
    scores, yx, tags = pc.score_peaks(sc, plan, pq, nq, pg, ng, tag=3)
    np.testing.assert_array_equal(pc.bits(scores), pc.bits(plain))
    cq, cg = q[:, :, CROP:-CROP, CROP:-CROP], g[:, :, CROP:-CROP, CROP:-CROP]
    for qi in range(nq):
        for gi in range(ng):
            if scores[qi, gi] > 0:
                summed = oracle.ncc_maps(cq[qi], cg[gi], precise=True).sum(axis=0)
                y, x = (int(v) for v in yx[qi, gi])
                assert 0 <= y < summed.shape[0] and 0 <= x < summed.shape[1], (case.name, qi, gi, y, x)
                assert summed[y, x] >= summed.max() - POSITION_LEAD, (case.name, qi, gi, (y, x))
    # maps: every pixel of every channel of the last pair (the others through single-item prepared sets would only repeat it)
    qi, gi = nq - 1, ng - 1
    pq1, pg1 = pc.prepare(sc, plan, q[qi:qi + 1], g[gi:gi + 1])
    maps = np.array(dev.to_host(sc.ncc_maps_device(plan, pq1, pg1)))
    sc.close()
    want_maps = oracle.ncc_maps(cq[qi], cg[gi], precise=True)
    assert maps.shape == want_maps.shape and maps.dtype == np.float32
    err = np.abs(maps.astype(np.float64) - want_maps)
    err[~np.isfinite(err)] = np.inf
    print(f"[pair6 paths] {case.name}: maps max |err| = {err.max():.3g}")
    assert err.max() <= TIGHT, (case.name, float(err.max()), np.unravel_index(int(err.argmax()), err.shape))
    dead = {c for i, c in case.dead_q if i == qi} | {c for i, c in case.dead_g if i == gi}
    for c in dead:
        assert not maps[c].any(), f"{case.name}: dead channel {c} must give exact zeros"
    # the map maximum against the score: the same float32 products, summed over at most six channels in another order
    top = max(float(maps.astype(np.float64).sum(axis=0).max()) / case.channels, 0.0)
    assert abs(top - float(plain[qi, gi])) <= TIGHT, (case.name, top, float(plain[qi, gi]))
    return plain


def golden():
    z = np.load(GOLDEN_FILE)
    return z, str(z["parent_commit"])


def write_golden(make_scorer, commit):
    """Record the emulation scores of the checked-out tree as the parent's (run once, on the parent commit)."""
    out = {"parent_commit": np.array(commit)}
    for case in EMU_CASES:
        out[case.name + "_seed"] = np.asarray(case.seed, dtype=np.int64)
        out[case.name + "_scores"] = check_plain(make_scorer, case)
    np.savez_compressed(GOLDEN_FILE, **out)


def check_against_parent(case, got):
    """Emulation only: the scores equal, bit for bit, those of the parent commit's kernel on the same seeds."""
    z, commit = golden()
    np.testing.assert_array_equal(np.asarray(z[case.name + "_seed"]), np.asarray(case.seed))
    np.testing.assert_array_equal(pc.bits(got), pc.bits(z[case.name + "_scores"]),
                                  err_msg=f"{case.name}: scores differ from those of {commit}")
