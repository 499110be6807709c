#!/usr/bin/env python3
"""Time the list form of the pair kernels and the cascade built on it (one process, every shape warmed up, the two sides of a
comparison alternating, device work closed by a synchronise).  Writes one JSON document.

  1. spr_ncc_score_peaks over a Q x G grid against spr_ncc_score_list over the same Q * G pairs, once sorted by gallery item
     and once shuffled (device events), bit-compared.
  2. NccScorer.multi_layer_score_matrix_device + ranks against similarity.retrieve_cascade + ranks on two feature layers of
     the same synthetic items (host clock around a synchronise), and where the cascade's time goes: an extra, instrumented
     pass with a synchronise around the coarse layer, every gallery preparation and every list call.

usage: time_cascade.py [--json PATH] [--reps 3] [--q 64] [--g-list 256] [--g 1500] [--depth 100]
"""
import argparse, hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from shoeprint_image_retrieval_amd import _lib, similarity, synth
from shoeprint_image_retrieval_amd.features import FeatureSet
from shoeprint_image_retrieval_amd.similarity import NccScorer

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--q", type=int, default=64)
ap.add_argument("--g-list", type=int, default=256)
ap.add_argument("--g", type=int, default=1500)
ap.add_argument("--depth", type=int, default=100)
ap.add_argument("--fine", default="256,128,64")
ap.add_argument("--coarse", default="512,32,16")
args = ap.parse_args()
FINE, COARSE = (tuple(int(v) for v in s.split(",")) for s in (args.fine, args.coarse))
sc = NccScorer(method="auto"); dev, lib = sc.dev, sc.lib
stats = lambda t: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def device_sets(shape, nq, ng, seed=1234):
    """(query batch, gallery batch, matches) of synthetic features made on the device."""
    c, h, w = shape
    g, q = dev.empty((ng, c, h, w), np.float32), dev.empty((nq, c, h, w), np.float32)
    m = synth.default_matches(nq, ng)
    lib.check(lib.spr_synth_gallery(dev.ptr(g), 0, ng, c, h, w, seed, dev.stream()))
    lib.check(lib.spr_synth_queries(dev.ptr(q), 0, nq, dev.ptr(dev.to_device(m)), c, h, w, seed, 3, 3, 2, dev.stream()))
    return q, g, m


# ---------------------------------------------------------------------------------------------- 1. list against dense
def list_against_dense():
    nq, ng = args.q, args.g_list
    q, g, _ = device_sets(FINE, nq, ng)
    plan = sc.plan(FINE[0], FINE[1:], FINE[1:])
    assert plan.has_list and plan.has_peaks
    pq, pg = sc.prepare_queries(plan, q), sc.prepare_gallery(plan, g)
    n = nq * ng
    every = np.array([(a, b) for b in range(ng) for a in range(nq)], dtype=np.int32)  # sorted by gallery item
    lists = {"sorted": every, "shuffled": every[np.random.default_rng(5).permutation(n)]}
    d_s, d_yx, d_tag = dev.zeros((nq, ng), np.float32), dev.zeros((nq, ng), np.int32), dev.zeros((nq, ng), np.int32)
    outs = {k: (dev.to_device(v), dev.zeros((n,), np.float32), dev.zeros((n,), np.int32), dev.zeros((n,), np.int32))
            for k, v in lists.items()}
    forms = {"dense": lambda: sc.score_prepared(plan, pq, nq, pg, ng, d_s, ng, 0, peaks=d_yx, tags=d_tag, tag=1)}
    for k, (pairs, s, yx, tag) in outs.items():
        forms[k] = (lambda pairs=pairs, s=s, yx=yx, tag=tag: sc.score_list_prepared(plan, pq, nq, pg, ng, pairs, n, s, yx, tag, tag=1))
    ms = {k: [] for k in forms}
    for rnd in range(args.reps + 1):  # (round 0 warms every form up)
        for name, call in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); torch.cuda.synchronize()
            if rnd:
                ms[name].append(e0.elapsed_time(e1))
    equal = {}
    for k, (pairs, s, yx, tag) in outs.items():
        qs, gs = lists[k][:, 0], lists[k][:, 1]
        equal[k] = all(np.array_equal(dev.to_host(got).view(np.int32), dev.to_host(want).view(np.int32)[qs, gs])
                       for got, want in ((s, d_s), (yx, d_yx), (tag, d_tag)))
    rate = {k: n / np.median(t) * 1e3 for k, t in ms.items()}
    return {"maps": list(FINE), "queries": nq, "gallery": ng, "pairs": n, "fft_size": list(plan.fft_size), "reps": args.reps,
            "ms": {k: stats(t) for k, t in ms.items()}, "pairs_per_s": {k: round(v) for k, v in rate.items()},
            "sorted_over_dense": round(rate["sorted"] / rate["dense"], 4), "shuffled_over_dense": round(rate["shuffled"] / rate["dense"], 4),
            "bit_equal_to_dense": equal}


# ---------------------------------------------------------------------------------------------- 2. cascade against fusion
def cascade_against_fusion():
    nq, ng = args.q, args.g
    layer_sets, match = [], None
    for shape in (FINE, COARSE):
        q, g, match = device_sets(shape, nq, ng)
        layer_sets.append((FeatureSet(dev, nq, [(shape, np.arange(nq), q)]), FeatureSet(dev, ng, [(shape, np.arange(ng), g)])))
    cfg = {"comparison": {"n_processes": 1, "rotations": None, "scales": None}}

    def fusion():
        return sc.ranks_of_device(sc.multi_layer_score_matrix_device(layer_sets), match)

    def cascade():
        return similarity.retrieve_cascade(layer_sets, cfg, args.depth, scorer=sc).ranks(match)

    sides = {"full fusion": fusion, "cascade": cascade}
    s, ranks = {k: [] for k in sides}, {}
    for rnd in range(args.reps + 1):
        for name, call in sides.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ranks[name] = call()
            torch.cuda.synchronize()
            if rnd:
                s[name].append(time.perf_counter() - t0)
    # where the cascade's time goes: one more pass with a synchronise around its three device phases
    phase = {"dense coarse layer": 0.0, "gallery preparation (fine layer)": 0.0, "list launches": 0.0}

    def timed(fn, key):
        def wrapper(*a, **kw):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize(); phase[key] += time.perf_counter() - t0
            return out
        return wrapper

    plain = sc.score_matrix_device, sc.prepare_gallery, sc.score_list_prepared
    torch.cuda.synchronize(); t0 = time.perf_counter()
    try:
        # (the coarse layer prepares its gallery inside score_matrix_device: hook the others only once it has returned)
        def coarse_then_hook(*a, **kw):
            out = timed(plain[0], "dense coarse layer")(*a, **kw)
            sc.prepare_gallery = timed(plain[1], "gallery preparation (fine layer)")
            sc.score_list_prepared = timed(plain[2], "list launches")
            return out
        sc.score_matrix_device = coarse_then_hook
        cascade()
    finally:
        for name in ("score_matrix_device", "prepare_gallery", "score_list_prepared"):
            sc.__dict__.pop(name, None)  # (back to the class's methods)
    torch.cuda.synchronize(); total = time.perf_counter() - t0
    phase["the rest (top-k, query preparation, gathers, host)"] = total - sum(phase.values())
    spread = max(s["full fusion"]) - min(s["full fusion"])
    gain = float(np.median(s["full fusion"]) - np.median(s["cascade"]))
    return {"queries": nq, "gallery": ng, "layers": [list(FINE), list(COARSE)], "depth": args.depth, "reps": args.reps,
            "seconds": {k: stats(t) for k, t in s.items()},
            "cascade_over_full_fusion": round(float(np.median(s["cascade"]) / np.median(s["full fusion"])), 4),
            "full_fusion_spread_s": spread, "median_gain_s": gain, "faster_by_more_than_the_spread": bool(gain > spread),
            "instrumented_cascade_s": {"total": total, **phase},
            "rank_1_queries": {k: int((r == 1).sum()) for k, r in ranks.items()},
            "queries_whose_match_is_a_candidate": int((ranks["cascade"] <= args.depth).sum())}


with open(_lib.DEFAULT_PATH, "rb") as fh:
    lib_hash = hashlib.sha256(fh.read()).hexdigest()[:16]
doc = {"command": "tools/ubench/time_cascade.py " + " ".join(sys.argv[1:]), "library_sha16": lib_hash,
       "device": torch.cuda.get_device_name(0),
       "method": "one process; every side runs once as a warm-up, then `reps` rounds that run the sides in turn; part 1: device "
                 "events around each call; part 2: host clock around a synchronise, rank vector included",
       "list_against_dense": list_against_dense(), "cascade_against_full_fusion": cascade_against_fusion()}
text = json.dumps(doc, indent=1)
print(text)
if args.json:
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
