#!/usr/bin/env python3
"""Time the surfaces form of the pair kernels against the list form, and retrieve(..., surfaces=True) against retrieve(...)
(one process, every side warmed up, the two sides of a comparison alternating, device work closed by a synchronise).  Writes one
JSON document.

  1. spr_ncc_score_surfaces against spr_ncc_score_list on the same list of pairs, sorted by gallery item (device events), the
     three list outputs bit-compared, for every --maps shape.  With --lib-b PATH the list form of a second build of the library
     (a build of the parent commit) takes turns with this build's in the same rounds.
  2. similarity.retrieve(..., surfaces=True) against similarity.retrieve(...) on FeatureSets with six rotations and four
     scales, 29 variant lists (host clock around a synchronise).

usage: time_surfaces.py [--json PATH] [--reps 5] [--pairs 6400] [--q 32] [--g 256] [--k 10] [--lib-b PATH]
"""
import argparse, hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from shoeprint_image_retrieval_amd import _lib, similarity, synth
from shoeprint_image_retrieval_amd.features import FeatureSet
from shoeprint_image_retrieval_amd.similarity import NccScorer

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--pairs", type=int, default=6400)
ap.add_argument("--maps", default="256,128,64;512,32,16")
ap.add_argument("--q", type=int, default=32)
ap.add_argument("--g", type=int, default=256)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--lib-b", default="")
ap.add_argument("--skip-retrieve", action="store_true")
args = ap.parse_args()
SHAPES = [tuple(int(v) for v in s.split(",")) for s in args.maps.split(";")]
sc = NccScorer(method="fft"); dev, lib = sc.dev, sc.lib


def load_older(path):
    """A second build that may predate the newest entry points: what it lacks answers 0."""
    import ctypes
    other = _lib.Library.__new__(_lib.Library)
    other.path, other.cdll = path, ctypes.CDLL(path)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        try:
            fn = getattr(other.cdll, name)
            fn.restype, fn.argtypes = restype, argtypes
        except AttributeError:
            fn = lambda *a: 0
        setattr(other, name, fn)
    return other


sc_b = NccScorer(method="fft", library=load_older(args.lib_b)) if args.lib_b else None
stats = lambda t: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def device_sets(shape, nq, ng, seed=1234):
    c, h, w = shape
    g, q = dev.empty((ng, c, h, w), np.float32), dev.empty((nq, c, h, w), np.float32)
    m = synth.default_matches(nq, ng)
    lib.check(lib.spr_synth_gallery(dev.ptr(g), 0, ng, c, h, w, seed, dev.stream()))
    lib.check(lib.spr_synth_queries(dev.ptr(q), 0, nq, dev.ptr(dev.to_device(m)), c, h, w, seed, 3, 3, 2, dev.stream()))
    return q, g, m


def surfaces_against_list(shape):
    nq = 32
    ng = args.pairs // nq
    n = nq * ng
    q, g, _ = device_sets(shape, nq, ng)
    plan = sc.plan(shape[0], shape[1:], shape[1:])
    assert plan.has_surfaces
    pq, pg = sc.prepare_queries(plan, q), sc.prepare_gallery(plan, g)
    pairs = dev.to_device(np.array([(a, b) for b in range(ng) for a in range(nq)], dtype=np.int32))  # sorted by gallery item
    ih, iw = shape[1] - 4, shape[2] - 4
    outs = {k: (dev.zeros((n,), np.float32), dev.zeros((n,), np.int32), dev.zeros((n,), np.int32)) for k in ("list", "surfaces", "list, build b")}
    maps = dev.zeros((n, ih, iw), np.float32)
    forms = {"list": lambda: sc.score_list_prepared(plan, pq, nq, pg, ng, pairs, n, *outs["list"], tag=1),
             "surfaces": lambda: sc.surfaces_prepared(plan, pq, nq, pg, ng, pairs, n, *outs["surfaces"][:2], maps, outs["surfaces"][2], tag=1)}
    if sc_b is not None:
        plan_b = sc_b.plan(shape[0], shape[1:], shape[1:])
        pq_b, pg_b = sc_b.prepare_queries(plan_b, q), sc_b.prepare_gallery(plan_b, g)
        forms["list, build b"] = lambda: sc_b.score_list_prepared(plan_b, pq_b, nq, pg_b, ng, pairs, n, *outs["list, build b"], tag=1)
    ms = {k: [] for k in forms}
    for rnd in range(args.reps + 1):  # (round 0 warms every form up)
        for name, call in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); torch.cuda.synchronize()
            if rnd:
                ms[name].append(e0.elapsed_time(e1))
    equal = {k: all(np.array_equal(dev.to_host(a).view(np.int32), dev.to_host(b).view(np.int32)) for a, b in zip(outs[k], outs["list"]))
             for k in forms if k != "list"}
    top = dev.to_host(maps).reshape(n, -1).max(axis=1)
    equal["floored surface maximum == score"] = bool(np.array_equal(np.maximum(top, 0).view(np.int32), dev.to_host(outs["surfaces"][0]).view(np.int32)))
    med = {k: float(np.median(t)) for k, t in ms.items()}
    spread = (max(ms["list"]) - min(ms["list"])) / med["list"]
    doc = {"maps": list(shape), "pairs": n, "fft_size": list(plan.fft_size), "reps": args.reps, "surface_bytes_per_pair": ih * iw * 4,
           "ms": {k: stats(t) for k, t in ms.items()}, "pairs_per_s": {k: round(n / v * 1e3) for k, v in med.items()},
           "surfaces_over_list_time": round(med["surfaces"] / med["list"], 4), "list_relative_spread": round(spread, 4),
           "bit_equal": equal}
    if sc_b is not None:
        doc["list_this_over_build_b_time"] = round(med["list"] / med["list, build b"], 4)
    return doc


def retrieve_with_and_without():
    shape = SHAPES[0]
    nq, ng = args.q, args.g
    q, g, _ = device_sets(shape, nq, ng)
    qs, gs = FeatureSet(dev, nq, [(shape, np.arange(nq), q)]), FeatureSet(dev, ng, [(shape, np.arange(ng), g)])
    cfg = {"comparison": {"n_processes": 1, "rotations": [-15, -9, -3, 3, 9, 15], "scales": [1.02, 1.04, 1.08, 0.96]}}
    from shoeprint_image_retrieval_amd.variants import variant_labels
    sides = {"retrieve": lambda: similarity.retrieve(qs, gs, cfg, k=args.k, scorer=sc),
             "retrieve, surfaces": lambda: similarity.retrieve(qs, gs, cfg, k=args.k, scorer=sc, surfaces=True)}
    s, last = {k: [] for k in sides}, {}
    for rnd in range(max(2, args.reps // 2) + 1):
        for name, call in sides.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            last[name] = call()
            torch.cuda.synchronize()
            if rnd:
                s[name].append(time.perf_counter() - t0)
    a, b = last["retrieve"], last["retrieve, surfaces"]
    same = all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("index", "variant", "peak_yx", "offset")) and \
        np.array_equal(a.score.view(np.int32), b.score.view(np.int32))
    return {"maps": list(shape), "queries": nq, "gallery": ng, "k": args.k, "variant_lists": len(variant_labels(cfg["comparison"]["rotations"], cfg["comparison"]["scales"])),
            "seconds": {k: stats(t) for k, t in s.items()},
            "extra_seconds_per_call": float(np.median(s["retrieve, surfaces"]) - np.median(s["retrieve"])),
            "same_shortlist": bool(same), "median_psr_rank_1": float(np.median(b.psr[:, 0])), "median_psr_rank_k": float(np.median(b.psr[:, -1]))}


with open(_lib.DEFAULT_PATH, "rb") as fh:
    lib_hash = hashlib.sha256(fh.read()).hexdigest()[:16]
doc = {"command": "tools/ubench/time_surfaces.py " + " ".join(sys.argv[1:]), "library_sha16": lib_hash,
       "device": torch.cuda.get_device_name(0),
       "method": "one process; every side runs once as a warm-up, then `reps` rounds that run the sides in turn; part 1: device "
                 "events around each call; part 2: host clock around a synchronise",
       "surfaces_against_list": [surfaces_against_list(s) for s in SHAPES]}
if not args.skip_retrieve:
    doc["retrieve_surfaces"] = retrieve_with_and_without()
text = json.dumps(doc, indent=1)
print(text)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        fh.write(text + "\n")
