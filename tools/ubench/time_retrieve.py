#!/usr/bin/env python3
"""Wall time of similarity.retrieve(locate=True) after one warm-up call, once without query variants and once with a
rotation / scale list, on device-synthesised maps.  Prints one JSON line.  The script uses nothing but retrieve() and the
synth entry points, so the same file times an older checkout of the package (copy it into that tree's tools/ubench/).

usage: time_retrieve.py            (TR_Q, TR_G, TR_C, TR_H, TR_W, TR_K, TR_REPS in the environment change the shape;
                                    TR_VARIANTS=0 skips the run with variants; TR_METHOD, TR_DTYPE: the scorer's method and
                                    storage type, default "auto" and "float32"; TR_PEAKS=1: NccScorer(matrix_core_peaks=True),
                                    which an older checkout does not know - leave it unset there)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from shoeprint_image_retrieval_amd import similarity, synth
from shoeprint_image_retrieval_amd.similarity import NccScorer

Q, G = int(os.environ.get("TR_Q", 32)), int(os.environ.get("TR_G", 256))
C, H, W = int(os.environ.get("TR_C", 256)), int(os.environ.get("TR_H", 128)), int(os.environ.get("TR_W", 64))
K, REPS = int(os.environ.get("TR_K", 10)), int(os.environ.get("TR_REPS", 2))
ROTATIONS, SCALES = [-15, -9, -3, 3, 9, 15, 180], [1.02, 1.04, 1.08]  # the reference's run.toml

METHOD, DTYPE = os.environ.get("TR_METHOD", "auto"), os.environ.get("TR_DTYPE", "float32")
PEAKS = os.environ.get("TR_PEAKS", "0") == "1"
sc = NccScorer(method=METHOD, storage=DTYPE, **({"matrix_core_peaks": True} if PEAKS else {}))
dev, lib = sc.dev, sc.lib
g = dev.empty((G, C, H, W), np.float32); q = dev.empty((Q, C, H, W), np.float32)
m = dev.to_device(synth.default_matches(Q, G))
lib.check(lib.spr_synth_gallery(dev.ptr(g), 0, G, C, H, W, 1234, dev.stream()))
lib.check(lib.spr_synth_queries(dev.ptr(q), 0, Q, dev.ptr(m), C, H, W, 1234, 3, 3, 2, dev.stream()))
q_items, g_items = list(dev.to_host(q)), list(dev.to_host(g))
del q, g

def cfg(rot, scales):
    return {"comparison": {"n_processes": 1, "rotations": rot, "scales": scales}}

def timed(config):
    similarity.retrieve(q_items, g_items, config, k=K, scorer=sc)  # warm-up: plans, tables, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        short = similarity.retrieve(q_items, g_items, config, k=K, scorer=sc)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, short

out = {"shape": [Q, G, C, H, W], "k": K, "repetitions": REPS, "method": METHOD, "dtype": DTYPE, "matrix_core_peaks": PEAKS}
t, short = timed(cfg(None, None))
out["no_variants_s"] = [round(x, 4) for x in t]
out["top1_is_planted_match"] = int((short.index[:, 0] == synth.default_matches(Q, G)).sum())
if os.environ.get("TR_VARIANTS", "1") != "0":
    t, short = timed(cfg(ROTATIONS, SCALES))
    out["variants"] = {"rotations": ROTATIONS, "scales": SCALES}
    out["with_variants_s"] = [round(x, 4) for x in t]
    out["with_variants_top1_is_planted_match"] = int((short.index[:, 0] == synth.default_matches(Q, G)).sum())
out["plan_methods"] = sorted({p.method for p in sc._plans.values()})
print(json.dumps(out))
