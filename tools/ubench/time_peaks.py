#!/usr/bin/env python3
"""Time spr_ncc_score against spr_ncc_score_peaks on the same prepared buffers (HIP events, interleaved rounds, one
process): what the arg-max epilogue of the pair kernels costs.  Prints one JSON line.
usage: time_peaks.py [method]   (TP_Q, TP_G, TP_C, TP_H, TP_W in the environment change the shape, TP_QH / TP_QW the query
maps' own size; TP_DTYPE the storage type: float32 | float16 | bfloat16.  A matrix-core method - "mfma" wants a 16-bit
TP_DTYPE, "mfma_f32" float32 - is asked for its peak form, NccScorer(matrix_core_peaks=True).)"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from shoeprint_image_retrieval_amd import synth
from shoeprint_image_retrieval_amd.similarity import NccScorer
C, H, W = int(os.environ.get("TP_C", 256)), int(os.environ.get("TP_H", 128)), int(os.environ.get("TP_W", 64))
NQ, NG = int(os.environ.get("TP_Q", 100)), int(os.environ.get("TP_G", 1500))
QH, QW = int(os.environ.get("TP_QH", H)), int(os.environ.get("TP_QW", W))
DTYPE = os.environ.get("TP_DTYPE", "float32")
method = sys.argv[1] if len(sys.argv) > 1 else "fft"
sc = NccScorer(method=method, storage=DTYPE, matrix_core_peaks=method in ("mfma", "mfma_f32")); dev = sc.dev; lib = sc.lib
g = dev.empty((NG, C, H, W), np.float32); q = dev.empty((NQ, C, QH, QW), np.float32)
m = dev.to_device(synth.default_matches(NQ, NG))
lib.check(lib.spr_synth_gallery(dev.ptr(g), 0, NG, C, H, W, 1234, dev.stream()))
if (QH, QW) == (H, W):
    lib.check(lib.spr_synth_queries(dev.ptr(q), 0, NQ, dev.ptr(m), C, H, W, 1234, 3, 3, 2, dev.stream()))
else:  # queries of another size than the gallery maps: gallery-like maps of their own
    lib.check(lib.spr_synth_gallery(dev.ptr(q), 0, NQ, C, QH, QW, 4321, dev.stream()))
g, q = dev.astype_storage(g, DTYPE), dev.astype_storage(q, DTYPE)
plan = sc.plan(C, (QH, QW), (H, W), dtype=DTYPE)
assert plan.has_peaks, "the plan has no peak form"
pq = sc.prepare_queries(plan, q); pg = sc.prepare_gallery(plan, g)
del g
plain, located = dev.zeros((NQ, NG), np.float32), dev.zeros((NQ, NG), np.float32)
yx, tags = dev.zeros((NQ, NG), np.int32), dev.zeros((NQ, NG), np.int32)
forms = {"spr_ncc_score": lambda: sc.score_prepared(plan, pq, NQ, pg, NG, plain, NG, 0),
         "spr_ncc_score_peaks": lambda: sc.score_prepared(plan, pq, NQ, pg, NG, located, NG, 0, peaks=yx, tags=tags, tag=1)}
ms = {k: [] for k in forms}
for rnd in range(5):
    for name, call in forms.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        if rnd:
            ms[name].append(e0.elapsed_time(e1))
same = bool(torch.equal(plain.view(torch.int32), located.view(torch.int32)))
print(json.dumps({"method": method, "plan_method": plan.method, "dtype": DTYPE, "fft_size": list(plan.fft_size),
                  "shape": [NQ, NG, C, H, W], "query_hw": [QH, QW], "scores_bit_equal": same,
                  "peaks_over_plain_min": round(min(ms["spr_ncc_score_peaks"]) / min(ms["spr_ncc_score"]), 4),
                  "peaks_over_plain_median": round(float(np.median(ms["spr_ncc_score_peaks"]) / np.median(ms["spr_ncc_score"])), 4),
                  **{k + "_ms": [round(v, 3) for v in t] for k, t in ms.items()},
                  **{k + "_pairs_per_s": round(NQ * NG / min(t) * 1e3) for k, t in ms.items()}}))
