#!/usr/bin/env python3
"""Kernel-only time of the float32 matrix-core pair kernel ("mfma_f32") against the FFT form on the same float32 maps, at the
config-3 shape (1024 channels, 32 x 16 on both sides) and at EfficientNetV2_M block 6 with a scaled query (176 channels,
33 x 16 on 32 x 16): python time_mfma_f32.py [--json OUT] [library ...]
--json writes the rates with the shader clock seen right after each timed loop and the library's sha256 (profiles/r04_mfma_f32_n1.json)."""
import glob, hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from shoeprint_image_retrieval_amd import _lib
from shoeprint_image_retrieval_amd.similarity import NccScorer
REPS = 5
args = sys.argv[1:]
out_json = args.pop(args.index("--json") + 1) if "--json" in args else None
if out_json: args.remove("--json")
def sclk_mhz():
    """current shader clock levels of the cards, from sysfs (plain reads; best effort)"""
    out = []
    for f in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            out += [int(l.split(":")[1].strip().lower().replace("mhz", "").replace("*", "")) for l in open(f).read().splitlines() if l.rstrip().endswith("*")]
        except (OSError, ValueError):
            pass
    return out
records = []
for path in (args or [None]):
    lib = _lib.load_library(path) if path else _lib.load_library()
    for C, QHW, NQ, NG in ((176, (33, 16), 64, 2048), (1024, (32, 16), 64, 5120)):
        for method in ("mfma_f32", "fft"):
            sc = NccScorer(method=method, library=lib); dev = sc.dev
            g = dev.empty((NG, C, 32, 16), np.float32); q = dev.empty((NQ, C, *QHW), np.float32)
            lib.check(lib.spr_synth_gallery(dev.ptr(g), 0, NG, C, 32, 16, 1234, dev.stream()))
            lib.check(lib.spr_synth_gallery(dev.ptr(q), 5000, NQ, C, *QHW, 1234, dev.stream()))
            plan = sc.plan(C, QHW, (32, 16))
            pq = sc.prepare_queries(plan, q); pg = sc.prepare_gallery(plan, g)
            scores = dev.zeros((NQ, NG), np.float32)
            for _ in range(2):
                sc.score_prepared(plan, pq, NQ, pg, NG, scores, NG, 0)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                sc.score_prepared(plan, pq, NQ, pg, NG, scores, NG, 0)
            b.record(); torch.cuda.synchronize()
            ms = a.elapsed_time(b) / REPS
            records.append({"library_sha256": hashlib.sha256(open(lib.path, "rb").read()).hexdigest(), "channels": C, "query_hw": list(QHW), "gallery_hw": [32, 16],
                            "dtype": "float32", "nq": NQ, "ng": NG, "method": method, "reps": REPS, "warmup": 2, "ms_per_call": round(ms, 3),
                            "pairs_per_s": round(NQ * NG / ms * 1e3, 1), "sclk_mhz_after": sclk_mhz(), "device": torch.cuda.get_device_name(0)})
            print(f"{os.path.basename(path) if path else 'shipped':20s} {C:5d} ch {QHW[0]}x{QHW[1]} on 32x16  {method:9s} {ms:9.2f} ms  {NQ * NG / ms / 1e3:7.2f} M pairs/s")
            del pq, pg, g, q
if out_json:
    json.dump({"what": "pair kernel only (spr_ncc_score on prepared buffers), HIP events around REPS calls after 2 warm-up calls; one process, one GPU",
               "records": records}, open(out_json, "w"), indent=1)
