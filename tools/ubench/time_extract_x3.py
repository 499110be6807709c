#!/usr/bin/env python3
"""Time the plain-VGG extractor under the float32, bfloat16x3 and bfloat16 plans, alternating in one process.

VGG16 features[:16] on a batch of 32 grey 512 x 256 images (TE_N / TE_BLOCK change that), seeded weights.  Every plan is warmed
up once, then the three plans take turns TE_REPS times (default 7); each turn is TE_CALLS extract_device calls between two
device events.  Prints medians and spreads and writes them, with the library's hash and the largest deviation of the
bfloat16x3 features from the float32 plan's at this size, to the JSON file named on the command line."""
import hashlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from shoeprint_image_retrieval_amd import _lib, network

N, H, W, BLOCK = int(os.environ.get("TE_N", 32)), 512, 256, int(os.environ.get("TE_BLOCK", 16))
REPS, CALLS = int(os.environ.get("TE_REPS", 7)), int(os.environ.get("TE_CALLS", 10))
PLANS = ("float32", "bfloat16x3", "bfloat16")
LIB_PATH = os.environ.get("TE_LIB") or _lib.DEFAULT_PATH  # TE_LIB: another build of the library (A/B runs; the ctypes route)
library = _lib.load_library(os.environ.get("TE_LIB") or None)
models = {d: network.Model({"model": {"type": "VGG16", "clahe_clip_limit": 2.0, "clahe_tile_grid_size": [8, 8]},
                            "mi355x": {"extractor_dtype": d}}, BLOCK, library=library) for d in PLANS}
imgs = torch.randint(0, 256, (N, H, W), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
outs = {d: m.extract_device(imgs) for d, m in models.items()}  # the warm-up
torch.cuda.synchronize()
ref = outs["float32"].double()
scale = ref.pow(2).mean().sqrt().item()
dev = {d: ((outs[d].double() - ref).abs().max().item() / scale, (outs[d].double() - ref).pow(2).mean().sqrt().item() / scale)
       for d in PLANS[1:]}
ms = {d: [] for d in PLANS}
for _ in range(REPS):
    for d in PLANS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            models[d].extract_device(imgs)
        e1.record()
        torch.cuda.synchronize()
        ms[d].append(e0.elapsed_time(e1) / CALLS)
with open(LIB_PATH, "rb") as f:
    digest = hashlib.sha256(f.read()).hexdigest()[:16]
res = {"library": os.path.relpath(LIB_PATH), "what": f"VGG16[:{BLOCK}] extract_device, {N} grey {H}x{W} images, seeded weights; plans alternating in one process, "
               f"{REPS} turns of {CALLS} calls each after one warm-up", "library_sha256_16": digest, "plans": {}}
for d in PLANS:
    med = statistics.median(ms[d])
    res["plans"][d] = {"ms_per_batch": [round(v, 3) for v in ms[d]], "median_ms": round(med, 3), "min_ms": round(min(ms[d]), 3),
                       "max_ms": round(max(ms[d]), 3), "images_per_s_median": round(N / med * 1e3, 1)}
    print(f"{d:11s} median {med:8.3f} ms  [{min(ms[d]):.3f}, {max(ms[d]):.3f}]  {N / med * 1e3:9.1f} images/s")
f32, x3 = res["plans"]["float32"], res["plans"]["bfloat16x3"]
res["x3_over_f32_speedup_median"] = round(f32["median_ms"] / x3["median_ms"], 3)
res["x3_slowest_vs_f32_fastest"] = round(f32["min_ms"] / x3["max_ms"], 3)
res["deviation_from_f32_features"] = {d: {"max_over_rms_f32": dev[d][0], "rms_over_rms_f32": dev[d][1]} for d in dev}
print(f"bfloat16x3 over float32: {res['x3_over_f32_speedup_median']} x (medians), {res['x3_slowest_vs_f32_fastest']} x (slowest x3 "
      f"turn against fastest float32 turn); max|x3 - f32| / rms(f32) {dev['bfloat16x3'][0]:.3e}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
