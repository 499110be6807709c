#!/usr/bin/env python3
"""Images/s of the EfficientNetV2_M extractor (features[:block], the reference's run.toml default model) at 512x256, with
the flops of the real (unpadded) layers and of the layers as issued (channel counts padded to 64).  With --taps (see
time_taps) it times the tapped forward against the plain one and against one plain forward per tapped layer instead."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from shoeprint_image_retrieval_amd import network
B = int(os.environ.get("TR_B", 32))


def time_taps(argv):
    """--taps 4,6 [--dtype float32,bfloat16] [--reps 7] [--baseline-lib other/libshoeprint_mi355x.so] [--json out.json]:
    per compute type the tapped forward of EfficientNetV2_M[:max(taps)] against its plain forward and against one plain
    forward per tap (what scoring those layers costs without taps), and - with --baseline-lib - against the plain forward of
    another build of the library in the same process.  One warm-up, then `reps` rounds that run every case once, in turn;
    per case the median and the spread (min .. max) of the rounds, in ms per batch."""
    import argparse, ctypes, json, statistics
    from shoeprint_image_retrieval_amd import _lib

    class OtherBuild(_lib.Library):
        """Another build of the library, bound with the entry points it exports (an older one lacks those added since)."""
        def __init__(self, path):
            self.path, self.cdll = path, ctypes.CDLL(path)
            for name, (restype, argtypes) in _lib.SIGNATURES.items():
                fn = getattr(self.cdll, name, None)
                if fn is not None:
                    fn.restype, fn.argtypes = restype, argtypes
                    setattr(self, name, fn)

    ap = argparse.ArgumentParser()
    ap.add_argument("--taps", required=True)
    ap.add_argument("--dtype", default="float32,bfloat16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args(argv)
    taps = sorted(int(t) for t in a.taps.split(","))
    imgs = torch.randint(0, 256, (B, 512, 256), dtype=torch.uint8, device="cuda")
    results = []
    for dtype in a.dtype.split(","):
        cfg = {"model": {"type": "EfficientNetV2_M", "clahe_clip_limit": 2.0, "clahe_tile_grid_size": [8, 8]},
               "mi355x": {"extractor_dtype": dtype}}
        deep = network.Model(cfg, taps[-1])
        cuts = [network.Model(cfg, t) for t in taps[:-1]]
        cases = {"plain": lambda: deep.extract_device(imgs), "tapped": lambda: deep.extract_taps_device(imgs, taps),
                 "separate": lambda: [m.extract_device(imgs) for m in cuts + [deep]]}
        if a.baseline_lib:
            base = network.Model(cfg, taps[-1], library=OtherBuild(os.path.abspath(a.baseline_lib)))
            cases = {"baseline plain": lambda: base.extract_device(imgs), **cases}
        ms = {k: [] for k in cases}
        for rep in range(a.reps + 1):  # round 0: the warm-up
            for k, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                if rep:
                    ms[k].append(e0.elapsed_time(e1))
        row = {"model": f"EfficientNetV2_M[:{taps[-1]}]", "taps": taps, "dtype": dtype, "batch": B, "image": [512, 256], "reps": a.reps,
               "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}}
        med = {k: v["median"] for k, v in row["ms"].items()}
        row["tapped_over_plain"] = med["tapped"] / med["plain"]
        row["tapped_over_separate"] = med["tapped"] / med["separate"]
        if a.baseline_lib:
            row["plain_over_baseline_plain"] = med["plain"] / med["baseline plain"]
        results.append(row)
        print(json.dumps(row))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"command": "tools/ubench/time_effnet.py " + " ".join(argv),
                       "method": "one process; one warm-up round, then `reps` rounds that run every case once, in turn; device events "
                                 "around each call, so the call's output and workspace allocations are inside the timed region (the "
                                 "same in every case); ms per batch; 'baseline plain' = the plain forward of --baseline-lib",
                       "cases": results}, fh, indent=1)


if "--taps" in sys.argv:
    time_taps(sys.argv[1:])
    sys.exit(0)
for block in (4, 6):
    m = network.Model({"model": {"type": "EfficientNetV2_M", "clahe_clip_limit": 2.0, "clahe_tile_grid_size": [8, 8]}}, block)
    h, w, real, issued = 512, 256, 0.0, 0.0
    for op in m.effnet_ops():
        if op["kind"] == 2:
            continue
        if op["stride"] == 2:
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        if op["kind"] == 1:
            real += 2 * 9 * op["cin"] * h * w; issued += 2 * 9 * op["cin_p"] * h * w
        else:
            real += 2 * op["ks"] ** 2 * op["cin"] * op["cout"] * h * w
            issued += 2 * op["ks"] ** 2 * op["cin_p"] * op["cout_p"] * h * w
    imgs = torch.randint(0, 256, (B, 512, 256), dtype=torch.uint8, device="cuda")
    m.extract_device(imgs); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3): out = m.extract_device(imgs)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 3
    print(f"EfficientNetV2_M features[:{block}], batch {B}: {ms:.2f} ms -> {B / ms * 1e3:.1f} images/s; {real / 1e9:.2f} GFLOP per image "
          f"({issued / 1e9:.2f} issued with padded channels) = {real * B / ms / 1e9:.1f} TFLOP/s real, {issued * B / ms / 1e9:.1f} issued "
          f"({issued * B / ms / 1e9 / 157.3:.1%} of the fp32 MFMA peak), {len(m.effnet_ops())} layers, out {tuple(out.shape)}")
    m.close()

# DenseNet_201, all of `features` (block 12)
m = network.Model({"model": {"type": "DenseNet_201", "clahe_clip_limit": 2.0, "clahe_tile_grid_size": [8, 8]}}, 12)
h, w = 128, 64  # behind conv0 (256 x 128) and pool0
flops = 2 * 147 * 64 * 256 * 128
issued = flops
for op in m.densenet_ops():
    if op["kind"] == 1:
        flops += 2 * op["cin"] * 128 * h * w; issued += 2 * op["cin"] * 128 * h * w
    elif op["kind"] == 2:
        flops += 2 * 9 * 128 * 32 * h * w; issued += 2 * 9 * 128 * 64 * h * w
    elif op["kind"] == 3:
        flops += 2 * op["cin"] * op["cout"] * h * w; issued += 2 * op["cin"] * op["cout"] * h * w
        h, w = h // 2, w // 2
imgs = torch.randint(0, 256, (B, 512, 256), dtype=torch.uint8, device="cuda")
m.extract_device(imgs); torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(3): out = m.extract_device(imgs)
e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / 3
print(f"DenseNet_201 features[:12], batch {B}: {ms:.2f} ms -> {B / ms * 1e3:.1f} images/s; {flops / 1e9:.2f} GFLOP per image "
      f"({issued / 1e9:.2f} issued) = {flops * B / ms / 1e9:.1f} TFLOP/s real, {issued * B / ms / 1e9:.1f} issued "
      f"({issued * B / ms / 1e9 / 157.3:.1%} of the fp32 MFMA peak), {len(m.densenet_ops())} layers, out {tuple(out.shape)}")
