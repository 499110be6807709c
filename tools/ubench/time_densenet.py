#!/usr/bin/env python3
"""Images/s of the DenseNet_201 extractor at 512x256, batch 32, blocks 9 and 12: the float32, bfloat16 and float16 plans
alternated in one process (warm-up for each, then REPS timed repetitions of each in turn, device events around every one),
with the spread over the repetitions and the real / issued GFLOP per image from densenet_ops().
    python time_densenet.py [--json OUT]     # OUT: profiles/r05_extractor_densenet16.json
    TD_ONLY=bfloat16:12 python time_densenet.py   # one plan only (a kernel trace of it)"""
import glob, hashlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from shoeprint_image_retrieval_amd import _lib, network
B, H, W = int(os.environ.get("TR_B", 32)), 512, 256
REPS, WARM = int(os.environ.get("TD_REPS", 7)), 2
args = sys.argv[1:]
out_json = args[args.index("--json") + 1] if "--json" in args else None
only = os.environ.get("TD_ONLY", "")
PEAK = {"float32": 157.3, "bfloat16": 2516.6, "float16": 2516.6}  # matrix-core peaks, TFLOP/s


def sclk_mhz():
    """current shader clock levels of the cards, from sysfs (plain reads; best effort)"""
    out = []
    for f in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            out += [int(l.split(":")[1].strip().lower().replace("mhz", "").replace("*", "")) for l in open(f).read().splitlines() if l.rstrip().endswith("*")]
        except (OSError, ValueError):
            pass
    return out


def gflop(ops, half):
    """(real, issued) GFLOP per 512x256 image: issued counts the stem's K padded to 160 and, per plan, the padded tiles - the
    f32 plan computes the 3x3 layers 64 channels wide, a 16-bit plan stages whole 32-channel k-steps and pads nothing else."""
    h, w = 128, 64  # behind conv0 (256 x 128) and pool0
    real = 2 * 147 * 64 * 256 * 128
    issued = 2 * (160 if half else 147) * 64 * 256 * 128
    for op in ops:
        if op["kind"] == 1:
            real += 2 * op["cin"] * 128 * h * w; issued += 2 * op["cin"] * 128 * h * w
        elif op["kind"] == 2:
            real += 2 * 9 * 128 * 32 * h * w; issued += 2 * 9 * 128 * (32 if half else 64) * h * w
        elif op["kind"] == 3:
            real += 2 * op["cin"] * op["cout"] * h * w; issued += 2 * op["cin"] * op["cout"] * h * w
            h, w = h // 2, w // 2
    return real / 1e9, issued / 1e9


lib = _lib.load_library()
imgs = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda")
records = []
for block in (9, 12):
    plans = [c for c in ("float32", "bfloat16", "float16") if not only or only == f"{c}:{block}"]
    models = {c: network.Model({"model": {"type": "DenseNet_201", "clahe_clip_limit": 2.0, "clahe_tile_grid_size": [8, 8]},
                                "mi355x": {"extractor_dtype": c}}, block) for c in plans}
    for m in models.values():
        for _ in range(WARM):
            out = m.extract_device(imgs)
    torch.cuda.synchronize()
    ms = {c: [] for c in plans}
    for _ in range(REPS):  # alternated: a drift of the clocks hits every plan alike
        for c, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = m.extract_device(imgs); e1.record(); torch.cuda.synchronize()
            ms[c].append(e0.elapsed_time(e1))
    clocks = sclk_mhz()
    for c, m in models.items():
        real, issued = gflop(m.densenet_ops(), c != "float32")
        rate = [B / t * 1e3 for t in ms[c]]
        med = statistics.median(rate)
        rec = {"model": "DenseNet_201", "block": block, "plan": c, "batch": B, "image_hw": [H, W], "reps": REPS, "warmup": WARM,
               "images_per_s_median": round(med, 1), "images_per_s_min": round(min(rate), 1), "images_per_s_max": round(max(rate), 1),
               "ms_per_batch_median": round(statistics.median(ms[c]), 3), "gflop_per_image_real": round(real, 3),
               "gflop_per_image_issued": round(issued, 3), "issued_tflops": round(issued * med / 1e3, 1),
               "share_of_matrix_core_peak": round(issued * med / 1e3 / PEAK[c], 4), "launches_per_batch": None,
               "sclk_mhz_after": clocks, "out_shape": list(out.shape)}
        n_ops = m.densenet_ops()
        # one launch per convolution, stem + max pool, the transitions' pools, the closing layout change
        rec["launches_per_batch"] = sum(1 for o in n_ops if o["kind"] in (1, 2, 3)) + sum(1 for o in n_ops if o["kind"] == 3) + 3
        records.append(rec)
        print(f"DenseNet_201 features[:{block}] {c:8s} batch {B}: {med:8.1f} images/s (min {min(rate):.1f}, max {max(rate):.1f} over {REPS}); "
              f"{real:.2f} GFLOP per image real, {issued:.2f} issued = {issued * med / 1e3:.1f} TFLOP/s issued "
              f"({issued * med / 1e3 / PEAK[c]:.1%} of the {PEAK[c]:.0f} TFLOP/s matrix-core peak), {rec['launches_per_batch']} launches")
    if "float32" in ms:
        f32 = next(r for r in records if r["block"] == block and r["plan"] == "float32")
        for c in plans:
            if c == "float32":
                continue
            r = next(r for r in records if r["block"] == block and r["plan"] == c)
            r["speedup_over_float32_median"] = round(r["images_per_s_median"] / f32["images_per_s_median"], 2)
            r["speedup_over_float32_worst_case"] = round(r["images_per_s_min"] / f32["images_per_s_max"], 2)  # slowest against fastest
            print(f"  {c} / float32 at block {block}: {r['speedup_over_float32_median']:.2f} x (slowest repetition against float32's "
                  f"fastest: {r['speedup_over_float32_worst_case']:.2f} x)")
    for m in models.values():
        m.close()
if out_json:
    json.dump({"what": "whole-extractor time (spr_densenet_forward through Model.extract_device, images in HBM), device events around "
                       "every repetition, the three plans alternated in one process on one MI355X",
               "device": torch.cuda.get_device_name(0), "library_sha256": hashlib.sha256(open(lib.path, "rb").read()).hexdigest(),
               "records": records}, open(out_json, "w"), indent=1)
