#!/usr/bin/env python3
"""Host route against resident route, and the two kernels of csrc/resident.hip, on one GPU.

    python tools/ubench/time_device_resident.py cluster [G] [out.json]    # extractor -> compare_maps, config 2's shape
    python tools/ubench/time_device_resident.py variants [out.json]       # retrieve(k = 10) under the reference's variant lists
    python tools/ubench/time_device_resident.py kernels [out.json]        # spr_items_gather / spr_block_scatter / a D2D copy

Protocol of the first two: one warm-up of each route, then three alternating repetitions in one process, a device
synchronise inside every timed window; medians and the spread (max - min) are reported, and the bytes each route moves in
each direction, counted from the shapes.  ``kernels`` times with events around five launches after a warm-up and is the
program to put behind ``rocprofv3 --kernel-trace --stats --``.
"""

import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from shoeprint_image_retrieval_amd import _lib, similarity  # noqa: E402
from shoeprint_image_retrieval_amd.features import FeatureSet  # noqa: E402


def timed(dev, fn):
    dev.synchronize()
    t0 = time.perf_counter()
    out = fn()
    dev.synchronize()
    return time.perf_counter() - t0, out


def alternate(dev, routes, reps=3):
    """{name: [seconds, ...]} and the last result of every route."""
    last = {}
    for name, fn in routes.items():  # warm-up
        last[name] = fn()
    dev.synchronize()
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            t, last[name] = timed(dev, fn)
            times[name].append(t)
    return times, last


def summary(times):
    return {name: {"median_s": statistics.median(t), "spread_s": max(t) - min(t), "all_s": t} for name, t in times.items()}


def cluster(g=1500, q=100):
    from shoeprint_image_retrieval_amd.network import Model

    cfg = {"model": {"type": "VGG16", "clahe_clip_limit": 2.0, "clahe_tile_grid_size": [8, 8]},
           "comparison": {"n_processes": 1, "rotations": None, "scales": None}}
    model = Model(cfg, 16)
    dev = model.dev
    rng = np.random.default_rng(10)
    q_img = list(rng.integers(0, 256, (q, 512, 256), dtype=np.uint8))
    g_img = list(rng.integers(0, 256, (g, 512, 256), dtype=np.uint8))
    match = [i % g for i in range(q)]
    scorer = similarity.NccScorer()

    def host():
        return similarity.compare_maps(model.get_multiple_feature_maps(q_img, progress=False),
                                       model.get_multiple_feature_maps(g_img, progress=False), match, cfg, scorer=scorer)

    def resident():
        return similarity.compare_maps(model.get_multiple_feature_maps_device(q_img, progress=False),
                                       model.get_multiple_feature_maps_device(g_img, progress=False), match, cfg, scorer=scorer)

    times, last = alternate(dev, {"host": host, "resident": resident})
    c, h, w = model.output_shape(512, 256)
    feat, img = 4 * c * h * w * (q + g), 512 * 256 * (q + g)
    return {"workload": f"grey 512x256, VGG16 features[:16] -> [{c},{h},{w}], Q = {q} x G = {g}, compare_maps",
            "ranks_equal": bool(np.array_equal(last["host"], last["resident"])), **summary(times),
            "bytes": {"host": {"h2d": img + feat + 4 * q * g + 4 * q, "d2h": feat + 4 * q * g + 4 * q},
                      "resident": {"h2d": img + 4 * (q + g) + 4 * q, "d2h": 4 * q}}}


def variants(q=32, g=256, k=10):
    rot, sc = [-15, -9, -3, 3, 9, 15, 180], [1.02, 1.04, 1.08]
    cfg = {"comparison": {"n_processes": 1, "rotations": rot, "scales": sc}}
    scorer = similarity.NccScorer(storage="bfloat16", matrix_core_peaks=True)
    dev = scorer.dev
    rng = np.random.default_rng(11)
    ql = [np.abs(rng.standard_normal((176, 32, 16))).astype(np.float32) for _ in range(q)]
    gl = [np.abs(rng.standard_normal((176, 32, 16))).astype(np.float32) for _ in range(g)]
    qs, gs = FeatureSet.from_host(dev, ql), FeatureSet.from_host(dev, gl)
    times, last = alternate(dev, {"host": lambda: similarity.retrieve(ql, gl, cfg, k=k, scorer=scorer),
                                  "resident": lambda: similarity.retrieve(qs, gs, cfg, k=k, scorer=scorer)})
    a, b = last["host"], last["resident"]
    same = all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ("index", "score", "variant", "peak_yx", "offset"))
    feat = 4 * 176 * 32 * 16 * (q + g)
    return {"workload": f"[176,32,16] maps stored as bfloat16, Q = {q} x G = {g}, retrieve(k = {k}), rotations {rot} x scales {sc} "
                        "(features already where the route wants them: lists on the host / FeatureSets in HBM)",
            "shortlists_equal": bool(same), **summary(times),
            "bytes": {"host": {"h2d": feat + 4 * q * g + 2 * 4 * q * g, "d2h": 3 * 4 * q * g + 2 * 4 * q * k},
                      "resident": {"h2d": 4 * (q + g) + 2 * 4 * q * g + 4 * q * k, "d2h": 4 * 4 * q * k}}}


def kernels():
    import torch

    lib = _lib.load_library()
    scorer = similarity.NccScorer(library=lib)
    dev = scorer.dev
    n, elems = 256, 256 * 128 * 64
    src = torch.randn(n + 8, elems, device=dev.device)
    index = dev.to_device(np.random.default_rng(0).permutation(n + 8)[:n].astype(np.int32))
    out32 = torch.empty(n, elems, device=dev.device)
    out16 = torch.empty(n, elems, device=dev.device, dtype=torch.bfloat16)
    copied = torch.empty(n, elems, device=dev.device)
    mat, sub = torch.zeros(100, 1500, device=dev.device), torch.rand(100, 256, device=dev.device)
    rows = dev.to_device(np.arange(100, dtype=np.int32))
    cols = dev.to_device(np.random.default_rng(1).permutation(1500)[:256].astype(np.int32))
    calls = {
        "gather_f32": (lambda: lib.check(lib.spr_items_gather(dev.ptr(src), elems, dev.ptr(index), n, dev.ptr(out32), _lib.F32, dev.stream())), 8 * n * elems),
        "gather_bf16": (lambda: lib.check(lib.spr_items_gather(dev.ptr(src), elems, dev.ptr(index), n, dev.ptr(out16), _lib.BF16, dev.stream())), 6 * n * elems),
        "d2d_copy_f32": (lambda: copied.copy_(src[:n]), 8 * n * elems),
        "scatter_max_100x256": (lambda: lib.check(lib.spr_block_scatter(dev.ptr(mat), 1500, dev.ptr(sub), 256, dev.ptr(rows), 100, dev.ptr(cols), 256, 1, dev.stream())), 3 * 4 * 100 * 256),
    }
    res = {}
    for name, (fn, nbytes) in calls.items():
        fn()
        dev.synchronize()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res[name] = {"median_ms": statistics.median(ms), "all_ms": ms, "compulsory_bytes": nbytes,
                     "GB_per_s": nbytes / (statistics.median(ms) * 1e-3) / 1e9}
    assert torch.equal(out32, src[index.long()]) and torch.equal(out16, src[index.long()].to(torch.bfloat16))
    return {"workload": f"gather {n} items of [256,128,64] float32 (permuted index) to float32 / bfloat16; scatter-max of a 100 x 256 block "
                        "into [100,1500]; torch copy_ of the same float32 bytes", **res}


if __name__ == "__main__":
    what, rest = sys.argv[1], sys.argv[2:]
    out = rest.pop() if rest and rest[-1].endswith(".json") else None
    result = {"cluster": lambda: cluster(*(int(v) for v in rest)), "variants": variants, "kernels": kernels}[what]()
    print(json.dumps(result, indent=1))
    if out:
        with open(out, "w") as fh:
            json.dump(result, fh, indent=1)
