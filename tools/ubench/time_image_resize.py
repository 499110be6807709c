#!/usr/bin/env python3
"""Time the loader's resize step three ways on the same decoded images, one process, alternating rounds:
  (a) host:            Pillow crop + LANCZOS resize + np.array on a thread pool (dataloader._load_one without the file decode)
  (b) device, copies:  DeviceResizer.upload + the two kernels + the download, per chunk of 64 images
  (b) device, resident: the decoded images already in device memory (every cluster after the first): kernels + download
and the two kernels alone (HIP events), as GB/s on compulsory bytes (cropped input + 8-bit intermediate written and read +
output).  One warm-up round, then TI_ROUNDS timed rounds; every round's time is printed, not the best.  Prints one JSON line.
usage: time_image_resize.py   (TI_N, TI_H, TI_W, TI_MAX_DIM, TI_THREADS, TI_ROUNDS in the environment change the workload)"""
import json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from PIL import Image
from shoeprint_image_retrieval_amd import synth
from shoeprint_image_retrieval_amd.image_resize import DeviceResizer

N, H, W = int(os.environ.get("TI_N", 256)), int(os.environ.get("TI_H", 2400)), int(os.environ.get("TI_W", 1200))
MAX_DIM, THREADS = int(os.environ.get("TI_MAX_DIM", 800)), int(os.environ.get("TI_THREADS", 16))
ROUNDS, CHUNK, HBM_GBS = int(os.environ.get("TI_ROUNDS", 5)), 64, 8000.0
scale = MAX_DIM / max(H, W)
size = (int(W * scale), int(H * scale))
box = (0, 0, W, H)

pils = [Image.fromarray(synth.shoeprint_image(77, i, 320, 160)).resize((W, H), Image.Resampling.BICUBIC) for i in range(N)]
arrays = [np.array(p) for p in pils]
resizer = DeviceResizer()
dev = resizer.dev


def host():
    with ThreadPoolExecutor(THREADS) as pool:
        return list(pool.map(lambda p: np.array(p.crop((0, 0, W, H)).resize(size, Image.Resampling.LANCZOS)), pils))


def device_with_copies():
    out = []
    for s in range(0, N, CHUNK):
        part = arrays[s: s + CHUNK]
        out += resizer.resize(part, [box] * len(part), [size] * len(part))
    return out


residents = [resizer.upload(arrays[s: s + CHUNK]) for s in range(0, N, CHUNK)]


def device_resident():
    out = []
    for r in residents:
        out += resizer.resize_resident(r, [box] * len(r.shapes), [size] * len(r.shapes))
    return out


def kernels_ms():
    total = 0.0
    for r in residents:
        plan = resizer.plan(r, [box] * len(r.shapes), [size] * len(r.shapes))
        out, ws = dev.empty_bytes(plan.out_bytes), dev.empty_bytes(max(plan.workspace_bytes, 256))
        items = dev.to_device(np.frombuffer(plan.items, dtype=np.uint8).copy())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        resizer.lib.check(resizer.lib.spr_image_resize_u8(dev.ptr(r.buf), dev.ptr(out), dev.ptr(items), plan.n, 1,
                                                          dev.ptr(resizer._tables_dev()), plan.blocks, dev.ptr(ws), dev.stream()))
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
    return total


paths = {"host_pillow": host, "device_with_copies": device_with_copies, "device_resident": device_resident}
want = host()
for name in ("device_with_copies", "device_resident"):
    got = paths[name]()
    assert len(got) == N and all(np.array_equal(a, b) for a, b in zip(want, got)), f"{name} differs from Pillow"
seconds = {k: [] for k in paths}
kernel = []
for rnd in range(ROUNDS + 1):
    for name, call in paths.items():
        dev.synchronize()
        t0 = time.perf_counter()
        call()
        dev.synchronize()
        if rnd:
            seconds[name].append(time.perf_counter() - t0)
    ms = kernels_ms()
    if rnd:
        kernel.append(ms)
compulsory = N * (H * W + 2 * H * size[0] + size[0] * size[1])
gbs = [compulsory / (ms * 1e-3) / 1e9 for ms in kernel]
print(json.dumps({
    "workload": {"images": N, "mode": "L", "decoded": [H, W], "resized": [size[1], size[0]], "chunk": CHUNK,
                 "host_threads": THREADS, "host_cpus": len(os.sched_getaffinity(0)), "rounds": ROUNDS},
    "bytes_equal_to_pillow": True,
    **{k + "_s": [round(v, 4) for v in t] for k, t in seconds.items()},
    **{k + "_images_per_s_median": round(N / float(np.median(t)), 1) for k, t in seconds.items()},
    "kernels_ms": [round(v, 3) for v in kernel],
    "kernels_compulsory_bytes": compulsory,
    "kernels_gb_per_s": [round(v, 1) for v in gbs],
    "kernels_fraction_of_8tb_per_s": [round(v / HBM_GBS, 4) for v in gbs],
}))
