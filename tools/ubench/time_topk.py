"""Times spr_topk_rows beside spr_rank_true_match, and spr_maps_peak, on one MI355X: HIP events around 20 back-to-back calls
after a warm-up, one process, the in-tree library (its sha256 goes into the record).

    python tools/ubench/time_topk.py [profiles/r05_topk.json]
"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from shoeprint_image_retrieval_amd import _lib
from shoeprint_image_retrieval_amd.device import TorchDevice

lib = _lib.load_library()
dev = TorchDevice()
REPS = 20

def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS  # microseconds per call

rec = {"library_sha256": hashlib.sha256(open(lib.path, "rb").read()).hexdigest(), "device": torch.cuda.get_device_name(0),
       "repetitions": REPS, "timer": "HIP events around 20 back-to-back calls after 3 warm-up calls, one process", "topk": [], }
for (nq, ng, k) in ((100, 1500, 10), (64, 12500, 20)):
    s = torch.rand((nq, ng), device="cuda", dtype=torch.float32)
    o_s = torch.empty((nq, k), device="cuda", dtype=torch.float32)
    o_i = torch.empty((nq, k), device="cuda", dtype=torch.int32)
    match = torch.randint(0, ng, (nq,), device="cuda", dtype=torch.int32)
    ranks = torch.empty((nq,), device="cuda", dtype=torch.int32)
    st = dev.stream()
    t_topk = timed(lambda: lib.check(lib.spr_topk_rows(s.data_ptr(), ng, nq, ng, None, 0, k, o_s.data_ptr(), o_i.data_ptr(), st)))
    t_rank = timed(lambda: lib.check(lib.spr_rank_true_match(s.data_ptr(), ng, nq, ng, match.data_ptr(), ranks.data_ptr(), st)))
    ref = torch.topk(s, k, dim=1)
    assert torch.equal(ref.values, o_s)
    rec["topk"].append({"shape": [nq, ng], "k": k, "spr_topk_rows_us": round(t_topk, 2), "spr_rank_true_match_us": round(t_rank, 2)})
p, c, h, w = 64, 256, 124, 60
maps = torch.randn((p, c, h, w), device="cuda", dtype=torch.float32)
o_s = torch.empty((p,), device="cuda", dtype=torch.float32)
o_yx = torch.empty((p, 2), device="cuda", dtype=torch.int32)
t = timed(lambda: lib.check(lib.spr_maps_peak(maps.data_ptr(), p, c, h, w, o_s.data_ptr(), o_yx.data_ptr(), dev.stream())))
nbytes = maps.numel() * 4
rec["maps_peak"] = {"shape": [p, c, h, w], "us": round(t, 2), "bytes_read": nbytes, "read_tb_per_s": round(nbytes / t / 1e6, 3),
                    "share_of_8_tb_per_s_peak": round(nbytes / t / 1e6 / 8.0, 4)}
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r05_topk.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(rec, open(out, "w"), indent=1)
print(json.dumps(rec))
