"""Per-layer (teacher-forced) parity of the 16-bit EfficientNet and ResNet extractors under emulation (tests/layer_cases.py),
with batches of differing images, tiles that straddle two images, guard bands around every buffer, and sensitivity tests that
prove the per-layer check catches the subtle errors the end-to-end statistical check cannot."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_cases as lc
from emu_util import emu_library
from host_device import HostDevice
from oracle import effnet_oracle


@pytest.mark.parametrize("arch,block,hw,n,compute", [
    ("EfficientNetV2_M", 6, (40, 36), 3, "bfloat16"),
    ("EfficientNetV2_S", 5, (40, 32), 2, "float16"),
    ("EfficientNet_B1", 6, (44, 36), 2, "bfloat16"),   # 5x5 depthwise, the expansion-1 stage
    ("EfficientNetV2_M", 7, (32, 32), 2, "float16"),   # stage 6 at 1 x 1: an SE mean over one pixel, padding on every side
    ("ResNet50", 7, (40, 36), 3, "bfloat16"),
    ("ResNet50", 5, (34, 47), 2, "float16"),
])
def test_emu_per_layer_parity_16bit(arch, block, hw, n, compute):
    lc.check_layers(arch, block, hw, n, compute, HostDevice(), emu_library())


def test_emu_per_layer_parity_resnet_wide_tiles():
    """ResNet50[:5] with the 128-channel tiles forced (SPR_GEMM16_BN=128, read once per process: a child process)."""
    env = dict(os.environ, SPR_GEMM16_BN="128")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "per_layer_parity_16bit and ResNet50-5"], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]


def test_emu_trace_layouts_of_f32_plans_and_argument_refusals():
    import f32_layer_cases as fc

    lib = emu_library()
    m = lc.make_model("EfficientNetV2_S", 3, "bfloat16", HostDevice(), lib)
    m32 = lc.make_model("ResNet50", 5, "float32", HostDevice(), lib)
    try:
        import ctypes as C

        total = C.c_size_t(0)
        # a float32 plan traces: SPR_OK, the expected records (float32 NHWC, the last NCHW), total_bytes their aligned sum
        assert len(fc.check_layout(m32, lib, 1, (40, 40))) == 1 + len(m32.conv_specs())
        assert lib.spr_resnet_trace_layout(m32.handle, 1, 40, 16, None, C.byref(total)) == -1  # SPR_ERR_ARG: at least 32 x 32
        assert lib.spr_effnet_trace_layout(m.handle, 1, 16, 40, None, C.byref(total)) == -1  # SPR_ERR_ARG: at least 32 x 32
        assert lib.spr_effnet_trace_layout(m.handle, 1, 40, 40, None, C.byref(total)) == len(m.effnet_ops()) and total.value > 0
    finally:
        m.close()
        m32.close()


# ---------------------------------------------------------------------------------------------------- sensitivity
@functools.lru_cache(maxsize=None)
def _trace(compute):
    """A real emulator trace: EfficientNetV2_S[:5] at 40 x 32, a print and a constant image - fused stages with expansion 1
    (SiLU in front of a residual) and 4, MBConv stages with squeeze-excitation."""
    keep = {}
    lc.check_layers("EfficientNetV2_S", 5, (40, 32), 2, compute, HostDevice(), emu_library(), keep=keep)
    return keep


def _first(ops, pred):
    return next(i for i in range(1, len(ops) - 1) if pred(i, ops[i]))


def _store(y: torch.Tensor, compute, cout_p, mode="rne"):
    """float64 NCHW (real channels) -> the stored 16-bit NHWC record (padded channels 0)."""
    v = y.to(torch.float32).numpy().transpose(0, 2, 3, 1)
    out = np.zeros(v.shape[:3] + (cout_p,), np.uint16)
    out[..., : v.shape[3]] = lc.f32_to_bits(v, compute, mode)
    return out


def _mutate(keep, what):
    """(layer, new record) of one mutation, restated in float64 from the layer's traced inputs."""
    ctx, raw = keep["ctx"], keep["trace"].raw
    ops, params, compute, eps = ctx["ops"], ctx["params"], ctx["compute"], ctx["bn_eps"]
    scaled = lambda i, o: o["kind"] == 0 and ops[i - 1]["kind"] == 2

    def restate(i, x=None, block_in=None, scale=None, op=None, p=None):
        x0, b0, s0 = lc.effnet_inputs(ops, raw, i, compute)
        return effnet_oracle.step16(op or ops[i], p or params[i], x0 if x is None else x, b0 if block_in is None else block_in,
                                    s0 if scale is None else scale, eps, compute, dtype=torch.float64)

    if what == "scaled operand not re-rounded":
        i = _first(ops, scaled)
        x, b, s = lc.effnet_inputs(ops, raw, i, compute)
        y = effnet_oracle.step16(ops[i], params[i], x * s, b, None, eps, compute, dtype=torch.float64)  # x * f unrounded
    elif what == "SiLU behind the residual":
        i = _first(ops, lambda i, o: o["kind"] == 0 and o["act"] == 2 and o["res"])
        y = F.silu(restate(i, op=dict(ops[i], act=0)))
    elif what == "image 0's factors for image 1":
        i = _first(ops, scaled)
        s = lc.effnet_inputs(ops, raw, i, compute)[2].clone()
        s[1] = s[0]
        y = restate(i, scale=s)
    elif what == "residual from the previous layer":
        i = _first(ops, lambda i, o: o["kind"] == 0 and o["res"] and ops[i - 1]["kind"] == 0 and not ops[i - 1]["block_end"])
        prev, cp = raw[i - 1], raw[i].shape[-1]
        wrong = prev.reshape(-1)[: raw[i].size].reshape(raw[i].shape)  # the previous tensor read with this layer's stride
        y = restate(i, block_in=lc._vals16(wrong, compute, ops[i]["cout"]))
    elif what == "round toward zero":
        i = _first(ops, lambda i, o: o["kind"] == 0 and not scaled(i, o))
        return i, _store(restate(i), compute, raw[i].shape[-1], "rtz")
    elif what == "depthwise weights rounded":
        i = _first(ops, lambda i, o: o["kind"] == 1)
        x = lc.effnet_inputs(ops, raw, i, compute)[0]
        wf, bf = effnet_oracle.fold16(ops[i], params[i], eps, compute)
        wf = effnet_oracle._round(wf, compute)
        y = F.silu(F.conv2d(x.double(), wf.double(), bf.double(), stride=ops[i]["stride"], padding=ops[i]["ks"] // 2,
                            groups=ops[i]["cin"]))
    elif what == "one bias off by one step":
        i = _first(ops, lambda i, o: o["kind"] == 0 and not scaled(i, o) and o["act"] == 2)
        _, bf = effnet_oracle.fold16(ops[i], params[i], eps, compute)
        c = int(np.argmax(np.abs(bf.numpy())))
        step = float(lc.ulp16(np.float64(bf[c]), compute))
        w, b, gamma, beta, mu, var = (np.array(a, dtype=np.float32) for a in params[i])
        beta[c] += np.float32(step)
        y = restate(i, p=(w, b, gamma, beta, mu, var))
    elif what == "padded channel nonzero":
        i = _first(ops, lambda i, o: o["kind"] == 0 and raw[i].shape[-1] > o["cout"])
        rec = raw[i].copy()
        rec[1, rec.shape[1] // 2, 0, ops[i]["cout"]] = lc.f32_to_bits(np.float32([0.5]), compute)[0]
        return i, rec
    else:
        raise KeyError(what)
    return i, _store(y, compute, raw[i].shape[-1])


MUTATIONS = ["scaled operand not re-rounded", "SiLU behind the residual", "image 0's factors for image 1",
             "residual from the previous layer", "round toward zero", "depthwise weights rounded", "one bias off by one step",
             "padded channel nonzero"]


@pytest.mark.parametrize("compute", ["bfloat16", "float16"])
@pytest.mark.parametrize("what", MUTATIONS)
def test_emu_per_layer_check_catches(what, compute):
    """Each mutation recomputes one layer from its traced inputs with the float64 restatement under that mutation, splices it
    into the real trace, and the per-layer check must flag THAT layer first (the layers behind it read its mutated output
    and may be flagged too; the layers in front of it are untouched and must pass)."""
    keep = _trace(compute)
    layer, rec = _mutate(keep, what)
    raw = list(keep["trace"].raw)
    assert not np.array_equal(raw[layer], rec), "the mutation changed nothing"
    raw[layer] = rec
    ctx = keep["ctx"]
    flagged = [i for i in range(layer + 2) if not lc.check_effnet_layer(ctx, raw, i).ok]
    assert flagged and flagged[0] == layer, (what, layer, flagged)
