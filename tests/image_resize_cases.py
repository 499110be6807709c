"""Checks of the device crop + LANCZOS resize (csrc/image_resize.hip, image_resize.py), shared by the CPU-emulation tests and
the MI355X tests.  The oracle is Pillow itself, called live: ``Image.fromarray(a).crop(box).resize(size, LANCZOS)`` is what
the reference's loader runs.  Every comparison is byte equality.

Inputs are seeded random bytes whose right half is thresholded to 0 / 255: hard edges make the Lanczos lobes overshoot, so
both clamps (at 0 and at 255, after each pass) are exercised; the cases that say so assert it on Pillow's own output.
"""

import ctypes as C

import numpy as np
import pytest
from PIL import Image

import dataset_util
from shoeprint_image_retrieval_amd import _lib
from shoeprint_image_retrieval_amd.image_resize import DeviceResizer, crop_box, lanczos_tables

GUARD = 4096  # poison bytes on each side of a buffer
POISON = 0xA7

# (h, w, scale, asserts that Pillow's output holds both 0 and 255)
SINGLE = [
    (97, 53, 0.37, False),       # downscale
    (41, 77, 1.9, True),         # upscale
    (50, 20, 1.02, True),        # 51 x 20: horizontal pass skipped
    (20, 50, 1.02, True),        # vertical pass skipped
    (64, 40, 1.0, True),         # copy
    (7, 5, 0.3, False),          # 2 x 1
    (19, 200, 0.11, False),      # wide and thin
    (120, 64, 0.999, True),      # near-identity
    (40, 1200, 1 / 30, False),   # 1 x 40, 181 taps: a window wider than the staged chunk of a row
    # tile extents plus one.  Horizontal tile: 32 source rows x 64 output columns; vertical tile: 8 output rows x 256 bytes
    (33, 514, 0.5, False),       # 16 x 257: 33 source rows, 257 output columns = 257 bytes of a grey row
    (18, 130, 0.5, False),       # 9 x 65: 9 output rows, 65 output columns
    (70, 36, 0.5, False),        # 35 x 18: vertical windows of 33 and more source rows, past one staged chunk of 32
]
SINGLE_IDS = [f"{h}x{w}-{s:.3g}" for h, w, s, _ in SINGLE]


def image(seed, h, w, channels):
    """Random bytes; the right half (at least one column) thresholded to 0 / 255."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w) if channels == 1 else (h, w, channels), dtype=np.uint8)
    half = w // 2 if w > 1 else 0
    a[:, half:] = np.where(a[:, half:] >= 128, 255, 0)
    return a


def pillow(a, box, size):
    """box (x, y, w, h); size (out_w, out_h)."""
    x, y, w, h = box
    return np.array(Image.fromarray(a).crop((x, y, x + w, y + h)).resize(size, Image.Resampling.LANCZOS))


def check_single(resizer, h, w, scale, channels, clamps):
    a = image(1000 * h + w, h, w, channels)
    size = (int(w * scale), int(h * scale))
    want = pillow(a, (0, 0, w, h), size)
    if clamps:
        assert (want == 0).any() and (want == 255).any(), "this input does not reach both clamps"
    (got,) = resizer.resize([a], [(0, 0, w, h)], [size])
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"


def check_crop(resizer, channels):
    """The crop ratios of the loader tests on an odd-sized image, down and up."""
    ratios = dataset_util.CASES[0]["crop"]
    assert ratios == [0.1, 0.2]
    h, w = 131, 87
    a = image(5, h, w, channels)
    box = crop_box(w, h, ratios)
    assert box == (17, 13, 53, 105)
    for scale in (0.61, 1.3, 1.0):
        size = (int(box[2] * scale), int(box[3] * scale))
        (got,) = resizer.resize([a], [box], [size])
        assert np.array_equal(got, pillow(a, box, size)), scale


RAGGED = [(60, 31, 0.5), (45, 80, 0.5), (60, 31, 0.5), (33, 33, 1.4), (90, 17, 1.0), (25, 64, 0.7), (60, 40, 0.5)]


def ragged_batch(channels):
    images = [image(40 + i, h, w, channels) for i, (h, w, _) in enumerate(RAGGED)]
    boxes = [(1, 2, w - 2, h - 3) if i % 2 else (0, 0, w, h) for i, (h, w, _) in enumerate(RAGGED)]
    sizes = [(int(b[2] * s), int(b[3] * s)) for b, (_, _, s) in zip(boxes, RAGGED)]
    assert len({(h, w) for h, w, _ in RAGGED}) >= 4 and len(RAGGED) >= 6
    return images, boxes, sizes


def check_ragged(resizer, channels):
    """Seven images of six sizes in one call; items 0 and 2 share both size pairs, items 0 and 6 the vertical one."""
    images, boxes, sizes = ragged_batch(channels)
    tables_before = len(resizer._table_at)
    got = resizer.resize(images, boxes, sizes)
    pairs = {(b[2], s[0]) for b, s in zip(boxes, sizes) if b[2] != s[0]} | {(b[3], s[1]) for b, s in zip(boxes, sizes) if b[3] != s[1]}
    assert len(resizer._table_at) - tables_before <= len(pairs), "a size pair got more than one table"
    for i, (a, box, size) in enumerate(zip(images, boxes, sizes)):
        assert np.array_equal(got[i], pillow(a, box, size)), f"item {i}"


def check_guard_bands(resizer, channels):
    """Poison on both sides of the output buffer and of the workspace stays untouched."""
    dev = resizer.dev
    images, boxes, sizes = ragged_batch(channels)
    resident = resizer.upload(images)
    plan = resizer.plan(resident, boxes, sizes)
    assert plan.workspace_bytes > 0
    bufs = []
    for nbytes in (plan.out_bytes, plan.workspace_bytes):
        bufs.append(dev.to_device(np.full(nbytes + 2 * GUARD, POISON, dtype=np.uint8)))
    resizer.run(plan, resident, out=dev.narrow0(bufs[0], GUARD, plan.out_bytes),
                workspace=dev.narrow0(bufs[1], GUARD, plan.workspace_bytes))
    dev.synchronize()
    for name, buf, nbytes in (("output", bufs[0], plan.out_bytes), ("workspace", bufs[1], plan.workspace_bytes)):
        host = dev.to_host(buf)
        assert (host[:GUARD] == POISON).all(), f"bytes before the {name} buffer were written"
        assert (host[GUARD + nbytes:] == POISON).all(), f"bytes after the {name} buffer were written"
    out = dev.to_host(bufs[0])[GUARD: GUARD + plan.out_bytes]
    for i, (a, box, size) in enumerate(zip(images, boxes, sizes)):
        n = size[0] * size[1] * channels
        want = pillow(a, box, size)
        assert np.array_equal(out[plan.out_offsets[i]: plan.out_offsets[i] + n], want.reshape(-1)), f"item {i}"
        # the padding between two results belongs to the output buffer but to no item
        end = plan.out_offsets[i + 1] if i + 1 < len(images) else plan.out_bytes
        assert (out[plan.out_offsets[i] + n: end] == POISON).all(), f"bytes after item {i} were written"


def check_argument_errors(resizer):
    lib, dev = resizer.lib, resizer.dev
    a = image(1, 20, 10, 1)
    with pytest.raises(ValueError, match="height and width must be > 0"):
        resizer.resize([a], [(0, 0, 10, 20)], [(0, 5)])
    with pytest.raises(ValueError, match="height and width must be > 0"):
        resizer.resize([a], [(0, 0, 10, 20)], [(4, 0)])
    with pytest.raises(ValueError):
        lanczos_tables(10, 0)
    # the C layout refuses the same item, a box outside the image, and a pass without its table
    items = (_lib.ImageResizeItem * 1)()
    ws, blocks = C.c_size_t(0), (C.c_int32 * 2)()

    def layout(**kw):
        it = items[0]
        it.in_off = it.out_off = 0
        it.in_h, it.in_w, it.in_stride = 20, 10, 10
        it.box_x, it.box_y, it.box_w, it.box_h = 0, 0, 10, 20
        it.out_w, it.out_h, it.htab, it.vtab, it.hk, it.vk = 10, 20, -1, -1, 0, 0
        for k, v in kw.items():
            setattr(it, k, v)
        return lib.spr_image_resize_layout(C.cast(items, C.c_void_p), 1, 1, C.byref(ws), blocks)

    assert layout() == _lib.SPR_OK and (blocks[0], blocks[1]) == (0, 3)
    assert layout(out_w=0) == _lib.SPR_ERR_ARG
    assert b"must be > 0" in lib.spr_last_error()
    assert layout(box_x=1) == _lib.SPR_ERR_ARG
    assert layout(out_w=5) == _lib.SPR_ERR_ARG  # the width changes but there is no horizontal table
    assert lib.spr_image_resize_layout(None, 1, 1, C.byref(ws), blocks) == _lib.SPR_ERR_ARG
    assert lib.spr_image_resize_layout(None, 0, 1, C.byref(ws), blocks) == _lib.SPR_OK and ws.value == 0
    assert lib.spr_image_resize_layout(C.cast(items, C.c_void_p), 1, 2, C.byref(ws), blocks) == _lib.SPR_ERR_ARG
    # the call itself: null pointers with n > 0, nothing at n == 0
    assert layout() == _lib.SPR_OK
    buf = dev.to_device(np.zeros(4096, np.uint8))
    p = dev.ptr(buf)
    good = [p, p, p, 1, 1, p, blocks, p, dev.stream()]
    for k in (0, 1, 2, 5, 7):
        args = list(good)
        args[k] = None
        assert lib.spr_image_resize_u8(*args) == _lib.SPR_ERR_ARG, k
        assert b"null pointer" in lib.spr_last_error()
    args = list(good)
    args[6] = None
    assert lib.spr_image_resize_u8(*args) == _lib.SPR_ERR_ARG
    assert lib.spr_image_resize_u8(None, None, None, 0, 1, None, None, None, dev.stream()) == _lib.SPR_OK
    assert lib.spr_image_resize_u8(p, p, p, -1, 1, p, blocks, p, dev.stream()) == _lib.SPR_ERR_ARG
    assert resizer.resize([], [], []) == []
