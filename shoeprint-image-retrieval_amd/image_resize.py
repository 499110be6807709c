"""Crop + LANCZOS resize of decoded 8-bit images on the device (reference dataloader.py:217-237).

The reference loads every image as ``image.crop(box).resize((int(w*scale), int(h*scale)), Image.Resampling.LANCZOS)``.
For modes "L" and "RGB" Pillow's resampler (Resample.c) is integer arithmetic once its coefficient tables exist, so the
host restates the tables (``lanczos_tables``: ``precompute_coeffs`` + ``normalize_coeffs_8bpc``, in Python floats with
``math.sin``, i.e. libm, as the C code) and ``spr_image_resize_u8`` (csrc/image_resize.hip) applies them to a ragged batch,
bit-identically to Pillow.  ``DeviceResizer`` caches the tables per (source size, output size) pair on the device, builds
the per-item descriptors, uploads decoded images (or takes images that are already resident) and returns host arrays.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2  # Resample.c: 8-bit pixels, 2 bits of headroom for the sum
_ALIGN = 256


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a = x * math.pi
        b = x / 3.0 * math.pi
        return (math.sin(a) / a) * (math.sin(b) / b)
    return 0.0


def lanczos_tables(in_size: int, out_size: int):
    """bounds int32 [out][2] (first source index, tap count), coefficients int32 [out][ksize] in 22-bit fixed point, ksize:
    precompute_coeffs (LANCZOS, support 3) followed by normalize_coeffs_8bpc of Resample.c."""
    if in_size < 1 or out_size < 1:
        raise ValueError("height and width must be > 0")
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        coeffs[xx, :xmax] = [int(-0.5 + w * one) if w < 0 else int(0.5 + w * one) for w in k]  # int(): toward zero, as (int)
        bounds[xx] = (xmin, xmax)
    if coeffs.min() < -(1 << 23) or coeffs.max() >= 1 << 23:  # the kernels multiply with the 24-bit multiplier
        raise ValueError(f"resize {in_size} -> {out_size}: a coefficient does not fit 24 bits")
    return bounds, coeffs, ksize


def crop_box(width: int, height: int, crop) -> tuple[int, int, int, int]:
    """(x, y, w, h) of dataloader.py:225-229: floor(size * ratio) pixels off each side."""
    ch = math.floor(height * crop[0])
    cw = math.floor(width * crop[1])
    return cw, ch, width - 2 * cw, height - 2 * ch


def _align(n: int) -> int:
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


class ResidentImages:
    """Decoded images of one mode packed into one device buffer (what ``DeviceResizer.upload`` returns)."""

    def __init__(self, buf, offsets, shapes, channels, nbytes):
        self.buf, self.offsets, self.shapes, self.channels, self.nbytes = buf, offsets, shapes, channels, nbytes


class ResizePlan:
    """Descriptors of one call, laid out: ``items`` (ctypes array), launch sizes, workspace and output bytes."""

    def __init__(self, items, n, channels, blocks, workspace_bytes, out_offsets, out_shapes, out_bytes):
        self.items, self.n, self.channels, self.blocks = items, n, channels, blocks
        self.workspace_bytes, self.out_offsets, self.out_shapes, self.out_bytes = workspace_bytes, out_offsets, out_shapes, out_bytes


class DeviceResizer:
    """Pillow's ``crop(box).resize(size, LANCZOS)`` of "L" / "RGB" images through the C ABI, a batch per call."""

    def __init__(self, lib=None, dev=None):
        if lib is None:
            from . import _lib

            lib = _lib.load_library()
        if dev is None:
            from .device import TorchDevice

            dev = TorchDevice()
        self.lib, self.dev = lib, dev
        self._table_at: dict[tuple[int, int], tuple[int, int]] = {}  # (in, out) -> (int32 offset in the arena, ksize)
        self._arena_host: list[np.ndarray] = [np.zeros(64, np.int32)]  # never empty: the call takes a non-null pointer
        self._arena_len = 64
        self._arena_dev = None  # uploaded again when a size pair was added; kept alive here between calls

    # ------------------------------------------------------------------ tables
    def _table(self, in_size: int, out_size: int) -> tuple[int, int]:
        key = (in_size, out_size)
        if key not in self._table_at:
            bounds, coeffs, ksize = lanczos_tables(in_size, out_size)
            self._table_at[key] = (self._arena_len, ksize)
            flat = np.concatenate([bounds.ravel(), coeffs.ravel()])
            self._arena_host.append(flat)
            self._arena_len += flat.size
            self._arena_dev = None
        return self._table_at[key]

    def _tables_dev(self):
        if self._arena_dev is None:
            self._arena_dev = self.dev.to_device(np.concatenate(self._arena_host))
        return self._arena_dev

    # ------------------------------------------------------------------ images
    def upload(self, images) -> ResidentImages:
        """Host uint8 arrays [h, w] (all) or [h, w, 3] (all) packed into one device buffer."""
        channels = _channels_of(images)
        offsets, total = [], 0
        for im in images:
            offsets.append(total)
            total += _align(im.size)
        packed = np.zeros(max(total, _ALIGN), dtype=np.uint8)
        for im, off in zip(images, offsets):
            packed[off: off + im.size] = np.ascontiguousarray(im).reshape(-1)
        return ResidentImages(self.dev.to_device(packed), offsets, [tuple(im.shape[:2]) for im in images], channels, packed.size)

    # ------------------------------------------------------------------ one call
    def plan(self, resident: ResidentImages, boxes, sizes, select=None, out_offsets=None) -> ResizePlan:
        """boxes: (x, y, w, h) per image; sizes: (out_w, out_h) per image, Pillow's order.  ``select``: the positions in
        ``resident`` this call resizes (default all; boxes and sizes are still per image of ``resident``).  ``out_offsets``:
        where each selected image's output starts in the output buffer, in bytes - the rows of a dense batch, say, which
        need no alignment (features.DeviceImages); default: one behind the other at 256-byte boundaries."""
        from ._lib import ImageResizeItem

        channels = resident.channels
        select = range(len(resident.shapes)) if select is None else list(select)
        n = len(select)
        items = (ImageResizeItem * max(n, 1))()
        dense, out_offsets, out_shapes, total = out_offsets, [], [], 0
        for i, k in enumerate(select):
            (h, w), off, (bx, by, bw, bh), (ow, oh) = resident.shapes[k], resident.offsets[k], boxes[k], sizes[k]
            if dense is not None:
                total = int(dense[i])
            if ow < 1 or oh < 1:
                raise ValueError("height and width must be > 0")  # Pillow's message for an empty target size
            it = items[i]
            it.in_off, it.in_h, it.in_w, it.in_stride = off, h, w, w * channels
            it.box_x, it.box_y, it.box_w, it.box_h = bx, by, bw, bh
            it.out_w, it.out_h, it.out_off = ow, oh, total
            it.htab, it.hk = self._table(bw, ow) if ow != bw else (-1, 0)
            it.vtab, it.vk = self._table(bh, oh) if oh != bh else (-1, 0)
            out_offsets.append(total)
            out_shapes.append((oh, ow) if channels == 1 else (oh, ow, channels))
            total += _align(ow * oh * channels)
        ws, blocks = C.c_size_t(0), (C.c_int32 * 2)()
        self.lib.check(self.lib.spr_image_resize_layout(C.cast(items, C.c_void_p), n, channels, C.byref(ws), blocks))
        return ResizePlan(items, n, channels, blocks, int(ws.value), out_offsets, out_shapes, total)

    def run(self, plan: ResizePlan, resident: ResidentImages, out=None, workspace=None):
        """Enqueue the call; ``out`` / ``workspace``: device byte buffers of plan.out_bytes / plan.workspace_bytes (made here
        if not given).  Returns the output buffer."""
        if out is None:
            out = self.dev.empty_bytes(max(plan.out_bytes, _ALIGN))
        if workspace is None:
            workspace = self.dev.empty_bytes(max(plan.workspace_bytes, _ALIGN))
        items_dev = self.dev.to_device(np.frombuffer(plan.items, dtype=np.uint8).copy())
        tables = self._tables_dev()
        self.lib.check(self.lib.spr_image_resize_u8(self.dev.ptr(resident.buf), self.dev.ptr(out), self.dev.ptr(items_dev),
                                                    plan.n, plan.channels, self.dev.ptr(tables), plan.blocks,
                                                    self.dev.ptr(workspace), self.dev.stream()))
        self._last = (items_dev, workspace)  # alive until the next call on this resizer
        return out

    def fetch(self, plan: ResizePlan, out) -> list[np.ndarray]:
        """The results as host arrays shaped like ``np.array(pillow_image)``."""
        host = self.dev.to_host(out)
        res = []
        for off, shape in zip(plan.out_offsets, plan.out_shapes):
            res.append(host[off: off + int(np.prod(shape))].reshape(shape))
        return res

    def resize_resident(self, resident: ResidentImages, boxes, sizes) -> list[np.ndarray]:
        if not resident.shapes:
            return []
        plan = self.plan(resident, boxes, sizes)
        return self.fetch(plan, self.run(plan, resident))

    def resize(self, images, boxes, sizes) -> list[np.ndarray]:
        """Upload, resize, download: ``np.array(Image.fromarray(im).crop(...).resize(size, LANCZOS))`` for every image."""
        if not images:
            return []
        return self.resize_resident(self.upload(images), boxes, sizes)


def _channels_of(images) -> int:
    kinds = {(im.ndim, im.shape[2] if im.ndim == 3 else 1, im.dtype == np.uint8) for im in images}
    if kinds == {(2, 1, True)}:
        return 1
    if kinds == {(3, 3, True)}:
        return 3
    raise ValueError("one call takes uint8 images that are all [h, w] or all [h, w, 3]")
