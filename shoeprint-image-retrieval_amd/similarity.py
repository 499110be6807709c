"""Query-vs-gallery NCC scoring and ranking on MI355X — host mirror of the reference scorer.

Drop-in for ``src/shoeprint_image_retrieval/similarity.py`` of the reference:

* ``compare_maps(shoemark_maps, shoeprint_maps, matching_pairs, config)``  (similarity.py:129-134)
* ``get_similarity(shoemark, shoeprint)``                                  (similarity.py:75-78)
* ``normxcorr(template, image, mode="same")``                              (similarity.py:26-31)

with the same argument meaning, return types and error behaviour, computed by the HIP
library behind the C ABI of ``include/shoeprint_mi355x.h`` (see ``_lib.py``).  The reference
forks ``n_processes`` CPU workers over query chunks (similarity.py:146-197); here every
(query, gallery) pair is a workgroup of one kernel launch, so ``n_processes`` is accepted
and ignored.  There is no CPU fallback: without the library or a GPU these functions raise.

``NccScorer`` is the device-level interface used by ``bench.py`` and the multi-GPU driver:
it keeps features, prepared spectra and the score matrix resident in HBM.

``retrieve`` is what casework asks for and the reference cannot give (it ranks a KNOWN true match only): per query the
k best gallery items, and for each where the mark sits on the print and under which rotation / scale variant.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, NamedTuple, Sequence

import numpy as np

from . import _lib
from ._lib import NCC_AUTO, NCC_DIRECT, NCC_FFT, NccShape

CROP = 2  # similarity.py:92-93
_METHODS = {"auto": NCC_AUTO, "fft": NCC_FFT, "direct": NCC_DIRECT, "fft_pow2": _lib.NCC_FFT_POW2, "mfma": _lib.NCC_MFMA,
            "mfma_f32": _lib.NCC_MFMA_F32}
_DTYPES = {np.dtype(np.float32): _lib.F32, np.dtype(np.float16): _lib.F16}


def _dtype_code(dtype) -> tuple[int, str]:
    """(spr_dtype, cache key) of a feature storage type: numpy float32 / float16, or bfloat16 given as the
    string "bfloat16", a torch.bfloat16, or uint16 bit patterns (numpy has no bfloat16)."""
    name = str(dtype).replace("torch.", "")
    if name in ("bfloat16", "bf16", "uint16", "<class 'numpy.uint16'>"):
        return _lib.BF16, "bf16"
    d = np.dtype(name if name in ("float32", "float16") else dtype)
    return _DTYPES[d], d.str


class _Plan:
    """Owns one spr_ncc_plan (one (query shape, gallery shape) class)."""

    def __init__(self, lib: _lib.Library, channels: int, q_hw, g_hw, crop: int, dtype: int, method: int,
                 enable_peaks: bool = False):
        self.lib = lib
        shape = NccShape(channels, q_hw[0], q_hw[1], g_hw[0], g_hw[1], crop, dtype, method)
        handle = C.c_void_p()
        lib.check(lib.spr_ncc_plan_create(C.byref(shape), C.byref(handle)))
        self.handle = handle
        if enable_peaks:  # a matrix-core plan's peak form is opt-in; a no-op on the others
            lib.check(lib.spr_ncc_plan_enable_peaks(handle))
        self.channels, self.q_hw, self.g_hw, self.crop = channels, tuple(q_hw), tuple(g_hw), crop
        self.method = lib.spr_ncc_plan_method(handle)
        rows, cols = C.c_int32(), C.c_int32()
        lib.check(lib.spr_ncc_plan_fft_size(handle, C.byref(rows), C.byref(cols)))
        self.fft_size = (rows.value, cols.value)
        self.query_item_bytes = lib.spr_ncc_query_bytes(handle, 1)
        self.gallery_item_bytes = lib.spr_ncc_gallery_bytes(handle, 1)
        # spr_ncc_score_peaks: FFT and direct plans, and matrix-core plans that were asked (enable_peaks)
        self.has_peaks = bool(lib.spr_ncc_plan_has_peaks(handle))
        # spr_ncc_score_list: FFT plans whose working set lies in LDS, and direct plans
        self.has_list = bool(lib.spr_ncc_plan_has_list(handle))
        # spr_ncc_score_surfaces: exactly the plans that have the list form
        self.has_surfaces = bool(lib.spr_ncc_plan_has_surfaces(handle))

    def close(self):
        if self.handle:
            self.lib.spr_ncc_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


def _as_item_list(maps) -> tuple[list | None, Any]:
    """Normalise the accepted inputs: returns (list of per-item arrays, None) for host lists /
    host arrays, or (None, device_array) for an already device-resident [N,C,h,w] batch."""
    if isinstance(maps, np.ndarray):
        if maps.ndim != 4:
            raise ValueError("a feature batch must be [N, C, h, w]")
        return list(maps), None
    if isinstance(maps, (list, tuple)):
        return list(maps), None
    return None, maps


def _host_items(dev, maps) -> list:
    """List of per-item host arrays of any accepted input (a device batch is copied to the host)."""
    items, batch = _as_item_list(maps)
    return list(dev.to_host(batch)) if items is None else items


class _HostSide:
    """A host item list behind the interface ``_blocks`` walks (``features.FeatureSet`` is the resident one)."""

    def __init__(self, dev, items):
        self.dev, self.items = dev, items

    def __len__(self) -> int:
        return len(self.items)

    def groups(self, used=None) -> dict[tuple, list[int]]:
        return _group_by_shape(self.items, used)

    def stack(self, lib, idx, storage: str | None = None):
        buf = self.dev.stack_to_device([self.items[i] for i in idx])
        return buf if storage is None else self.dev.astype_storage(buf, storage)


def _is_resident(maps) -> bool:
    from .features import FeatureSet

    return isinstance(maps, FeatureSet)


def _side(dev, maps):
    """Any accepted input as a side of the walk: a FeatureSet as it is (nothing is copied), everything else as a host list."""
    return maps if _is_resident(maps) or isinstance(maps, _HostSide) else _HostSide(dev, _host_items(dev, maps))


class NccScorer:
    """Scores queries against a gallery with the HIP NCC kernels; everything stays in HBM.

    Parameters
    ----------
    device : backend object (default ``TorchDevice()``: PyTorch-ROCm on the current GPU)
    library: ``_lib.Library`` (default: the in-tree libshoeprint_mi355x.so)
    method : "auto" | "fft" | "direct" | "fft_pow2" | "mfma" | "mfma_f32"  (pair-kernel choice, see the C header)
    max_prepared_bytes: HBM budget for the prepared form of one gallery chunk (default: a third
        of the free memory, at most 64 GiB); larger galleries are processed chunk by chunk.
    storage: HBM storage type of feature batches uploaded from host lists ("float32" | "float16" | "bfloat16");
        arithmetic is float32 / float64 whatever the storage.
    f32_matrix_cores: with method "auto", a float32 plan first asks for "mfma_f32" (float32 maps as hi + lo on the bf16
        matrix cores: cropped maps up to 28 x 12, cropped templates up to 30 x 16) and takes what "auto" gives where that
        method does not cover the plan - per plan, so ragged sets and query variants mix methods by shape.
    matrix_core_peaks: every plan is asked for the peak form (spr_ncc_plan_enable_peaks), so plans of the matrix-core
        methods ("mfma", "mfma_f32", and what "auto" resolves to them) too give position and best variant out of the
        scoring pass: ``score_matrix_located`` and ``retrieve`` then make no second pass over their blocks.  Off by
        default: such plans keep the maximum only, as before the form existed.
    """

    def __init__(self, device=None, library: _lib.Library | None = None, method: str = "auto",
                 max_prepared_bytes: int | None = None, crop: int = CROP, storage: str = "float32",
                 f32_matrix_cores: bool = False, matrix_core_peaks: bool = False):
        self.lib = library or _lib.load_library()
        if device is None:
            from .device import TorchDevice

            device = TorchDevice()
        self.dev = device
        self.method = _METHODS[method]
        self.crop = crop
        self.max_prepared_bytes = max_prepared_bytes
        if storage not in ("float32", "float16", "bfloat16"):
            raise ValueError(f"unknown storage type {storage!r}")
        self.storage = storage
        self.f32_matrix_cores = bool(f32_matrix_cores)
        self.matrix_core_peaks = bool(matrix_core_peaks)
        self._plans: dict[tuple, _Plan] = {}
        self._variants = None

    # ------------------------------------------------------------------ plans
    def plan(self, channels: int, q_hw, g_hw, dtype=np.float32, crop: int | None = None) -> _Plan:
        crop = self.crop if crop is None else crop
        code, dkey = _dtype_code(dtype)
        key = (channels, tuple(q_hw), tuple(g_hw), dkey, crop, self.method)
        p = self._plans.get(key)
        if p is None:
            if self.f32_matrix_cores and self.method == NCC_AUTO and code == _lib.F32:
                try:
                    p = _Plan(self.lib, channels, q_hw, g_hw, crop, code, _lib.NCC_MFMA_F32, self.matrix_core_peaks)
                except _lib.SprError as e:
                    if e.code != _lib.SPR_ERR_UNSUPPORTED:
                        raise
            if p is None:
                p = _Plan(self.lib, channels, q_hw, g_hw, crop, code, self.method, self.matrix_core_peaks)
            self._plans[key] = p
        return p

    def close(self):
        for p in self._plans.values():
            p.close()
        self._plans.clear()

    # ------------------------------------------------------------------ device-level steps
    def _budget(self) -> int:
        if self.max_prepared_bytes is not None:
            return int(self.max_prepared_bytes)
        return max(256 << 20, min(self.dev.free_bytes() // 3, 64 << 30))

    def prepare_queries(self, plan: _Plan, q_dev):
        n = self.dev.shape(q_dev)[0]
        out = self.dev.empty_bytes(max(1, plan.query_item_bytes * n))
        self.lib.check(self.lib.spr_ncc_prepare_queries(plan.handle, self.dev.ptr(q_dev), n, self.dev.ptr(out),
                                                        self.dev.stream()))
        return out

    def prepare_gallery(self, plan: _Plan, g_dev, out=None):
        n = self.dev.shape(g_dev)[0]
        if out is None:
            out = self.dev.empty_bytes(max(1, plan.gallery_item_bytes * n))
        self.lib.check(self.lib.spr_ncc_prepare_gallery(plan.handle, self.dev.ptr(g_dev), n, self.dev.ptr(out),
                                                        self.dev.stream()))
        return out

    def score_prepared(self, plan: _Plan, pq, nq: int, pg, ng: int, scores, ld: int, col0: int,
                       accumulate_max: bool = False, peaks=None, tags=None, tag: int = 0):
        """spr_ncc_score; with ``peaks`` (device int32, laid out like ``scores``) spr_ncc_score_peaks: the same scores and
        beside each the position ``(y << 16) | x`` of its maximum, in ``tags`` (optional, same layout) the ``tag`` of the
        call that stored it.  Plans of the matrix-core methods have no peak form unless the scorer was made with
        ``matrix_core_peaks`` (``plan.has_peaks``): SprError."""
        if peaks is None:
            self.lib.check(self.lib.spr_ncc_score(plan.handle, self.dev.ptr(pq), nq, self.dev.ptr(pg), ng,
                                                  self.dev.ptr(scores), ld, col0, 1 if accumulate_max else 0,
                                                  self.dev.stream()))
            return
        self.lib.check(self.lib.spr_ncc_score_peaks(plan.handle, self.dev.ptr(pq), nq, self.dev.ptr(pg), ng,
                                                    self.dev.ptr(scores), self.dev.ptr(peaks),
                                                    None if tags is None else self.dev.ptr(tags), ld, col0,
                                                    1 if accumulate_max else 0, int(tag), self.dev.stream()))

    def score_list_prepared(self, plan: _Plan, pq, nq: int, pg, ng: int, pairs, n_pairs: int, scores, peaks, tags=None,
                            accumulate_max: bool = False, tag: int = 0):
        """spr_ncc_score_list: ``score_prepared`` with ``peaks`` for the ``n_pairs`` entries of ``pairs`` (device int32
        [n_pairs, 2]: position in ``pq``, position in ``pg``) instead of the whole grid; ``scores`` / ``peaks`` / ``tags``
        (optional) are device vectors of one entry per pair.  An entry that names no item is skipped.  Plans without the
        form (``plan.has_list``: the workspace instance, the matrix-core methods): SprError."""
        self.lib.check(self.lib.spr_ncc_score_list(plan.handle, self.dev.ptr(pq), nq, self.dev.ptr(pg), ng,
                                                   self.dev.ptr(pairs), n_pairs, self.dev.ptr(scores), self.dev.ptr(peaks),
                                                   None if tags is None else self.dev.ptr(tags),
                                                   1 if accumulate_max else 0, int(tag), self.dev.stream()))

    def surfaces_prepared(self, plan: _Plan, pq, nq: int, pg, ng: int, pairs, n_pairs: int, scores, peaks, surfaces,
                          tags=None, accumulate_max: bool = False, tag: int = 0):
        """spr_ncc_score_surfaces: ``score_list_prepared`` that also stores every entry's channel-mean NCC map into
        ``surfaces`` (device float32 [n_pairs, ih, iw], the cropped gallery map's size) wherever it writes the entry's
        (score, peak, tag).  Plans without the form (``plan.has_surfaces``): SprError."""
        self.lib.check(self.lib.spr_ncc_score_surfaces(plan.handle, self.dev.ptr(pq), nq, self.dev.ptr(pg), ng,
                                                       self.dev.ptr(pairs), n_pairs, self.dev.ptr(scores), self.dev.ptr(peaks),
                                                       None if tags is None else self.dev.ptr(tags), self.dev.ptr(surfaces),
                                                       1 if accumulate_max else 0, int(tag), self.dev.stream()))

    def surface_peaks_device(self, surfaces, n_peaks: int = 2, ry: int = 0, rx: int = 0):
        """spr_surface_peaks of the device float32 [n, h, w] ``surfaces``: device (values float32 [n, n_peaks], packed
        positions int32 [n, n_peaks] - ``(y << 16) | x``, -1 = no pixel left -, psr float32 [n]).  Peak j is the maximum
        outside the windows ``|y - y_i| <= ry and |x - x_i| <= rx`` of the peaks before it; psr is the peak-to-sidelobe
        ratio of peak 0 over the pixels outside its window."""
        n, h, w = self.dev.shape(surfaces)
        n_peaks = int(n_peaks)
        _require_contiguous(surfaces, "surfaces")
        if n > 0 and self._torch_ops() is not None:
            return self._torch_ops().surface_peaks(surfaces, n_peaks, int(ry), int(rx))
        values = self.dev.empty((max(n, 1), max(n_peaks, 1)), np.float32)
        yx = self.dev.empty((max(n, 1), max(n_peaks, 1)), np.int32)
        psr = self.dev.empty((max(n, 1),), np.float32)
        self.lib.check(self.lib.spr_surface_peaks(self.dev.ptr(surfaces), n, h, w, n_peaks, int(ry), int(rx),
                                                  self.dev.ptr(values), self.dev.ptr(yx), self.dev.ptr(psr), self.dev.stream()))
        return self.dev.narrow0(values, 0, n), self.dev.narrow0(yx, 0, n), self.dev.narrow0(psr, 0, n)

    def mean_maps_device(self, plan: _Plan, pq, pg, slots, max_bytes: int = 256 << 20) -> np.ndarray:
        """Host float32 [P, ih, iw] channel-mean NCC maps of the pairs ``slots`` of one plan - the route of plans without a
        surfaces form: spr_ncc_maps of every pair as in ``peaks_device``, then ONE spr_maps_mean launch per chunk.  The
        maximum of a map has the bits of ``peaks_device``'s score."""
        ih, iw = plan.g_hw[0] - 2 * plan.crop, plan.g_hw[1] - 2 * plan.crop
        per = plan.channels * ih * iw * 4
        out = np.zeros((len(slots), ih, iw), np.float32)
        step = max(1, min(len(slots), max_bytes // per))
        for s0 in range(0, len(slots), step):
            part = slots[s0:s0 + step]
            maps = self.dev.zeros((len(part), plan.channels, ih, iw), np.float32)  # (channels dead on either side stay 0)
            for k, (qp, gp) in enumerate(part):
                self.lib.check(self.lib.spr_ncc_maps(plan.handle, self.dev.ptr(pq) + qp * plan.query_item_bytes,
                                                     self.dev.ptr(pg) + gp * plan.gallery_item_bytes,
                                                     self.dev.ptr(maps) + k * per, self.dev.stream()))
            mean = self.dev.empty((len(part), ih, iw), np.float32)
            self.lib.check(self.lib.spr_maps_mean(self.dev.ptr(maps), len(part), plan.channels, ih, iw, self.dev.ptr(mean),
                                                  self.dev.stream()))
            out[s0:s0 + len(part)] = self.dev.to_host(mean)
        return out

    def gallery_chunk_items(self, plan: _Plan, n_gallery: int, share: int = 1) -> int:
        """Gallery items per prepared chunk; ``share`` = how many prepared forms of the chunk are alive at once (one per
        distinct query-variant shape: the 1/sigma map depends on the template size) and split the budget."""
        per_item = plan.gallery_item_bytes
        return int(max(1, min(n_gallery, self._budget() // max(1, share) // max(1, per_item), 65535)))

    def scores_device(self, q_dev, g_dev, scores=None, accumulate_max: bool = False, plan: _Plan | None = None):
        """[Q,G] float32 score matrix (device) of a uniform query batch [Q,C,h,w] against a uniform
        gallery batch [G,C,h',w'], both already in HBM.  One step of the hot path.  The storage type is
        taken from the buffers: float32, float16, or bfloat16 (torch.bfloat16 or uint16 bit patterns); the
        arithmetic is float32 / float64 as ever."""
        nq, c, qh, qw = self.dev.shape(q_dev)
        ng, c2, gh, gw = self.dev.shape(g_dev)
        if c != c2:
            raise ValueError(f"channel mismatch: queries {c}, gallery {c2}")
        if plan is None and str(q_dev.dtype) != str(g_dev.dtype):
            raise ValueError(f"storage type mismatch: queries {q_dev.dtype}, gallery {g_dev.dtype}")
        if plan is None and scores is None and not accumulate_max and self._torch_ops() is not None:
            # north_star's named mechanism: the registered PyTorch-ROCm custom op (csrc/torch_ops.cpp), same entry points
            method = self.method
            if self.f32_matrix_cores:  # the op resolves a method name by itself: hand it the one this scorer's plan took
                if self.plan(c, (qh, qw), (gh, gw), dtype=q_dev.dtype).method == _lib.NCC_MFMA_F32:
                    method = _lib.NCC_MFMA_F32
            return self._torch_ops().ncc_scores(q_dev, g_dev, self.crop, _lib.METHOD_NAMES[method], self._budget())
        if plan is None:
            plan = self.plan(c, (qh, qw), (gh, gw), dtype=q_dev.dtype)
        if scores is None:
            scores = self.dev.zeros((nq, ng), np.float32)
        if nq == 0 or ng == 0:
            return scores
        pq = self.prepare_queries(plan, q_dev)
        chunk = self.gallery_chunk_items(plan, ng)
        pg = self.dev.empty_bytes(plan.gallery_item_bytes * chunk)
        for start in range(0, ng, chunk):
            n = min(chunk, ng - start)
            self.prepare_gallery(plan, self.dev.narrow0(g_dev, start, n), out=pg)
            for q0 in range(0, nq, 65535):
                qn = min(65535, nq - q0)
                self.score_prepared(plan, self._offset(pq, q0 * plan.query_item_bytes), qn, pg, n,
                                    self.dev.narrow0(scores, q0, qn), ng, start, accumulate_max)
        return scores

    def _offset(self, byte_buf, nbytes: int):
        return byte_buf if nbytes == 0 else self.dev.narrow0(byte_buf, nbytes, self.dev.shape(byte_buf)[0] - nbytes)

    def _torch_ops(self):
        """torch.ops.shoeprint_mi355x when this scorer runs the in-tree library on PyTorch-ROCm tensors and the op library
        is built (and not switched off with SPR_TORCH_OPS=0); None otherwise (emulation tests, explicit libraries)."""
        if getattr(self, "_ops_cache", False) is False:
            from . import _torch_ops

            ok = (self.dev.name == "hip" and self.lib is _lib.load_library() and _torch_ops.enabled())
            self._ops_cache = _torch_ops.load() if ok else None
        return self._ops_cache

    def ranks_device(self, scores, match_dev):
        nq, ng = self.dev.shape(scores)
        if nq > 0 and self._torch_ops() is not None and scores.is_contiguous() and match_dev.is_contiguous():
            return self._torch_ops().ranks(scores, match_dev)
        _require_contiguous(scores, "scores")
        _require_contiguous(match_dev, "match")
        ranks = self.dev.zeros((max(nq, 1),), np.int32)
        self.lib.check(self.lib.spr_rank_true_match(self.dev.ptr(scores), ng, nq, ng, self.dev.ptr(match_dev),
                                                    self.dev.ptr(ranks), self.dev.stream()))
        return self.dev.narrow0(ranks, 0, nq)

    def ncc_maps_device(self, plan: _Plan, pq, pg):
        ih, iw = plan.g_hw[0] - 2 * plan.crop, plan.g_hw[1] - 2 * plan.crop
        out = self.dev.zeros((plan.channels, ih, iw), np.float32)
        self.lib.check(self.lib.spr_ncc_maps(plan.handle, self.dev.ptr(pq), self.dev.ptr(pg), self.dev.ptr(out),
                                             self.dev.stream()))
        return out

    def topk_device(self, scores, k: int, global_col0: int = 0, col_index=None):
        """(scores [Q,k] float32, index [Q,k] int32), both on the device: the k best items of every row of the device
        matrix ``scores`` [Q,G] in the ranker's order (position p holds the item ``ranks_device`` ranks p + 1; ties: the
        larger index first).  The index of column j is ``global_col0 + j`` (a shard: the global index of its first column)
        or, with ``col_index`` (device int32 [Q,G], -1 = empty), ``col_index[q, j]`` - the form that merges candidate
        lists gathered from shards.  Slots beyond the number of items hold score 0 and index -1.  1 <= k <= 256."""
        nq, ng = self.dev.shape(scores)
        k = int(k)
        _require_contiguous(scores, "scores")  # (the kernels take a dense [Q, G] matrix: a strided view would be misread)
        if col_index is None and global_col0 == 0 and nq > 0 and self._torch_ops() is not None:
            return self._torch_ops().topk(scores, k)
        if col_index is not None:
            _require_contiguous(col_index, "col_index")
            if tuple(self.dev.shape(col_index)) != (nq, ng):
                raise ValueError(f"col_index is {self.dev.shape(col_index)}, the scores are {(nq, ng)}")
        out_s = self.dev.empty((max(nq, 1), max(k, 0)), np.float32)
        out_i = self.dev.empty((max(nq, 1), max(k, 0)), np.int32)
        self.lib.check(self.lib.spr_topk_rows(self.dev.ptr(scores), ng, nq, ng,
                                              None if col_index is None else self.dev.ptr(col_index), int(global_col0), k,
                                              self.dev.ptr(out_s), self.dev.ptr(out_i), self.dev.stream()))
        return self.dev.narrow0(out_s, 0, nq), self.dev.narrow0(out_i, 0, nq)

    def peaks_device(self, plan: _Plan, pq, pg, slots, max_bytes: int = 256 << 20):
        """Host (score float32 [P], yx int32 [P,2]) of the pairs ``slots`` = [(query position in ``pq``, gallery position
        in ``pg``), ...] of one plan: spr_ncc_maps of every pair into a slice of a [P_chunk, C, ih, iw] buffer (at most
        ``max_bytes``), then ONE spr_maps_peak launch per chunk."""
        ih, iw = plan.g_hw[0] - 2 * plan.crop, plan.g_hw[1] - 2 * plan.crop
        per = plan.channels * ih * iw * 4
        score = np.zeros(len(slots), np.float32)
        yx = np.zeros((len(slots), 2), np.int32)
        step = max(1, min(len(slots), max_bytes // per))
        for s0 in range(0, len(slots), step):
            part = slots[s0:s0 + step]
            maps = self.dev.zeros((len(part), plan.channels, ih, iw), np.float32)  # (channels dead on either side stay 0)
            for k, (qp, gp) in enumerate(part):
                self.lib.check(self.lib.spr_ncc_maps(plan.handle, self.dev.ptr(pq) + qp * plan.query_item_bytes,
                                                     self.dev.ptr(pg) + gp * plan.gallery_item_bytes,
                                                     self.dev.ptr(maps) + k * per, self.dev.stream()))
            out_s = self.dev.empty((len(part),), np.float32)
            out_yx = self.dev.empty((len(part), 2), np.int32)
            self.lib.check(self.lib.spr_maps_peak(self.dev.ptr(maps), len(part), plan.channels, ih, iw, self.dev.ptr(out_s),
                                                  self.dev.ptr(out_yx), self.dev.stream()))
            score[s0:s0 + len(part)] = self.dev.to_host(out_s)
            yx[s0:s0 + len(part)] = self.dev.to_host(out_yx)
        return score, yx

    # ------------------------------------------------------------------ list-of-arrays level
    def _blocks(self, q_items, g_items, rotations, scales, q_used=None, g_used=None):
        """THE walk over ragged item sets (``_side``: host lists or resident ``FeatureSet``s, either per side), behind
        ``score_matrix``, ``score_matrix_located`` and ``locate``: grouping by
        shape, variant lists, plans, chunk budget and gallery preparation are decided here and nowhere else.  Of the items
        ``q_used`` / ``g_used`` (ascending indices; default all) every query shape class is stacked, uploaded, expanded by
        ``VariantBuilder.variants`` and cast to the storage type once; every gallery shape class gets one plan per distinct
        variant shape (the 1/sigma map depends on the template size) and goes chunk by chunk, the prepared forms of a chunk -
        one per plan, all alive while the query classes are walked - sharing the budget.  Yields per (gallery chunk, query
        class) a ``_Block``; its ``prepared(vs)`` uploads the chunk on first need and prepares it once per variant shape, so a
        block the consumer passes over costs nothing.  A block is good until the walk is advanced.  A resident side is never
        copied to the host: its stacks are spr_items_gather calls (``FeatureSet.stack``), the cast to the storage type fused
        into the gallery chunks' and, without variants, the query classes'."""
        from .variants import VariantBuilder

        if self._variants is None:
            self._variants = VariantBuilder(self.lib, self.dev)  # (keeps its resample tables on the device)
        q_side = []
        plain = rotations is None and scales is None
        for qshape, q_idx in q_items.groups(q_used).items():
            if plain and _is_resident(q_items):  # no float32 intermediate to expand: gathered and cast in one pass
                q_side.append((qshape, q_idx, [(0, tuple(qshape[1:]), q_items.stack(self.lib, q_idx, self.storage))]))
                continue
            batches = self._variants.variants(q_items.stack(self.lib, q_idx), rotations, scales)
            q_side.append((qshape, q_idx, [(number, tuple(self.dev.shape(v)[2:]), self.dev.astype_storage(v, self.storage))
                                           for number, v in enumerate(batches)]))
        for gshape, g_idx in g_items.groups(g_used).items():
            plans = {}
            for qshape, _, variants in q_side:
                if qshape[0] != gshape[0]:
                    raise ValueError(f"channel mismatch: query {qshape}, gallery {gshape}")
                for _, vs, _ in variants:
                    plans[vs] = self.plan(qshape[0], vs, gshape[1:], dtype=self.storage)
            chunk = min(self.gallery_chunk_items(p, len(g_idx), share=len(plans)) for p in plans.values())
            for start in range(0, len(g_idx), chunk):
                idx = g_idx[start:start + chunk]
                alive = {}  # None -> the uploaded chunk, variant shape -> its prepared form

                def prepared(vs):
                    if vs not in alive:
                        if None not in alive:
                            alive[None] = g_items.stack(self.lib, idx, self.storage)
                        alive[vs] = self.prepare_gallery(plans[vs], alive[None])
                    return alive[vs]

                for _, q_idx, variants in q_side:
                    yield _Block(q_idx, variants, idx, plans, chunk, prepared)

    def locate(self, shoemark_maps, shoeprint_maps, pairs, rotations=None, scales=None):
        """Where and under which variant every pair of ``pairs`` = [(query index, gallery index), ...] matches best:
        host arrays (score float32 [P], variant int32 [P], yx int32 [P,2]).  Per pair and per variant list - numbered in
        the order of ``VariantBuilder.variants``, 0 = the query as it is - the channel-summed NCC map is reduced to its
        peak (first maximum in row-major order, cropped search-map coordinates); the variant with the largest peak wins,
        the lowest number among equal peaks.  ``score`` is that peak over the channel count: get_similarity's value,
        NOT floored at 0.  A second pass beside the pair kernels, which keep only the maximum: ``score_matrix``'s walk
        (``_blocks``) over the items the pairs name, so the union of those gallery items is uploaded once and prepared once
        per plan, and blocks that hold no pair are passed over."""
        return self._locate(shoemark_maps, shoeprint_maps, pairs, rotations, scales)[:3]

    def _locate(self, shoemark_maps, shoeprint_maps, pairs, rotations, scales):
        """``locate`` plus the cropped size (th, tw) int32 [P,2] of every pair's winning variant template, read off the
        variant batches themselves."""
        q_items, g_items = _side(self.dev, shoemark_maps), _side(self.dev, shoeprint_maps)
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = len(pairs)
        best = np.full(n, -np.inf, dtype=np.float32)
        variant = np.zeros(n, dtype=np.int32)
        yx = np.zeros((n, 2), dtype=np.int32)
        t_hw = np.zeros((n, 2), dtype=np.int32)
        if n == 0:
            return best, variant, yx, t_hw
        if pairs.min() < 0 or pairs[:, 0].max() >= len(q_items) or pairs[:, 1].max() >= len(g_items):
            raise IndexError("a pair names an item outside the query or gallery set")
        q_used, g_used = (sorted({int(i) for i in pairs[:, side]}) for side in (0, 1))
        for b in self._blocks(q_items, g_items, rotations, scales, q_used, g_used):
            q_pos = {q: i for i, q in enumerate(b.q_idx)}
            g_pos = {g: i for i, g in enumerate(b.g_idx)}
            sel = [i for i in range(n) if int(pairs[i, 0]) in q_pos and int(pairs[i, 1]) in g_pos]
            if not sel:
                continue
            slots = [(q_pos[int(pairs[i, 0])], g_pos[int(pairs[i, 1])]) for i in sel]
            for number, vs, v in b.variants:
                plan = b.plans[vs]
                pg = b.prepared(vs)
                score, pos = self.peaks_device(plan, self.prepare_queries(plan, v), pg, slots)
                better = score > best[sel]  # strictly: the lowest variant number keeps an equal peak
                rows = np.asarray(sel)[better]
                best[rows], variant[rows], yx[rows] = score[better], number, pos[better]
                t_hw[rows] = (vs[0] - 2 * self.crop, vs[1] - 2 * self.crop)
        return best, variant, yx, t_hw

    def score_pairs(self, shoemark_maps, shoeprint_maps, pairs, rotations=None, scales=None):
        """``score_matrix_located`` read at ``pairs`` = [(query index, gallery index), ...], bit for bit, without the matrix:
        host ``(scores float32 [P], variant int32 [P], yx int32 [P,2], t_hw int32 [P,2])`` - the score floored at 0 and
        maximised over the variant lists, the lowest variant number among equal scores, its peak and the cropped size of
        its template; (0, -1, (-1, -1), (0, 0)) where no variant rises above 0.  The third consumer of ``_blocks``: only the
        shape classes and gallery chunks that hold a listed pair are stacked, prepared and visited.  Per block the pairs go
        up once as a device list sorted by gallery position (neighbouring workgroups then share a gallery item's lines)
        and every variant is one spr_ncc_score_list call.  A block one of whose plans has no list form (``plan.has_list``)
        is scored densely, as ``_walk_device`` scores it, and its listed cells are gathered (``cells_device``); where it has
        no peak form either, variant and position come from the second pass of ``locate``, as in ``_fill_unfused``."""
        return self._score_pairs(shoemark_maps, shoeprint_maps, pairs, rotations, scales, None)

    def pair_surfaces(self, shoemark_maps, shoeprint_maps, pairs, rotations=None, scales=None):
        """``score_pairs`` with every pair's correlation surface: ``(score, variant, peak_yx, t_hw, surfaces)``, the first
        four bit for bit ``score_pairs``', ``surfaces`` a list of host float32 [ih, iw] arrays, one per pair (prints are
        ragged) - the channel-mean NCC map of the winning variant over the cropped gallery map, the map ``peak_yx`` is the
        arg-max of; all zeros where no variant rises above 0 (variant -1).  The same walk, variant order and tags as
        ``score_pairs``, one spr_ncc_score_surfaces call per variant through accumulate_max: the device buffer ends with the
        winning variant's map.  A block one of whose plans lacks the form (``plan.has_surfaces``: the matrix-core methods,
        the workspace instance) takes its triple as ``score_pairs`` does; its maps are spr_ncc_maps of the winning variant
        folded by spr_maps_mean (float64 channel sums: the maximum has the bits of ``locate``'s score)."""
        surfaces: list = [None] * len(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        return (*self._score_pairs(shoemark_maps, shoeprint_maps, pairs, rotations, scales, surfaces), surfaces)

    def _score_pairs(self, shoemark_maps, shoeprint_maps, pairs, rotations, scales, surfaces):
        """``score_pairs``; with ``surfaces`` (a list of one slot per pair) also ``pair_surfaces``' maps, written into it."""
        dev = self.dev
        q_items, g_items = _side(dev, shoemark_maps), _side(dev, shoeprint_maps)
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = len(pairs)
        scores = np.zeros(n, dtype=np.float32)
        variant = np.full(n, -1, dtype=np.int32)
        yx = np.full((n, 2), -1, dtype=np.int32)
        t_hw = np.zeros((n, 2), dtype=np.int32)
        if n == 0:
            return scores, variant, yx, t_hw
        if pairs.min() < 0 or pairs[:, 0].max() >= len(q_items) or pairs[:, 1].max() >= len(g_items):
            raise IndexError("a pair names an item outside the query or gallery set")
        q_used, g_used = (sorted({int(i) for i in pairs[:, side]}) for side in (0, 1))
        unlocated = []  # entries of blocks without a peak form
        unmapped = []   # ``surfaces``: entries of blocks without a surfaces form
        for b in self._blocks(q_items, g_items, rotations, scales, q_used, g_used):
            q_pos = np.full(len(q_items), -1, dtype=np.int64)
            g_pos = np.full(len(g_items), -1, dtype=np.int64)
            q_pos[b.q_idx] = np.arange(len(b.q_idx))
            g_pos[b.g_idx] = np.arange(len(b.g_idx))
            sel = np.flatnonzero((q_pos[pairs[:, 0]] >= 0) & (g_pos[pairs[:, 1]] >= 0))
            if len(sel) == 0:
                continue
            self.last_chunk_items = b.chunk_items  # (read by the tests)
            qs, gs = q_pos[pairs[sel, 0]], g_pos[pairs[sel, 1]]
            order = np.argsort(gs, kind="stable")
            sel, qs, gs = sel[order], qs[order], gs[order]
            sizes = {number: (vs[0] - 2 * self.crop, vs[1] - 2 * self.crop) for number, vs, _ in b.variants}
            nq_b, ng_b = len(b.q_idx), len(b.g_idx)
            if all(b.plans[vs].has_list for _, vs, _ in b.variants):
                listed = dev.to_device(np.ascontiguousarray(np.stack([qs, gs], axis=1), dtype=np.int32))
                sub = dev.zeros((len(sel),), np.float32)
                sub_yx = dev.to_device(np.full(len(sel), -1, dtype=np.int32))
                sub_tag = dev.to_device(np.full(len(sel), -1, dtype=np.int32))
                maps = None
                if surfaces is not None:  # (one map shape per block: the gallery class's; entries no variant wins stay 0)
                    g_hw = b.plans[b.variants[0][1]].g_hw
                    maps = dev.zeros((len(sel), g_hw[0] - 2 * self.crop, g_hw[1] - 2 * self.crop), np.float32)
                for number, vs, v in b.variants:
                    plan = b.plans[vs]
                    pg = b.prepared(vs)
                    if maps is None:
                        self.score_list_prepared(plan, self.prepare_queries(plan, v), nq_b, pg, ng_b, listed, len(sel), sub,
                                                 sub_yx, sub_tag, accumulate_max=True, tag=number)
                    else:
                        self.surfaces_prepared(plan, self.prepare_queries(plan, v), nq_b, pg, ng_b, listed, len(sel), sub,
                                               sub_yx, maps, sub_tag, accumulate_max=True, tag=number)
                got = (dev.to_host(sub), dev.to_host(sub_tag), dev.to_host(sub_yx))
                if maps is not None:
                    for i, m in zip(sel, np.array(dev.to_host(maps))):
                        surfaces[i] = m
            else:  # the dense route of _walk_device for this block alone, read at the listed cells
                fused = all(b.plans[vs].has_peaks for _, vs, _ in b.variants)
                sub = dev.zeros((nq_b, ng_b), np.float32)
                sub_yx = dev.to_device(np.full((nq_b, ng_b), -1, dtype=np.int32)) if fused else None
                sub_tag = dev.to_device(np.full((nq_b, ng_b), -1, dtype=np.int32)) if fused else None
                for number, vs, v in b.variants:
                    plan = b.plans[vs]
                    pg = b.prepared(vs)
                    self.score_prepared(plan, self.prepare_queries(plan, v), nq_b, pg, ng_b, sub, ng_b, 0, accumulate_max=True,
                                        peaks=sub_yx, tags=sub_tag, tag=number)
                got = (self.cells_device(sub, ng_b, qs, gs).view(np.float32),
                       self.cells_device(sub_tag, ng_b, qs, gs) if fused else np.full(len(sel), -1, dtype=np.int32),
                       self.cells_device(sub_yx, ng_b, qs, gs) if fused else np.full(len(sel), -1, dtype=np.int32))
                if not fused:
                    unlocated.append(sel)
                if surfaces is not None:
                    unmapped.append(sel)
            scores[sel], variant[sel], yx[sel] = got[0], got[1], _unpack_yx(got[2])
            hit = got[1] >= 0
            t_hw[sel[hit]] = np.array([sizes[int(number)] for number in got[1][hit]], dtype=np.int32).reshape(-1, 2)
        if unlocated:
            rest = np.concatenate(unlocated)
            rest = rest[scores[rest] > 0]  # (as the fused form: no position where the floored score is 0)
            if len(rest):
                _, variant[rest], yx[rest], t_hw[rest] = self._locate(q_items, g_items, pairs[rest], rotations, scales)
        if unmapped:
            self._fill_unmapped(q_items, g_items, pairs, np.concatenate(unmapped), variant, rotations, scales, surfaces)
        return scores, variant, yx, t_hw

    def _fill_unmapped(self, q_items, g_items, pairs, rows, variant, rotations, scales, surfaces) -> None:
        """``pair_surfaces`` for the entries ``rows`` of blocks without a surfaces form: a second walk over the items they
        name, and per block and variant the maps (``mean_maps_device``) of the entries that variant won; zeros where none did."""
        q_used, g_used = (sorted({int(i) for i in pairs[rows, side]}) for side in (0, 1))
        for b in self._blocks(q_items, g_items, rotations, scales, q_used, g_used):
            q_pos = {q: i for i, q in enumerate(b.q_idx)}
            g_pos = {g: i for i, g in enumerate(b.g_idx)}
            sel = [int(i) for i in rows if int(pairs[i, 0]) in q_pos and int(pairs[i, 1]) in g_pos]
            if not sel:
                continue
            g_hw = b.plans[b.variants[0][1]].g_hw
            for i in sel:
                if variant[i] < 0:
                    surfaces[i] = np.zeros((g_hw[0] - 2 * self.crop, g_hw[1] - 2 * self.crop), np.float32)
            for number, vs, v in b.variants:
                won = [i for i in sel if variant[i] == number]
                if not won:
                    continue
                plan = b.plans[vs]
                slots = [(q_pos[int(pairs[i, 0])], g_pos[int(pairs[i, 1])]) for i in won]
                for i, m in zip(won, self.mean_maps_device(plan, self.prepare_queries(plan, v), b.prepared(vs), slots)):
                    surfaces[i] = m

    def score_matrix(self, shoemark_maps, shoeprint_maps, accumulate_into=None, rotations=None,
                     scales=None) -> np.ndarray:
        """Host float32 [Q,G] matrix for the reference's list-of-arrays inputs, including ragged
        sets (items of different spatial size): items are grouped by shape and every
        (query shape, gallery shape) class is one plan.  With ``rotations`` / ``scales`` every query
        batch is expanded on the device into the reference's variant list (variants.py) and the
        matrix keeps the running maximum over variants (similarity.py:357-367)."""
        q_items, q_dev = _as_item_list(shoemark_maps)
        g_items, g_dev = _as_item_list(shoeprint_maps)
        resident = _is_resident(shoemark_maps) or _is_resident(shoeprint_maps)
        if q_items is None and g_items is None and rotations is None and scales is None and not resident:
            return self.dev.to_host(self.scores_device(q_dev, g_dev))
        return self._walk(shoemark_maps, shoeprint_maps, accumulate_into, rotations, scales, False)[0]

    def score_matrix_located(self, shoemark_maps, shoeprint_maps, rotations=None, scales=None):
        """``score_matrix`` with, for every pair, the variant that gave its score and where that variant's NCC map peaks:
        host ``(scores float32 [Q,G], variant int32 [Q,G], yx int32 [Q,G,2])``, out of the scoring pass itself
        (spr_ncc_score_peaks) - the same walk (``_blocks``), hence the same grouping by shape, variant lists (numbered as
        ``VariantBuilder.variants`` / ``variant_labels``), gallery chunks and budget sharing, and bit for bit the same
        ``scores``.  ``yx`` is in cropped search-map coordinates; the lowest variant number wins among equal scores.  A pair
        whose score is 0 (no variant's map rises above 0) has variant -1 and yx (-1, -1).  The arg-max is taken on the
        kernels' float32 channel sums, ``locate`` sums the per-channel maps in float64: the two may name different pixels where
        the two largest sums lie within rounding of each other.  Plans without a peak form (the matrix-core methods of a
        scorer made without ``matrix_core_peaks``) are scored as ever and their blocks located by the second pass of
        ``locate``."""
        return self._score_matrix_located(shoemark_maps, shoeprint_maps, rotations, scales)[:3]

    def _score_matrix_located(self, shoemark_maps, shoeprint_maps, rotations, scales, fill_unfused: bool = True):
        """``score_matrix_located`` plus the cropped template size (th, tw) int32 [Q,V,2] of every query's variants.
        ``fill_unfused`` False leaves the blocks of plans without a peak form at variant -1 / yx (-1, -1) instead of
        running the second pass over ALL their pairs: ``retrieve`` locates only the pairs it shortlists."""
        return self._walk(shoemark_maps, shoeprint_maps, None, rotations, scales, True, fill_unfused)

    def _walk(self, shoemark_maps, shoeprint_maps, accumulate_into, rotations, scales, located: bool,
              fill_unfused: bool = True):
        """The host form of the scoring walk behind ``score_matrix`` (``located`` False: plain spr_ncc_score launches, the
        last three results are None) and ``score_matrix_located``: (scores, variant, yx, t_hw).  ``_walk_device`` folds the
        blocks on the device; the finished matrices come down once each."""
        q_items, g_items = _side(self.dev, shoemark_maps), _side(self.dev, shoeprint_maps)
        nq, ng = len(q_items), len(g_items)
        out = np.zeros((nq, ng), dtype=np.float32) if accumulate_into is None else accumulate_into
        variant = yx = t_hw = None
        if located:
            from .variants import variant_labels

            variant = np.full((nq, ng), -1, dtype=np.int32)
            yx = np.full((nq, ng, 2), -1, dtype=np.int32)
            t_hw = np.zeros((nq, len(variant_labels(rotations, scales)), 2), dtype=np.int32)
        if nq == 0 or ng == 0:
            return out, variant, yx, t_hw
        s_dev, tag_dev, packed_dev, t_hw, second_pass = self._walk_device(q_items, g_items, rotations, scales, located)
        out[...] = np.maximum(out, self.dev.to_host(s_dev))
        if located:
            variant[...] = self.dev.to_host(tag_dev)
            yx[...] = _unpack_yx(self.dev.to_host(packed_dev))
        if located and second_pass and fill_unfused:
            self._fill_unfused(q_items, g_items, second_pass, rotations, scales, out, variant, yx)
        return out, variant, yx, t_hw

    def _fill_unfused(self, q_items, g_items, second_pass, rotations, scales, out, variant, yx) -> None:
        """The second pass over the blocks of plans without a peak form: ``locate`` on every pair of them, written into the
        host matrices where the floored score is above 0 (as the fused form: no position where it is 0)."""
        pairs = np.array([(q, g) for q_idx, idx in second_pass for q in q_idx for g in idx], dtype=np.int64)
        _, p_variant, p_yx, _ = self._locate(q_items, g_items, pairs, rotations, scales)
        hit = out[pairs[:, 0], pairs[:, 1]] > 0
        variant[pairs[hit, 0], pairs[hit, 1]] = p_variant[hit]
        yx[pairs[hit, 0], pairs[hit, 1]] = p_yx[hit]

    def _walk_device(self, q_items, g_items, rotations, scales, located: bool):
        """The scoring consumer of ``_blocks``: device (scores float32 [Q,G], variant int32 [Q,G], packed position int32
        [Q,G] - ``(y << 16) | x``, -1 = none), the host t_hw, and the blocks (query indices, gallery indices) one of whose
        plans has no peak form, which stay at variant -1 / position -1.  Every block is scored into a device matrix of its
        own, all variants in ascending number through accumulate_max, and folded into the [Q,G] matrices by
        spr_block_scatter: its query and gallery indices are each distinct and every cell belongs to one block."""
        dev = self.dev
        nq, ng = len(q_items), len(g_items)
        scores = dev.zeros((nq, ng), np.float32)
        tag = packed = t_hw = None
        second_pass = []
        if located:
            from .variants import variant_labels

            tag = dev.to_device(np.full((nq, ng), -1, dtype=np.int32))
            packed = dev.to_device(np.full((nq, ng), -1, dtype=np.int32))
            t_hw = np.zeros((nq, len(variant_labels(rotations, scales)), 2), dtype=np.int32)
        if nq == 0 or ng == 0:
            return scores, tag, packed, t_hw, second_pass
        for b in self._blocks(q_items, g_items, rotations, scales):
            q_idx, idx = b.q_idx, b.g_idx
            self.last_chunk_items = b.chunk_items  # (read by the tests)
            sub = dev.zeros((len(q_idx), len(idx)), np.float32)
            fused = located and all(b.plans[vs].has_peaks for _, vs, _ in b.variants)
            sub_yx = sub_tag = None
            if fused:
                sub_yx = dev.to_device(np.full((len(q_idx), len(idx)), -1, dtype=np.int32))
                sub_tag = dev.to_device(np.full((len(q_idx), len(idx)), -1, dtype=np.int32))
            elif located:
                second_pass.append((q_idx, idx))
            for number, vs, v in b.variants:
                plan = b.plans[vs]
                if located:
                    t_hw[q_idx, number] = (vs[0] - 2 * self.crop, vs[1] - 2 * self.crop)  # (the same in every chunk)
                pg = b.prepared(vs)
                self.score_prepared(plan, self.prepare_queries(plan, v), len(q_idx), pg, len(idx), sub, len(idx), 0,
                                    accumulate_max=True, peaks=sub_yx, tags=sub_tag, tag=number)
            rows = dev.to_device(np.asarray(q_idx, dtype=np.int32))
            cols = dev.to_device(np.asarray(idx, dtype=np.int32))
            for dst, src, mode in ((scores, sub, 1), (tag, sub_tag, 0), (packed, sub_yx, 0)):
                if src is not None:
                    self.lib.check(self.lib.spr_block_scatter(dev.ptr(dst), ng, dev.ptr(src), len(idx), dev.ptr(rows),
                                                              len(q_idx), dev.ptr(cols), len(idx), mode, dev.stream()))
        return scores, tag, packed, t_hw, second_pass

    def score_matrix_device(self, q, g, rotations=None, scales=None, located: bool = False):
        """``score_matrix`` that leaves its result in HBM: the device float32 [Q,G] matrix of any accepted inputs (host
        lists or ``FeatureSet``s, either per side).  With ``located`` also, as ``score_matrix_located``, the device int32
        [Q,G] variant numbers and packed positions ``(y << 16) | x`` (-1 where the score is 0) and the host t_hw int32
        [Q,V,2]: ``(scores, variant, packed_yx, t_hw)``.  Blocks of plans without a peak form are located by the second pass
        of ``locate``, which needs the host copy of the scores to know where they are above 0: such a scorer pays one
        transfer of the matrix down and of the two int32 matrices up."""
        q_items, g_items = _side(self.dev, q), _side(self.dev, g)
        s_dev, tag, packed, t_hw, second_pass = self._walk_device(q_items, g_items, rotations, scales, located)
        if not located:
            return s_dev
        if second_pass:
            out, variant, yx = self.dev.to_host(s_dev), self.dev.to_host(tag), _unpack_yx(self.dev.to_host(packed))
            self._fill_unfused(q_items, g_items, second_pass, rotations, scales, out, variant, yx)
            tag = self.dev.to_device(variant)
            packed = self.dev.to_device(np.where(variant < 0, -1, (yx[..., 0] << 16) | yx[..., 1]).astype(np.int32))
        return s_dev, tag, packed, t_hw

    def cells_device(self, matrix, ld: int, qs, gs) -> np.ndarray:
        """Host copy of the 4-byte cells ``matrix[qs[i], gs[i]]`` of a dense device [Q, ld] matrix (float32 or int32; the
        result has the bits as int32): one spr_items_gather of one-element items, so a shortlist's entries come down and not
        the matrix."""
        dev = self.dev
        flat = np.asarray(qs, dtype=np.int64) * int(ld) + np.asarray(gs, dtype=np.int64)
        if len(flat) == 0:
            return np.zeros(0, dtype=np.int32)
        if flat.max() >= 2 ** 31:
            raise ValueError("matrix too large for a 32-bit cell index")
        out = dev.empty((len(flat),), np.int32)
        index = dev.to_device(flat.astype(np.int32))
        self.lib.check(self.lib.spr_items_gather(dev.ptr(matrix), 1, dev.ptr(index), len(flat), dev.ptr(out), _lib.F32,
                                                 dev.stream()))
        return dev.to_host(out).astype(np.int32, copy=False)

    def multi_layer_scores_device(self, layers, out=None):
        """Device [Q,G] float32 mean over feature layers of the per-layer score matrices (e.g.
        conv3_3 + conv4_3 + conv5_3 maps of the same items; build-defined, the reference scores one layer).
        ``layers`` = [(q_dev [Q,C_l,h_l,w_l], g_dev [G,C_l,h_l,w_l]), ...] resident in HBM.  Nothing leaves the
        device: each layer's matrix is folded into the running mean by spr_scores_fuse."""
        layers = list(layers)
        if not layers:
            raise ValueError("no feature layers given")
        weight = 1.0 / len(layers)
        layer_scores = None
        for k, (q_dev, g_dev) in enumerate(layers):
            nq, ng = self.dev.shape(q_dev)[0], self.dev.shape(g_dev)[0]
            if out is None:
                out = self.dev.zeros((nq, ng), np.float32)
            if layer_scores is None:
                layer_scores = self.dev.zeros((nq, ng), np.float32)
            self.scores_device(q_dev, g_dev, scores=layer_scores)
            self.lib.check(self.lib.spr_scores_fuse(self.dev.ptr(out), self.dev.ptr(layer_scores), nq * ng,
                                                    0.0 if k == 0 else 1.0, weight, self.dev.stream()))
        return out

    def multi_layer_score_matrix_device(self, layer_sets, rotations=None, scales=None):
        """The ragged, variant-aware sibling of ``multi_layer_scores_device``: ``layer_sets`` = [(query ``FeatureSet``,
        gallery ``FeatureSet``), ...], one pair per feature layer of the same items (``Model.
        get_multiple_feature_maps_device(taps=...)``; host lists are taken too).  Each layer's matrix is its
        ``score_matrix_device`` - the maximum over the query variants of ``rotations`` x ``scales`` - and spr_scores_fuse
        folds them into the device float32 [Q,G] mean.  Nothing leaves the device."""
        layer_sets = list(layer_sets)
        if not layer_sets:
            raise ValueError("no feature layers given")
        weight = 1.0 / len(layer_sets)
        out = None
        for k, (q, g) in enumerate(layer_sets):
            layer_scores = self.score_matrix_device(q, g, rotations=rotations, scales=scales)
            nq, ng = self.dev.shape(layer_scores)
            if out is None:
                out = self.dev.zeros((nq, ng), np.float32)
            elif tuple(self.dev.shape(out)) != (nq, ng):
                raise ValueError(f"layer {k} scores {nq} x {ng} items, the layers before it {tuple(self.dev.shape(out))}")
            if nq * ng:
                self.lib.check(self.lib.spr_scores_fuse(self.dev.ptr(out), self.dev.ptr(layer_scores), nq * ng,
                                                        0.0 if k == 0 else 1.0, weight, self.dev.stream()))
        return out

    def multi_layer_score_matrix(self, layers) -> np.ndarray:
        """Host copy of multi_layer_scores_device (one transfer, of the fused matrix)."""
        return self.dev.to_host(self.multi_layer_scores_device(layers))

    def ranks(self, scores_host: np.ndarray, matching_pairs: Sequence[int]) -> np.ndarray:
        nq, ng = scores_host.shape
        if nq == 0:
            return np.zeros(0, dtype=np.int32)
        return self.ranks_of_device(self.dev.to_device(np.ascontiguousarray(scores_host, dtype=np.float32)), matching_pairs)

    def ranks_of_device(self, s_dev, matching_pairs: Sequence[int]) -> np.ndarray:
        """``ranks`` of a score matrix that is already in HBM (``score_matrix_device``): only the rank vector comes down."""
        if self.dev.shape(s_dev)[0] == 0:
            return np.zeros(0, dtype=np.int32)
        m_dev = self.dev.to_device(np.asarray(matching_pairs, dtype=np.int32))
        ranks = self.dev.to_host(self.ranks_device(s_dev, m_dev)).astype(np.int32, copy=True)
        if (ranks == 0).any():
            # the reference's np.where(...)[0][0] raises IndexError when the id is not in the gallery
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")
        return ranks


def _require_contiguous(buf, name: str) -> None:
    """The C ABI takes dense row-major buffers: refuse a strided view instead of reading the wrong elements."""
    check = getattr(buf, "is_contiguous", None)
    if not (check() if check is not None else buf.flags["C_CONTIGUOUS"]):
        raise ValueError(f"{name} must be contiguous")


def _unpack_yx(packed) -> np.ndarray:
    """Packed positions ``(y << 16) | x`` -> int32 [..., 2]; -1 (no position) -> (-1, -1)."""
    packed = np.asarray(packed).astype(np.int32, copy=False)
    return np.where((packed < 0)[..., None], -1, np.stack([packed >> 16, packed & 0xFFFF], axis=-1)).astype(np.int32)


def _group_by_shape(items, used=None) -> dict[tuple, list[int]]:
    """Shape -> indices of the items of that shape, of all items or of those ``used`` names."""
    groups: dict[tuple, list[int]] = {}
    for i in range(len(items)) if used is None else used:
        if items[i].ndim != 3:
            raise ValueError("feature maps must be [C, h, w] (customtypes.py:11-14)")
        groups.setdefault(tuple(items[i].shape), []).append(i)
    return groups


class _Block(NamedTuple):
    """One (gallery chunk, query shape class) of ``NccScorer._blocks``."""

    q_idx: list        # the class's query indices, in the order of its variant batches
    variants: list     # [(variant number, variant (h, w), device batch [len(q_idx), C, h, w] in storage type), ...], ascending
    g_idx: list        # the chunk's gallery indices
    plans: dict        # variant (h, w) -> plan against the gallery class
    chunk_items: int   # the chunk size the budget gave this gallery class
    prepared: Any      # prepared(variant (h, w)) -> the chunk's prepared form for that plan


# ---------------------------------------------------------------------------------------------
# The reference's call surface
# ---------------------------------------------------------------------------------------------
_default_scorer: NccScorer | None = None


def default_scorer() -> NccScorer:
    global _default_scorer
    if _default_scorer is None:
        _default_scorer = NccScorer()
    return _default_scorer


_config_scorers: dict[tuple, NccScorer] = {}


def scorer_from_config(config: dict, *, device=None, library: _lib.Library | None = None) -> NccScorer:
    """The scorer that ``[mi355x]`` of run.toml asks for: ``ncc_method`` ("auto" | "fft" | "fft_pow2" | "direct" | "mfma" |
    "mfma_f32"), ``dtype`` (HBM storage type of the feature maps: "float32" | "float16" | "bfloat16"), ``max_prepared_gib``
    (HBM budget of one prepared gallery chunk; 0 = automatic), ``f32_matrix_cores`` and ``matrix_core_peaks`` (see
    NccScorer).  Reference files, which have no such table, get the defaults."""
    extra = config.get("mi355x") or {}
    method = extra.get("ncc_method", "auto") or "auto"
    storage = extra.get("dtype", "float32") or "float32"
    gib = float(extra.get("max_prepared_gib", 0.0) or 0.0)
    if method not in _METHODS:
        raise ValueError(f"[mi355x].ncc_method = {method!r}: expected one of {sorted(_METHODS)}")
    f32_mc = bool(extra.get("f32_matrix_cores", False))
    mc_peaks = bool(extra.get("matrix_core_peaks", False))
    key = (method, storage, gib, f32_mc, mc_peaks, id(device), id(library))
    if key == ("auto", "float32", 0.0, False, False, id(None), id(None)):
        return default_scorer()
    if key not in _config_scorers:
        _config_scorers[key] = NccScorer(device=device, library=library, method=method, storage=storage,
                                         f32_matrix_cores=f32_mc, matrix_core_peaks=mc_peaks,
                                         max_prepared_bytes=int(gib * (1 << 30)) if gib > 0 else None)
    return _config_scorers[key]


def compare_maps(
    shoemark_maps: list[np.ndarray],
    shoeprint_maps: list[np.ndarray],
    matching_pairs: list[int],
    config: dict,
    *,
    scorer: NccScorer | None = None,
    progress: bool = False,
) -> np.ndarray:
    """Ranks (1-based, int32 [Q]) of every query's true match — reference similarity.py:129-227.

    ``matching_pairs[i]`` is the index into ``shoeprint_maps`` of query i's true match;
    ``config["comparison"]`` supplies ``n_processes`` (ignored: the GPU grid replaces the
    process pool), ``rotations`` and ``scales`` (query variants, see variants.py; with both set the
    reference builds 1 + (R+1)*S variant lists and — a latent defect, SURVEY §4 — then waits forever for
    (R+1)*(S+1) progress ticks; the variant lists are reproduced, the hang is not).
    """
    comp = config["comparison"]
    rotations, scales = comp.get("rotations"), comp.get("scales")
    scorer = scorer or scorer_from_config(config)
    if _is_resident(shoemark_maps) and _is_resident(shoeprint_maps):
        # features.FeatureSet on both sides: the matrix is ranked where it was folded, only the rank vector comes down
        ranks = scorer.ranks_of_device(scorer.score_matrix_device(shoemark_maps, shoeprint_maps, rotations, scales),
                                       matching_pairs)
    else:
        scores = scorer.score_matrix(shoemark_maps, shoeprint_maps, rotations=rotations, scales=scales)
        ranks = scorer.ranks(scores, matching_pairs)
    if progress:
        for i, r in enumerate(ranks):
            print(f"Print {i} true match ranked {r}")  # similarity.py:375
    return ranks


@dataclass
class Shortlist:
    """What ``retrieve`` returns.  Slot [q, p] is the gallery item ranked p + 1 for query q; slots beyond the gallery size
    hold index -1 (score 0, and with ``locate``: variant -1, peak_yx (-1, -1), offset (0, 0)).  The last four fields are
    filled by ``retrieve(..., surfaces=True)``: what an examiner judges the peak by.  Empty slots hold None / 0 / 0 / -1."""

    index: np.ndarray            # int32 [Q,k] gallery index
    score: np.ndarray            # float32 [Q,k] its entry of the score matrix (floored at 0, maximum over variants)
    variant: np.ndarray | None   # int32 [Q,k] number of the best query variant (variants.variant_labels names them)
    peak_yx: np.ndarray | None   # int32 [Q,k,2] peak of that variant's channel-summed NCC map, cropped gallery-map coordinates
    offset: np.ndarray | None    # int32 [Q,k,2] top-left corner of the cropped variant template in the cropped gallery map
    surface: np.ndarray | None = None         # object [Q,k]: float32 [ih,iw] channel-mean NCC map of the best variant (``pair_surfaces``)
    psr: np.ndarray | None = None             # float32 [Q,k] peak-to-sidelobe ratio of that map's maximum (spr_surface_peaks)
    peak_values: np.ndarray | None = None     # float32 [Q,k,peaks] the map's best separated peaks, the maximum first
    peak_positions: np.ndarray | None = None  # int32 [Q,k,peaks,2] where they lie, (-1, -1) = no pixel left


def retrieve(
    shoemark_maps: list[np.ndarray],
    shoeprint_maps: list[np.ndarray],
    config: dict,
    k: int = 10,
    *,
    locate: bool = True,
    scorer: NccScorer | None = None,
    surfaces: bool = False,
    peaks: int = 2,
) -> Shortlist:
    """The ``k`` best gallery items of every query (1 <= k <= 256), best first in the ranker's order, and - with
    ``locate`` - for each of them the best query variant, the peak of its NCC map and the offset
    ``(y - th//2, x - tw//2)`` at which the cropped ``th x tw`` variant template lies on the cropped gallery map.
    ``config["comparison"]`` supplies rotations and scales as for ``compare_maps``.  With a ``features.FeatureSet`` on both
    sides the score matrix never leaves HBM (``retrieve_resident``).  With ``surfaces`` every shortlisted pair also gets
    its correlation surface (``NccScorer.pair_surfaces``: one more pass over the Q * k pairs), the surface's ``peaks`` best
    separated peaks (1..8) and the peak-to-sidelobe ratio of its maximum (spr_surface_peaks).  The exclusion window is half
    the winning variant's cropped template, ``ry = th // 2, rx = tw // 2``: the runner-up is an alignment whose template
    centre lies outside the best one's footprint.  Everything else is what it is without the keyword, bit for bit."""
    kw = {"locate": locate, "scorer": scorer, "surfaces": surfaces, "peaks": peaks}
    if _is_resident(shoemark_maps) and _is_resident(shoeprint_maps):
        return retrieve_resident(shoemark_maps, shoeprint_maps, config, k, **kw)[1]
    return retrieve_with_scores(shoemark_maps, shoeprint_maps, config, k, **kw)[1]


def retrieve_with_scores(shoemark_maps, shoeprint_maps, config: dict, k: int = 10, *, locate: bool = True,
                         scorer: NccScorer | None = None, surfaces: bool = False,
                         peaks: int = 2) -> tuple[np.ndarray, Shortlist]:
    """``retrieve`` together with the host float32 [Q,G] score matrix it was taken from (what ``score_matrix`` gives for
    these maps and variants, bit for bit): one scoring pass serves ranks of known matches and the shortlist
    (run_mi355x.py).  With ``locate`` the pass is ``score_matrix_located``'s list-of-arrays walk - device-resident
    batches are copied to the host and uploaded again by shape group, where ``locate=False`` keeps ``score_matrix``'s
    device route - and blocks of plans without a peak form are not filled: their shortlisted pairs, Q*k of them, go
    through the second pass as entries with score 0 do.  ``features.FeatureSet``s on both sides stay in HBM throughout
    (``retrieve_resident``); the matrix comes down once, because it is returned."""
    comp = config["comparison"]
    rotations, scales = comp.get("rotations"), comp.get("scales")
    scorer = scorer or scorer_from_config(config)
    if _is_resident(shoemark_maps) and _is_resident(shoeprint_maps):
        s_dev, short = retrieve_resident(shoemark_maps, shoeprint_maps, config, k, locate=locate, scorer=scorer,
                                         surfaces=surfaces, peaks=peaks)
        return scorer.dev.to_host(s_dev), short
    if not locate:
        scores = scorer.score_matrix(shoemark_maps, shoeprint_maps, rotations=rotations, scales=scales)
        short = _shortlist(scorer, shoemark_maps, shoeprint_maps, scores, k, False, rotations, scales)
    else:
        scores, *located = scorer._score_matrix_located(shoemark_maps, shoeprint_maps, rotations, scales, fill_unfused=False)
        short = _shortlist(scorer, shoemark_maps, shoeprint_maps, scores, k, True, rotations, scales, located=located)
    if surfaces:
        _add_surfaces(scorer, short, shoemark_maps, shoeprint_maps, rotations, scales, peaks)
    return scores, short


def retrieve_resident(shoemark_maps, shoeprint_maps, config: dict, k: int = 10, *, locate: bool = True,
                      scorer: NccScorer | None = None, surfaces: bool = False, peaks: int = 2):
    """``retrieve_with_scores`` for ``features.FeatureSet``s that leaves the matrix where it is: (device float32 [Q,G]
    scores, Shortlist).  The top k are taken from the device matrix and the shortlisted entries' variant and position are
    gathered from the device matrices; what comes down is the Shortlist's own arrays (and ``locate``'s per-pair results for
    entries the scoring pass has no position for)."""
    comp = config["comparison"]
    rotations, scales = comp.get("rotations"), comp.get("scales")
    scorer = scorer or scorer_from_config(config)
    if not locate:
        s_dev = scorer.score_matrix_device(shoemark_maps, shoeprint_maps, rotations, scales)
        short = _shortlist(scorer, shoemark_maps, shoeprint_maps, s_dev, k, False, rotations, scales, resident=True)
    else:
        q_items, g_items = _side(scorer.dev, shoemark_maps), _side(scorer.dev, shoeprint_maps)
        s_dev, *located = scorer._walk_device(q_items, g_items, rotations, scales, True)[:4]  # (unfused blocks: not filled)
        short = _shortlist(scorer, shoemark_maps, shoeprint_maps, s_dev, k, True, rotations, scales, located=located,
                           resident=True)
    if surfaces:
        _add_surfaces(scorer, short, shoemark_maps, shoeprint_maps, rotations, scales, peaks)
    return s_dev, short


def _add_surfaces(scorer: NccScorer, short: Shortlist, shoemark_maps, shoeprint_maps, rotations, scales, peaks: int) -> None:
    """The four surface fields of a shortlist: ``pair_surfaces`` of its entries, then spr_surface_peaks per map shape and
    exclusion window (half the winning variant's cropped template).  Nothing else of ``short`` is touched."""
    if isinstance(peaks, bool) or int(peaks) != peaks or not 1 <= int(peaks) <= 8:
        raise ValueError(f"peaks = {peaks!r}: expected an integer in [1, 8]")
    peaks = int(peaks)
    dev = scorer.dev
    nq, kk = short.index.shape
    short.surface = np.full((nq, kk), None, dtype=object)
    short.psr = np.zeros((nq, kk), dtype=np.float32)
    short.peak_values = np.zeros((nq, kk, peaks), dtype=np.float32)
    short.peak_positions = np.full((nq, kk, peaks, 2), -1, dtype=np.int32)
    qs, ps = np.nonzero(short.index >= 0)
    if len(qs) == 0:
        return
    *_, t_hw, maps = scorer.pair_surfaces(shoemark_maps, shoeprint_maps, np.stack([qs, short.index[qs, ps]], axis=1),
                                          rotations=rotations, scales=scales)
    groups: dict[tuple, list[int]] = {}
    for i, m in enumerate(maps):
        short.surface[qs[i], ps[i]] = m
        groups.setdefault((m.shape, int(t_hw[i, 0]) // 2, int(t_hw[i, 1]) // 2), []).append(i)
    for (_, ry, rx), rows in groups.items():
        values, yx, psr = scorer.surface_peaks_device(dev.to_device(np.stack([maps[i] for i in rows])), peaks, ry, rx)
        short.peak_values[qs[rows], ps[rows]] = dev.to_host(values)
        short.peak_positions[qs[rows], ps[rows]] = _unpack_yx(dev.to_host(yx))
        short.psr[qs[rows], ps[rows]] = dev.to_host(psr)


def _shortlist(scorer: NccScorer, shoemark_maps, shoeprint_maps, scores, k: int, locate: bool, rotations,
               scales, located=None, resident: bool = False) -> Shortlist:
    """``retrieve`` behind its score matrix: ``scores`` is what ``scorer.score_matrix`` gave for these maps and variants
    (run_mi355x.py ranks from the same matrix instead of scoring twice).  ``located`` = the (variant, yx, t_hw) that
    ``scorer._score_matrix_located`` gave beside ``scores``: the shortlisted entries are gathered from them, and only those
    whose score is 0 - the scoring pass has no position for them - go through the second pass of ``NccScorer.locate``, which
    gives the un-floored peak (without ``located``: all of them).  ``resident``: ``scores`` is the device matrix of
    ``score_matrix_device`` instead, ``located`` its device (variant, packed position) matrices and the host t_hw:
    nothing is uploaded again and only the shortlisted cells come down (``NccScorer.cells_device``)."""
    dev = scorer.dev
    top_s, top_i = scorer.topk_device(scores if resident else dev.to_device(np.ascontiguousarray(scores, dtype=np.float32)), k)
    out = Shortlist(dev.to_host(top_i).astype(np.int32, copy=True), dev.to_host(top_s).astype(np.float32, copy=True),
                    None, None, None)
    if not locate:
        return out
    nq, kk = out.index.shape
    out.variant = np.full((nq, kk), -1, dtype=np.int32)
    out.peak_yx = np.full((nq, kk, 2), -1, dtype=np.int32)
    out.offset = np.zeros((nq, kk, 2), dtype=np.int32)
    qs, ps = np.nonzero(out.index >= 0)
    if len(qs) == 0:
        return out
    gs = out.index[qs, ps]

    def put(qs, ps, variant, yx, t_hw):
        out.variant[qs, ps], out.peak_yx[qs, ps], out.offset[qs, ps] = variant, yx, yx - t_hw // 2

    if located is not None:
        all_variant, all_yx, all_t_hw = located
        if resident:
            ng = dev.shape(scores)[1]
            variant = scorer.cells_device(all_variant, ng, qs, gs)
            cell_yx = _unpack_yx(scorer.cells_device(all_yx, ng, qs, gs))
        else:
            variant, cell_yx = all_variant[qs, gs], all_yx[qs, gs]
        put(qs, ps, variant, cell_yx, all_t_hw[qs, np.maximum(variant, 0)])
        rest = variant < 0
        qs, ps, gs = qs[rest], ps[rest], gs[rest]
        if len(qs) == 0:
            return out
    put(qs, ps, *scorer._locate(shoemark_maps, shoeprint_maps, np.stack([qs, gs], axis=1), rotations, scales)[1:])
    return out


@dataclass
class Cascade:
    """What ``retrieve_cascade`` returns: per query its ``depth`` = M best prints of the coarse layer, re-ranked by the fused
    score of all layers.  Slot [q, p] is the candidate ranked p + 1; slots beyond the gallery size hold index -1 (score 0,
    variant -1, peak_yx (-1, -1), offset (0, 0)), and so do the located fields of a candidate whose located layer scores 0."""

    coarse: Any                  # device float32 [Q,G]: the coarse layer's score matrix
    index: np.ndarray            # int32 [Q,M] gallery index, best first
    score: np.ndarray            # float32 [Q,M] fused score: the mean over the layers, the bits of the full fused matrix's cell
    variant: np.ndarray          # int32 [Q,M] best query variant on the located layer
    peak_yx: np.ndarray          # int32 [Q,M,2] peak of that variant's NCC map, cropped gallery-map coordinates of that layer
    offset: np.ndarray           # int32 [Q,M,2] top-left corner of the cropped variant template in the cropped gallery map
    scorer: Any = None
    located: Any = None          # (query set, gallery set, rotations, scales) of the located layer: ``shortlist(surfaces=True)``

    def shortlist(self, k: int, *, surfaces: bool = False, peaks: int = 2) -> Shortlist:
        """The first ``k`` columns (1 <= k <= M) as ``retrieve`` lays them out.  With ``surfaces`` the four surface fields
        of ``retrieve(..., surfaces=True)``, on the located layer."""
        if not 1 <= int(k) <= self.index.shape[1]:
            raise ValueError(f"k = {k}: the cascade holds {self.index.shape[1]} candidates per query")
        k = int(k)
        short = Shortlist(self.index[:, :k].copy(), self.score[:, :k].copy(), self.variant[:, :k].copy(),
                          self.peak_yx[:, :k].copy(), self.offset[:, :k].copy())
        if surfaces:
            q, g, rotations, scales = self.located
            _add_surfaces(self.scorer, short, q, g, rotations, scales, peaks)
        return short

    def ranks(self, matching_pairs: Sequence[int]) -> np.ndarray:
        """int32 [Q]: the position of query q's match among its re-ranked candidates + 1 where it is one of them, otherwise
        its rank in the coarse matrix (``ranks_of_device``), which is above M by construction.  A match index outside the
        gallery raises the reference's IndexError."""
        ranks = self.scorer.ranks_of_device(self.coarse, matching_pairs)
        match = np.asarray(matching_pairs, dtype=np.int64)
        for q in range(len(ranks)):
            at = np.flatnonzero(self.index[q] == match[q])
            if len(at):
                ranks[q] = at[0] + 1
        return ranks


def retrieve_cascade(layer_sets, config: dict, depth: int, *, coarse: int = -1, locate_layer: int | None = None,
                     scorer: NccScorer | None = None) -> Cascade:
    """Coarse-to-fine retrieval over feature layers of the same items.  ``layer_sets`` = [(query set, gallery set), ...] as
    ``multi_layer_score_matrix_device`` takes them.  Layer ``coarse`` - the cheap one - is scored against the whole gallery
    (``score_matrix_device``); per query its M = ``depth`` best prints (``topk_device``: the ranker's order) are the
    candidates; every other layer scores only those Q * M pairs (``score_pairs``: spr_ncc_score_list); the candidates' fused
    score is the mean over all layers, folded by spr_scores_fuse in the order of ``layer_sets`` exactly as the full fused
    matrix is, so a candidate's fused score has the bits of that matrix's cell; and the candidates are re-ranked by it
    (``topk_device`` in its merging form: ties go to the larger gallery index).  With ``depth`` >= G the result is the
    ranking of the full fused matrix; below that, a query whose match is no candidate keeps its coarse rank.
    ``config["comparison"]`` supplies rotations and scales.  ``locate_layer`` (default: the first layer that is not the
    coarse one, the finest) gives the located fields.  1 <= depth <= 256; at least two layers."""
    layer_sets = list(layer_sets)
    if len(layer_sets) < 2:
        raise ValueError(f"a cascade needs at least two feature layers, got {len(layer_sets)}")
    if isinstance(depth, bool) or int(depth) != depth or not 1 <= int(depth) <= 256:
        raise ValueError(f"depth = {depth!r}: expected an integer in [1, 256]")
    n_layers = len(layer_sets)
    if not -n_layers <= coarse < n_layers:
        raise ValueError(f"coarse = {coarse}: there are {n_layers} layers")
    coarse %= n_layers
    if locate_layer is None:
        locate_layer = 0 if coarse != 0 else 1
    if not -n_layers <= locate_layer < n_layers:
        raise ValueError(f"locate_layer = {locate_layer}: there are {n_layers} layers")
    locate_layer %= n_layers
    comp = config["comparison"]
    rotations, scales = comp.get("rotations"), comp.get("scales")
    scorer = scorer or scorer_from_config(config)
    dev, lib = scorer.dev, scorer.lib
    m = min(int(depth), 256)
    coarse_scores = scorer.score_matrix_device(*layer_sets[coarse], rotations=rotations, scales=scales)
    nq, ng = dev.shape(coarse_scores)
    for k, (q, g) in enumerate(layer_sets):
        if (len(_side(dev, q)), len(_side(dev, g))) != (nq, ng):
            raise ValueError(f"layer {k} holds {len(_side(dev, q))} x {len(_side(dev, g))} items, the coarse layer {nq} x {ng}")
    out = Cascade(coarse_scores, np.full((nq, m), -1, np.int32), np.zeros((nq, m), np.float32), np.full((nq, m), -1, np.int32),
                  np.full((nq, m, 2), -1, np.int32), np.zeros((nq, m, 2), np.int32), scorer,
                  (*layer_sets[locate_layer], rotations, scales))
    if nq == 0:
        return out
    top_s, top_i = scorer.topk_device(coarse_scores, m)
    candidates = dev.to_host(top_i).astype(np.int32, copy=True)
    qs, ps = np.nonzero(candidates >= 0)
    pairs = np.stack([qs, candidates[qs, ps]], axis=1)
    weight = 1.0 / n_layers
    fused = dev.zeros((nq, m), np.float32)
    located = None
    for k, (q, g) in enumerate(layer_sets):
        if k == coarse:
            layer = top_s
        else:
            got = scorer.score_pairs(q, g, pairs, rotations=rotations, scales=scales)
            if k == locate_layer:
                located = got
            vec = np.zeros((nq, m), np.float32)
            vec[qs, ps] = got[0]
            layer = dev.to_device(vec)
        lib.check(lib.spr_scores_fuse(dev.ptr(fused), dev.ptr(layer), nq * m, 0.0 if k == 0 else 1.0, weight, dev.stream()))
    if located is None:  # (the coarse layer was asked to locate: its candidates' pairs, scored once more with positions)
        located = scorer.score_pairs(*layer_sets[locate_layer], pairs, rotations=rotations, scales=scales)
    top_s, top_i = scorer.topk_device(fused, m, col_index=dev.to_device(candidates))
    out.score[...] = dev.to_host(top_s)
    out.index[...] = dev.to_host(top_i)
    # the located fields follow their candidates to the re-ranked positions
    slot = np.full((nq, ng), -1, dtype=np.int64)
    slot[qs, candidates[qs, ps]] = np.arange(len(qs))
    rq, rp = np.nonzero(out.index >= 0)
    src = slot[rq, out.index[rq, rp]]
    _, variant, yx, t_hw = located
    out.variant[rq, rp], out.peak_yx[rq, rp] = variant[src], yx[src]
    out.offset[rq, rp] = np.where((variant[src] >= 0)[:, None], yx[src] - t_hw[src] // 2, 0)
    return out


def _pair_maps(scorer: NccScorer | None, template: np.ndarray, image: np.ndarray, crop: int | None) -> np.ndarray:
    """Host float32 [C, ih, iw] NCC maps of one [C, h, w] template over one [C, h', w'] image."""
    scorer = scorer or default_scorer()
    t = np.ascontiguousarray(template, dtype=np.float32)
    i = np.ascontiguousarray(image, dtype=np.float32)
    plan = scorer.plan(t.shape[0], t.shape[1:], i.shape[1:], crop=crop)
    pq = scorer.prepare_queries(plan, scorer.dev.to_device(t[None]))
    pg = scorer.prepare_gallery(plan, scorer.dev.to_device(i[None]))
    return scorer.dev.to_host(scorer.ncc_maps_device(plan, pq, pg))


def get_similarity(shoemark: np.ndarray, shoeprint: np.ndarray, *, scorer: NccScorer | None = None) -> np.floating[Any]:
    """max over positions of the channel-summed NCC maps, divided by the channel count
    (similarity.py:75-108); both stacks are cropped by 2 pixels per edge first."""
    maps = _pair_maps(scorer, shoemark, shoeprint, None).astype(np.float64)
    return np.max(maps.sum(axis=0)) / maps.shape[0]


def normxcorr(template: np.ndarray, image: np.ndarray, mode: str = "same", *, scorer: NccScorer | None = None) -> np.ndarray:
    """Normalised cross-correlation map of ``template`` over ``image`` (similarity.py:26-72)."""
    if mode != "same":
        raise NotImplementedError("only mode='same' is on the hot path (similarity.py:104)")
    return _pair_maps(scorer, np.asarray(template)[None], np.asarray(image)[None], 0)[0]
