"""Ragged sets that live in HBM: ``FeatureSet`` (what the extractor hands to the scorer) and ``DeviceImages`` (what the
loader hands to the extractor).

The reference passes Python lists of arrays between its stages; items may differ in size (FID-300 crime-scene marks, the
size clusters of dataloader.py).  A ragged set keeps such a list on the device as *shape classes*: per distinct item shape
one dense batch and the caller's index of every item in it.  Classes come in the order in which their shape first appears
in the list - the order ``similarity._group_by_shape`` gives for a host list - so a walk over a set makes the plans and
launches of the same walk over the list.

Only backend methods that every device backend has are used here (allocation, ``to_device`` / ``to_host``, ``narrow0``,
``ptr``); items are picked out of a class with ``spr_items_gather`` (csrc/resident.hip) through the C ABI.
"""

from __future__ import annotations

import numpy as np

from . import _lib

_STORAGE = {"float32": _lib.F32, "float16": _lib.F16, "bfloat16": _lib.BF16}


class _RaggedSet:
    """``classes`` = [(item shape, int32 item indices, device batch [n_k, *shape]), ...]: row r of a batch is item
    ``indices[r]`` of the set.  ``from_host`` gives ascending indices per class; a set assembled on the device may hold
    them in any order (the extractor lays image classes that share a feature shape one behind the other)."""

    dtype = np.float32

    def __init__(self, dev, n: int, classes):
        self.dev = dev
        self._n = int(n)
        self.classes = [(tuple(int(s) for s in shape), np.ascontiguousarray(idx, dtype=np.int32), batch)
                        for shape, idx, batch in classes]
        self._where = np.full((self._n, 2), -1, dtype=np.int64)  # item -> (class, row)
        seen = {}
        for k, (shape, idx, batch) in enumerate(self.classes):
            if shape in seen:
                raise ValueError(f"two classes of shape {shape}: a shape class is one batch")
            seen[shape] = k
            if tuple(dev.shape(batch)) != (len(idx),) + shape:
                raise ValueError(f"class {shape}: batch is {tuple(dev.shape(batch))}, {len(idx)} items named")
            if len(idx) and (idx.min() < 0 or idx.max() >= self._n or (self._where[idx, 0] >= 0).any()):
                raise ValueError(f"class {shape}: item indices outside the set or named twice")
            self._where[idx, 0] = k
            self._where[idx, 1] = np.arange(len(idx))
        if (self._where[:, 0] < 0).any():
            raise ValueError("the classes do not name every item of the set")

    def __len__(self) -> int:
        return self._n

    @property
    def nbytes(self) -> int:
        size = np.dtype(self.dtype).itemsize
        return sum(len(idx) * int(np.prod(shape)) * size for shape, idx, _ in self.classes)

    def shape_of(self, i: int) -> tuple:
        return self.classes[self._where[i, 0]][0]

    @classmethod
    def from_host(cls, dev, items):
        """Upload a list of host arrays, one transfer per shape class."""
        groups: dict[tuple, list[int]] = {}
        for i, a in enumerate(items):
            cls._check_item(a)
            groups.setdefault(tuple(a.shape), []).append(i)
        return cls(dev, len(items), [(shape, idx, cls._upload(dev, [items[i] for i in idx])) for shape, idx in groups.items()])

    def to_host_list(self) -> list[np.ndarray]:
        """The set as the list the host route passes around: fresh C-contiguous arrays in caller order."""
        out: list = [None] * self._n
        for _, idx, batch in self.classes:
            host = self.dev.to_host(batch)
            for r, i in enumerate(idx):
                out[i] = np.ascontiguousarray(host[r])
        return out


class FeatureSet(_RaggedSet):
    """Feature maps float32 [C, h, w] of a query or gallery set, resident in HBM."""

    dtype = np.float32

    @staticmethod
    def _check_item(a) -> None:
        if a.ndim != 3:
            raise ValueError("feature maps must be [C, h, w] (customtypes.py:11-14)")

    @staticmethod
    def _upload(dev, items):
        return dev.stack_to_device(items)

    def groups(self, used=None) -> dict[tuple, list[int]]:
        """Shape -> indices of the items of that shape, of all items or of those ``used`` names: what
        ``similarity._group_by_shape`` gives for the host list."""
        groups: dict[tuple, list[int]] = {}
        for i in range(self._n) if used is None else used:
            groups.setdefault(self.classes[self._where[i, 0]][0], []).append(int(i))
        return groups

    def stack(self, lib, idx, storage: str | None = None):
        """Device batch [len(idx), C, h, w] of the items ``idx`` (one shape class) in ``storage`` (None: float32):
        spr_items_gather, the cast fused in.  A whole class asked for in its own order as float32 is the class batch itself.
        16-bit results sit in a float16-typed buffer whatever the storage: a 2-byte container, the plan knows the type."""
        dev = self.dev
        where = self._where[np.asarray(idx, dtype=np.int64)]
        k = int(where[0, 0])
        if (where[:, 0] != k).any():
            raise ValueError("the items of one stack must share a shape")
        shape, _, batch = self.classes[k]
        code = _STORAGE[storage or "float32"]
        rows = where[:, 1]
        if code == _lib.F32 and len(rows) == dev.shape(batch)[0] and (rows == np.arange(len(rows))).all():
            return batch
        out = dev.empty((len(rows),) + shape, np.float32 if code == _lib.F32 else np.float16)
        index = dev.to_device(rows.astype(np.int32))
        lib.check(lib.spr_items_gather(dev.ptr(batch), int(np.prod(shape)), dev.ptr(index), len(rows), dev.ptr(out), code,
                                       dev.stream()))
        return out


class DeviceImages(_RaggedSet):
    """uint8 images, grey [H, W] or RGB [H, W, 3], resident in HBM: per class a batch [n_k, H, W] or [n_k, H, W, 3]."""

    dtype = np.uint8

    @staticmethod
    def _check_item(a) -> None:
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
            raise ValueError("images must be grey [H,W] or RGB [H,W,3] uint8 arrays")

    @staticmethod
    def _upload(dev, items):
        return dev.to_device(np.stack([np.ascontiguousarray(a, dtype=np.uint8) for a in items]))
