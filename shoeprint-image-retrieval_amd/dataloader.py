"""Dataset loading: size clustering, scale / block selection, crop, resize, id parsing.

Host-side mirror of the reference's ``dataloader.py`` (``Dataloader(config)`` is an iterator over size
clusters of the query images; each step yields ``(query images, ALL gallery images at the cluster's scale,
gallery index of every query's true match, network block)`` — dataloader.py:26-113).  This is CPU I/O that
runs once per image; it uses Pillow like the reference does.  The crop + LANCZOS resize, which runs
once per image *per cluster*, can run on the device instead (``[mi355x] device_resize``, see ``Dataloader``).

Behaviour kept from the reference because it decides the scale and block (and therefore the ranks):
  * "Algorithm 1" scale / block search incl. its asymmetric skip-block loops       (dataloader.py:366-419)
  * cluster merging by |scale difference| <= tolerance and equal block               (:314-362)
  * ``_image_extremes``: Pillow's ``size`` is (width, height) but is unpacked as (height, width), so the two
    crop ratios are applied to the opposite axes, and the ``elif`` lets one image update only one extreme (:446-464)
  * crop box from floor(size*ratio), resize to int(size*scale) with LANCZOS            (:217-237)
  * ids: WVU2019 = first 3 characters, Impress = before the first "_" / ".", FID-300 = stem + label_table.csv (:245-250, 101-107)
Deliberate differences:
  * K-means is seeded (``random_state=0``; the reference's is unseeded, dataloader.py:284); clusters are
    reported in order of first appearance in the directory listing, as the reference's dict does.
  * the directory listing is sorted before clustering (``os.listdir`` order is file-system dependent).
  * images are loaded by a thread pool over correct chunks: the reference's chunking drops or mis-sizes items
    unless ``len(files) % n_processes == 0`` and then papers over it (:143, :178-181).
"""

from __future__ import annotations

import csv
import os
from concurrent.futures import ThreadPoolExecutor
from math import floor
from pathlib import Path
from typing import Any

import numpy as np
from PIL import Image


_CHUNK_IMAGES = 64  # decoded images per device resize call ([mi355x] device_resize)


class Dataloader:
    """Initialise, pre-process and provide access to datasets (reference dataloader.py:26-113).

    ``[mi355x] device_resize = true``: files are decoded by the thread pool as before, and the crop + LANCZOS resize of
    mode-"L" and mode-"RGB" images runs on the device (image_resize.DeviceResizer, byte-identical to Pillow), one call per
    chunk of images; every other mode goes through Pillow per image.  The decoded gallery stays in device memory, up to
    ``[mi355x] max_decoded_gib``, so later clusters - which resize the whole gallery again at their own scale - neither read
    nor decode its files again.  ``resizer``: the DeviceResizer to use (default: one on the current GPU).

    ``[mi355x] device_resident = true`` on top of that: a step yields ``features.DeviceImages`` instead of the two lists -
    per output shape one dense uint8 batch in device memory, which the resize calls write directly - so the images are
    not copied back (``to_host_list()`` gives the lists, byte for byte)."""

    def __init__(self, config: dict, resizer=None) -> None:
        self.config = config
        extra = config.get("mi355x", {})
        self._device_resize = bool(extra.get("device_resize", False))
        self._resizer = resizer
        self._device_resident = self._device_resize and bool(extra.get("device_resident", False))
        if self._device_resize and resizer is None:
            from .image_resize import DeviceResizer

            self._resizer = DeviceResizer()  # raises without a GPU or the library: no fallback
        self._decoded_budget = int(float(extra.get("max_decoded_gib", 8.0)) * (1 << 30))
        self._decoded_bytes = 0
        self._kept: dict[tuple[str, int], Any] = {}  # (directory, chunk) -> decoded chunk resident on the device
        self.dataset_dir = Path(config["dataset"]["dir"])
        self.shoeprint_dir = self.dataset_dir / "Gallery"
        self.shoemark_dir = self.dataset_dir / "Query"
        self.shoeprint_files = sorted(os.listdir(self.shoeprint_dir))
        self.shoemark_files = sorted(os.listdir(self.shoemark_dir))
        print("The dataset contains: \n", f"    {len(self.shoeprint_files)} reference shoeprints\n",
              f"    {len(self.shoemark_files)} shoemarks")
        clustered = self._cluster_images_by_size(self.shoemark_dir, config["dataset"]["n_clusters"])
        self.scales, self.blocks, self.clusters = self._minimise_clusters(clustered)
        self.num_clusters = len(self.clusters)
        self._current_cluster = 0

    def __iter__(self):
        return self

    def __next__(self) -> tuple[list[np.ndarray], list[np.ndarray], list[int], int]:
        if self._current_cluster >= self.num_clusters:
            raise StopIteration
        scale = self.scales[self._current_cluster]
        shoemark_images, shoemark_ids = self._load_images(self.clusters[self._current_cluster], self.shoemark_dir, scale)
        shoeprint_images, shoeprint_ids = self._load_images(self.shoeprint_files, self.shoeprint_dir, scale, keep=True)
        if self.config["dataset"]["type"] != "FID-300":
            # ValueError if a query's id has no gallery item, as list.index does in the reference (:99)
            matching_pairs = [shoeprint_ids.index(i) for i in shoemark_ids]
        else:
            table: dict[int, int] = {}
            with (self.dataset_dir / "label_table.csv").open() as fh:
                for row in csv.reader(fh):
                    table[int(row[0])] = int(row[1])
            matching_pairs = [table[i] - 1 for i in shoemark_ids]
        block = self.blocks[self._current_cluster]
        self._current_cluster += 1
        return shoemark_images, shoeprint_images, matching_pairs, block

    # ------------------------------------------------------------------ loading
    def _load_images(self, image_files: list[str], image_directory: Path, scale: float, keep: bool = False):
        files = sorted(image_files)
        crop = self.config["dataset"]["crop"]
        kind = self.config["dataset"]["type"]
        workers = max(1, min(int(self.config["dataset"].get("n_processes", 1)), len(files) or 1))
        with ThreadPoolExecutor(workers) as pool:
            if self._device_resize:
                return self._load_images_device(pool, files, image_directory, scale, crop, kind, keep)
            loaded = list(pool.map(lambda f: _load_one(image_directory / f, f, scale, crop, kind), files))
        return [im for im, _ in loaded], [i for _, i in loaded]

    def _load_images_device(self, pool, files, directory: Path, scale: float, crop, kind: str, keep: bool):
        """``keep``: the directory is loaded again by every cluster (the gallery): its decoded chunks stay on the device
        while they fit the budget."""
        from .image_resize import crop_box

        idents = [_parse_id(f, kind) for f in files]
        if self._device_resident:
            return self._load_images_resident(pool, files, directory, scale, crop, kind, keep), idents
        images: list[Any] = [None] * len(files)
        for c, start in enumerate(range(0, len(files), _CHUNK_IMAGES)):
            names = files[start: start + _CHUNK_IMAGES]
            chunk = self._chunk(pool, directory, names, (str(directory), c), keep)
            for where, resident in chunk.groups:
                boxes = [crop_box(w, h, crop) for h, w in resident.shapes]
                sizes = [(int(b[2] * scale), int(b[3] * scale)) for b in boxes]
                for k, out in zip(where, self._resizer.resize_resident(resident, boxes, sizes)):
                    images[start + k] = out
            others = list(pool.map(lambda k: _load_one(directory / names[k], names[k], scale, crop, kind)[0], chunk.others))
            for k, out in zip(chunk.others, others):
                images[start + k] = out
        return images, idents

    def _chunk(self, pool, directory: Path, names, key, keep: bool):
        chunk = self._kept.get(key) if keep else None
        if chunk is None:
            decoded = list(pool.map(lambda f: _decode_image(directory / f), names))
            chunk = _DecodedChunk(self._resizer, decoded)
            if keep and self._decoded_bytes + chunk.nbytes <= self._decoded_budget:
                self._kept[key] = chunk
                self._decoded_bytes += chunk.nbytes
        return chunk

    def _load_images_resident(self, pool, files, directory: Path, scale: float, crop, kind: str, keep: bool):
        """The directory as ``features.DeviceImages``.  Output shapes are known from the files' headers (other modes: from
        what Pillow made of them), so every shape class is allocated once and each resize call - one per (chunk, mode,
        class) - writes its images into their rows; images of other modes are resized by Pillow as ever, uploaded, and
        copied into their rows by the same kernels (a resize to the same size is a copy)."""
        from .features import DeviceImages
        from .image_resize import crop_box

        dev = self._resizer.dev

        def header(name):
            with Image.open(directory / name) as image:
                if image.mode not in ("L", "RGB"):
                    return None
                w, h = image.size
            box = crop_box(w, h, crop)
            ow, oh = int(box[2] * scale), int(box[3] * scale)
            if ow < 1 or oh < 1:
                raise ValueError("height and width must be > 0")  # Pillow's message for an empty target size
            return (oh, ow) if image.mode == "L" else (oh, ow, 3)

        shapes = list(pool.map(header, files))
        other = {k: np.ascontiguousarray(_load_one(directory / files[k], files[k], scale, crop, kind)[0], dtype=np.uint8)
                 for k, s in enumerate(shapes) if s is None}
        for k, a in other.items():
            DeviceImages._check_item(a)
            shapes[k] = tuple(a.shape)
        members: dict[tuple, list[int]] = {}
        for k, s in enumerate(shapes):
            members.setdefault(s, []).append(k)
        batches = {s: dev.empty((len(idx),) + s, np.uint8) for s, idx in members.items()}
        row = {k: r for idx in members.values() for r, k in enumerate(idx)}

        def resize_into(resident, positions, boxes, sizes):
            """``positions[i]``: the file that image i of ``resident`` is; one call per shape class among them."""
            by_class: dict[tuple, list[int]] = {}
            for i, k in enumerate(positions):
                by_class.setdefault(shapes[k], []).append(i)
            for s, select in by_class.items():
                item = int(np.prod(s))
                plan = self._resizer.plan(resident, boxes, sizes, select, [row[positions[i]] * item for i in select])
                self._resizer.run(plan, resident, out=batches[s])

        for c, start in enumerate(range(0, len(files), _CHUNK_IMAGES)):
            chunk = self._chunk(pool, directory, files[start: start + _CHUNK_IMAGES], (str(directory), c), keep)
            for where, resident in chunk.groups:
                boxes = [crop_box(w, h, crop) for h, w in resident.shapes]
                sizes = [(int(b[2] * scale), int(b[3] * scale)) for b in boxes]
                resize_into(resident, [start + k for k in where], boxes, sizes)
        for ndim in (2, 3):
            where = [k for k, a in other.items() if a.ndim == ndim]
            if where:
                resident = self._resizer.upload([other[k] for k in where])
                whole = [(0, 0, w, h) for h, w in resident.shapes]
                resize_into(resident, where, whole, [(b[2], b[3]) for b in whole])
        return DeviceImages(dev, len(files), [(s, idx, batches[s]) for s, idx in members.items()])

    # ------------------------------------------------------------------ clustering
    def _cluster_images_by_size(self, image_dir: Path, n_clusters: int) -> dict[int, list[str]]:
        from sklearn.cluster import KMeans

        sizes, names = [], []
        for name in sorted(os.listdir(image_dir)):
            with Image.open(image_dir / name) as im:
                width, height = im.size
            sizes.append([min(width, height)])  # group by the smallest image dimension (:275-279)
            names.append(name)
        labels = KMeans(n_clusters=n_clusters, random_state=0, n_init=10).fit(sizes).labels_
        clusters: dict[int, list[str]] = {}
        for name, label in zip(names, labels):
            clusters.setdefault(int(label), []).append(name)
        return clusters

    def _minimise_clusters(self, clusters: dict[int, list[str]]):
        tolerance = self.config["dataset"]["cluster_minimise_tolerance"]
        scales: list[float] = []
        blocks: list[int] = []
        groups: list[list[str]] = []
        largest_print, smallest_print = self._image_extremes(self.shoeprint_files, self.shoeprint_dir)
        for files in clusters.values():
            largest_mark, smallest_mark = self._image_extremes(files, self.shoemark_dir)
            smallest_dim = min(smallest_mark[1], smallest_print[1])
            largest_dim = max(largest_mark[1], largest_print[1])
            scale, block = self._find_best_scale(smallest_dim, largest_dim, minimum_dim=self.config["model"]["minimum_dim"],
                                                 block=self.config["model"]["start_block"])
            for index, other in enumerate(scales):  # first selected scale within the tolerance (:314-319)
                if abs(scale - other) <= tolerance:
                    if blocks[index] == block:
                        groups[index] += files
                    else:
                        scales.append(scale); blocks.append(block); groups.append(list(files))
                    break
            else:
                scales.append(scale); blocks.append(block); groups.append(list(files))
        return scales, blocks, groups

    def _find_best_scale(self, smallest_dim: int, largest_dim: int, minimum_dim: int, block: int) -> tuple[float, int]:
        """Ideal input scale and network block ("Algorithm 1 of the paper", dataloader.py:366-419)."""
        maximum_dim = self.config["model"]["maximum_dim"]
        end_block = self.config["model"]["end_block"]
        skip_blocks = self.config["model"]["skip_blocks"]
        scale: float = 1
        if smallest_dim < minimum_dim:
            if block > end_block:
                block -= 1
                while block in skip_blocks:
                    block -= 1
                return self._find_best_scale(smallest_dim, largest_dim, int(minimum_dim / 2), block)
            return 1, block
        if largest_dim > maximum_dim:
            scale = maximum_dim / largest_dim
            if smallest_dim * scale < minimum_dim:
                if block > end_block:
                    block -= 1
                    while block in skip_blocks and block != end_block:
                        block -= 1
                else:
                    scale = minimum_dim / smallest_dim
        return scale, block

    def _image_extremes(self, image_files: list[str], image_directory: Path):
        """((largest name, largest dim), (smallest name, smallest dim)) after cropping — with the reference's
        axis swap and one-update-per-image rule (see the module docstring)."""
        crop = self.config["dataset"]["crop"]
        largest_dim, largest_name = 0, ""
        smallest_dim, smallest_name = 2**31 - 1, ""
        for name in image_files:
            with Image.open(image_directory / name) as im:
                height, width = im.size  # sic: Pillow returns (width, height)
            height -= floor(height * crop[0] * 2)
            width -= floor(width * crop[1] * 2)
            big, small = max(width, height), min(width, height)
            if big > largest_dim:
                largest_name, largest_dim = name, big
            elif small < smallest_dim:
                smallest_name, smallest_dim = name, small
        return (largest_name, largest_dim), (smallest_name, smallest_dim)


def _load_one(path: Path, name: str, scale: float, crop, dataset_type: str) -> tuple[np.ndarray, int]:
    with Image.open(path) as image:
        crop_height = floor(image.height * crop[0])
        crop_width = floor(image.width * crop[1])
        image = image.crop((crop_width, crop_height, image.width - crop_width, image.height - crop_height))
        resized = image.resize((int(image.width * scale), int(image.height * scale)), Image.Resampling.LANCZOS)
        array = np.array(resized)
    return array, _parse_id(name, dataset_type)


def _decode_image(path: Path) -> np.ndarray | None:
    """The decoded pixels of a mode-"L" ([h, w]) or mode-"RGB" ([h, w, 3]) file; None for any other mode, which Pillow
    resizes by rules of its own (NEAREST for "1" and "P", premultiplied alpha, 16-bit and float arithmetic)."""
    with Image.open(path) as image:
        if image.mode not in ("L", "RGB"):
            return None
        return np.array(image)


class _DecodedChunk:
    """One chunk of a directory, decoded: the "L" and the "RGB" images each packed into a device buffer (``groups``: positions
    in the chunk and the resident images), and the positions of the files of other modes."""

    def __init__(self, resizer, decoded: list):
        self.others = [k for k, a in enumerate(decoded) if a is None]
        self.groups = []
        self.nbytes = 0
        for ndim in (2, 3):
            where = [k for k, a in enumerate(decoded) if a is not None and a.ndim == ndim]
            if where:
                resident = resizer.upload([decoded[k] for k in where])
                self.groups.append((where, resident))
                self.nbytes += resident.nbytes


def _parse_id(name: str, dataset_type: str) -> int:
    if dataset_type == "Impress":
        ident = int(name.split("_")[0].split(".")[0])
    elif dataset_type == "WVU2019":
        ident = int(name[:3])
    elif dataset_type == "FID-300":
        ident = int(name[:-4])
    else:
        raise ValueError(f"unknown dataset type {dataset_type!r} (FID-300, Impress or WVU2019)")
    return ident
