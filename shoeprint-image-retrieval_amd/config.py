"""run.toml loader with the reference's schema (config.py:11-64) plus an optional ``[mi355x]`` table.

The reference reads the file with the ``toml`` package; ``tomli`` (same TOML 1.0 grammar) is what
this image ships.  As in the reference, ``rotations = ""`` / ``scales = ""`` mean "none"
(config.py:60-63).  Reference files stay valid: keys under ``[mi355x]`` are build-only extras
(``dtype``, ``ncc_method``, ``max_prepared_gib``, ``weights``, ``shortlist``, ``device_resize``, ``matrix_core_peaks``, ``device_resident``, ``cascade_blocks`` ...) and all have defaults.
"""

from __future__ import annotations

from pathlib import Path
from typing import Any, TypedDict

import tomli


class DatasetConfig(TypedDict, total=True):
    dir: str
    type: str
    crop: list[float]
    n_processes: int
    n_clusters: int
    cluster_minimise_tolerance: float


class ModelConfig(TypedDict, total=True):
    type: str
    clahe_clip_limit: float
    clahe_tile_grid_size: list[int]
    start_block: int
    end_block: int
    skip_blocks: list[int]
    minimum_dim: int
    maximum_dim: int


class ComparisonConfig(TypedDict, total=True):
    n_processes: int
    rotations: list[int] | None
    scales: list[float] | None


class Mi355xConfig(TypedDict, total=False):
    dtype: str
    ncc_method: str
    max_prepared_gib: float
    f32_matrix_cores: bool  # with ncc_method "auto": float32 plans the "mfma_f32" method covers run on the bf16 matrix cores
    matrix_core_peaks: bool  # plans of the matrix-core methods take the arg-max in the scoring pass (spr_ncc_plan_enable_peaks)
    weights: str
    gallery_cache: str  # directory for persisted gallery features (feature_cache.py); "" = off
    extractor_dtype: str  # "float32" (the reference's arithmetic) | "bfloat16" | "float16": compute type of the extractor
    shortlist: int  # 1 .. 256: run_mi355x.py also prints, per query, that many best gallery prints with variant and offset
    device_resize: bool  # the loader's crop + LANCZOS resize of "L" / "RGB" images runs on the device (image_resize.py)
    max_decoded_gib: float  # with device_resize: decoded gallery images kept in device memory between clusters, at most
    device_resident: bool  # images (with device_resize), features and scores stay in device memory from the loader to the ranks
    max_feature_gib: float  # with device_resident: a cluster whose query + gallery features exceed it takes the host route
    fuse_blocks: list[int]  # slice ends below a cluster's block whose score matrices are fused with the block's (mean); [] = off
    cascade_blocks: list[int]  # slice ends below a cluster's block that re-rank the block's cascade_depth best prints; [] = off
    cascade_depth: int  # 1 .. 256: candidates per query the cascade keeps from its coarse layer


class Config(TypedDict, total=False):
    dataset: DatasetConfig
    model: ModelConfig
    comparison: ComparisonConfig
    mi355x: Mi355xConfig


MI355X_DEFAULTS: dict[str, Any] = {"dtype": "float32", "ncc_method": "auto", "max_prepared_gib": 0.0, "weights": "",
                                   "gallery_cache": "", "extractor_dtype": "float32", "f32_matrix_cores": False,
                                   "shortlist": 0, "device_resize": False, "max_decoded_gib": 8.0,
                                   "matrix_core_peaks": False, "device_resident": False, "max_feature_gib": 64.0,
                                   "fuse_blocks": [], "cascade_blocks": [], "cascade_depth": 100}


def normalise(raw: dict) -> Config:
    comp = raw.setdefault("comparison", {})
    for key in ("rotations", "scales"):
        if comp.get(key, "") == "":
            comp[key] = None
    extra = dict(MI355X_DEFAULTS)
    extra.update(raw.get("mi355x", {}))
    shortlist = extra["shortlist"]
    if isinstance(shortlist, bool) or not isinstance(shortlist, int) or not 0 <= shortlist <= 256:
        raise ValueError(f"[mi355x].shortlist = {shortlist!r}: expected an integer in [0, 256] (0 = off)")
    if not isinstance(extra["device_resize"], bool):
        raise ValueError(f"[mi355x].device_resize = {extra['device_resize']!r}: expected true or false")
    if not isinstance(extra["matrix_core_peaks"], bool):
        raise ValueError(f"[mi355x].matrix_core_peaks = {extra['matrix_core_peaks']!r}: expected true or false")
    if not isinstance(extra["device_resident"], bool):
        raise ValueError(f"[mi355x].device_resident = {extra['device_resident']!r}: expected true or false")
    ceiling = extra["max_feature_gib"]
    if isinstance(ceiling, bool) or not isinstance(ceiling, (int, float)) or ceiling < 0:
        raise ValueError(f"[mi355x].max_feature_gib = {ceiling!r}: expected a number of GiB >= 0 (0 = always the host route)")
    budget = extra["max_decoded_gib"]
    if isinstance(budget, bool) or not isinstance(budget, (int, float)) or budget < 0:
        raise ValueError(f"[mi355x].max_decoded_gib = {budget!r}: expected a number of GiB >= 0 (0 = keep nothing)")
    fuse = extra["fuse_blocks"]
    if not isinstance(fuse, list) or any(isinstance(t, bool) or not isinstance(t, int) for t in fuse):
        raise ValueError(f"[mi355x].fuse_blocks = {fuse!r}: expected a list of integers ([] = off)")
    cascade, depth = extra["cascade_blocks"], extra["cascade_depth"]
    if not isinstance(cascade, list) or any(isinstance(t, bool) or not isinstance(t, int) for t in cascade):
        raise ValueError(f"[mi355x].cascade_blocks = {cascade!r}: expected a list of integers ([] = off)")
    if isinstance(depth, bool) or not isinstance(depth, int) or not 1 <= depth <= 256:
        raise ValueError(f"[mi355x].cascade_depth = {depth!r}: expected an integer in [1, 256]")
    for name, taps in (("fuse_blocks", fuse), ("cascade_blocks", cascade)):
        if not taps:
            continue
        from .network import tap_ends  # (the table of slice ends per backbone; nothing is loaded or built)

        try:
            accepted = tap_ends(str(raw.get("model", {}).get("type", "")))
        except LookupError:
            accepted = None  # (Model raises the reference's LookupError for the type itself)
        bad = [t for t in taps if accepted is not None and t not in accepted]
        if bad:
            raise ValueError(f"[mi355x].{name} = {taps!r}: {bad} are not feature taps of {raw['model']['type']} "
                             f"(slice ends {accepted})")
    if cascade:
        if fuse:
            raise ValueError("[mi355x].cascade_blocks with fuse_blocks: a cluster is either fused over the whole gallery or "
                             "re-ranked on its best candidates")
        if extra["gallery_cache"]:
            raise ValueError("[mi355x].cascade_blocks with gallery_cache: cached galleries hold one layer")
        if shortlist > depth:
            raise ValueError(f"[mi355x].cascade_depth = {depth} with shortlist = {shortlist}: the cascade re-ranks cascade_depth "
                             "candidates per query and has no more than those to list")
    if fuse:
        if shortlist > 0:
            raise ValueError("[mi355x].fuse_blocks with shortlist > 0: located peaks are per layer, a shortlist on the fused "
                             "score is not built")
        if extra["gallery_cache"]:
            raise ValueError("[mi355x].fuse_blocks with gallery_cache: cached galleries hold one layer")
    raw["mi355x"] = extra
    return raw  # type: ignore[return-value]


def load_config(config_file: Path | str) -> Config:
    with Path(config_file).open("rb") as fh:
        return normalise(tomli.load(fh))
