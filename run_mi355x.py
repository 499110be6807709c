#!/usr/bin/env python3
"""Run shoeprint image retrieval on MI355X — the reference's ``run.py`` (run.py:1-34) on this package.

    python run_mi355x.py [run.toml]

Same flow: load the config, iterate the size clusters of the query set, extract features of the queries and
of the whole gallery with the truncated network chosen for the cluster, rank every query's true match, print
the S-scores of that cluster against the whole-data-set totals.  Additionally prints rank-1 and mAP over all
clusters at the end.  With ``[mi355x] shortlist = K`` it also prints, under every query's rank line, the K best gallery
prints with score, best query variant and the offset at which the mark lies on the print.  With ``[mi355x] device_resident = true``
features and scores stay in device memory from the extractor to the ranks (features.FeatureSet): per cluster only the rank vector
and the shortlist come back, the printed output and the ranks are the same.  With ``[mi355x] fuse_blocks = [..]`` (default []: off)
a cluster whose block is b is scored on the feature layers {t in fuse_blocks : t < b} and b - one tapped extractor pass, one score
matrix per layer, their mean on the device (``fused_ranks``); not together with ``shortlist`` or ``gallery_cache``.
With ``[mi355x] cascade_blocks = [..]`` (default []: off) such a cluster is ranked coarse to fine instead (``cascade_ranks``): the
block b is scored against the whole gallery, its ``cascade_depth`` best prints per query are scored on the layers
{t in cascade_blocks : t < b} as a list of pairs and re-ranked by the mean over all layers; ``shortlist`` lists the re-ranked prints.
"""

import os
import sys

from shoeprint_image_retrieval_amd.config import load_config
from shoeprint_image_retrieval_amd import feature_cache
from shoeprint_image_retrieval_amd.dataloader import Dataloader
from shoeprint_image_retrieval_amd.features import DeviceImages, FeatureSet
from shoeprint_image_retrieval_amd.network import Model
from shoeprint_image_retrieval_amd.parse_results import cmp_all, mean_average_precision, rank1
from shoeprint_image_retrieval_amd.similarity import (compare_maps, retrieve_cascade, retrieve_resident, retrieve_with_scores,
                                                      scorer_from_config)
from shoeprint_image_retrieval_amd.variants import variant_labels


def ranks_with_shortlist(shoemark_features, shoeprint_features, matching_shoeprint_ids, config, gallery_files, k):
    """compare_maps(..., progress=True) from ONE score matrix that also feeds the shortlist of retrieve(): the same rank line per query,
    followed by its k best gallery prints."""
    comp = config["comparison"]
    scorer = scorer_from_config(config)
    if isinstance(shoemark_features, FeatureSet) and isinstance(shoeprint_features, FeatureSet):
        scores, short = retrieve_resident(shoemark_features, shoeprint_features, config, k, scorer=scorer)
        ranks = scorer.ranks_of_device(scores, matching_shoeprint_ids)  # (the matrix stays where it is)
    else:
        scores, short = retrieve_with_scores(shoemark_features, shoeprint_features, config, k, scorer=scorer)
        ranks = scorer.ranks(scores, matching_shoeprint_ids)
    labels = variant_labels(comp.get("rotations"), comp.get("scales"))
    for i, r in enumerate(ranks):
        print(f"Print {i} true match ranked {r}")
        for p, g in enumerate(short.index[i]):
            if g < 0:
                break
            dy, dx = short.offset[i, p]
            print(f"    {p + 1}. {gallery_files[g]}  score {short.score[i, p]:.4f}  {labels[short.variant[i, p]]}  "
                  f"offset ({dy}, {dx})")
    return ranks


def feature_bytes(model, *image_sets) -> int:
    """Bytes of the float32 features ``model`` makes of the images (host lists or DeviceImages), from their shapes alone."""
    total = 0
    for images in image_sets:
        shapes = [(s, len(idx)) for s, idx, _ in images.classes] if isinstance(images, DeviceImages) else [(im.shape, 1) for im in images]
        sizes = {}
        for shape, n in shapes:
            if shape[:2] not in sizes:
                c, h, w = model.output_shape(shape[0], shape[1])
                sizes[shape[:2]] = 4 * c * h * w
            total += n * sizes[shape[:2]]
    return total


def _host_images(images):
    return images.to_host_list() if isinstance(images, DeviceImages) else images


def fused_ranks(model, layers, shoemark_images, shoeprint_images, matching_shoeprint_ids, config):
    """[mi355x] fuse_blocks: one tapped extractor pass per image batch hands out the feature layers ``layers`` (slice ends,
    the model's block last), every layer is scored as usual (the maximum over the query variants) and the cluster's score is
    the mean of the layers' matrices; features and scores stay in device memory, the rank vector comes back."""
    comp = config["comparison"]
    scorer = scorer_from_config(config)
    shoemark_sets = model.get_multiple_feature_maps_device(shoemark_images, taps=layers)
    shoeprint_sets = model.get_multiple_feature_maps_device(shoeprint_images, taps=layers)
    print("Calculating ranks:")
    scores = scorer.multi_layer_score_matrix_device(list(zip(shoemark_sets, shoeprint_sets)), rotations=comp.get("rotations"),
                                                    scales=comp.get("scales"))
    ranks = scorer.ranks_of_device(scores, matching_shoeprint_ids)
    for i, r in enumerate(ranks):
        print(f"Print {i} true match ranked {r}")
    return ranks


def cascade_ranks(model, layers, shoemark_images, shoeprint_images, matching_shoeprint_ids, config, gallery_files, k):
    """[mi355x] cascade_blocks: one tapped extractor pass per image batch hands out the feature layers ``layers`` (slice ends,
    the model's block last); the block is the coarse layer of ``retrieve_cascade``, the layers below it re-rank its
    ``cascade_depth`` best prints per query.  Prints the rank line per query and, with ``k`` > 0, its k best prints by the
    fused score, variant and offset from the finest layer."""
    comp = config["comparison"]
    scorer = scorer_from_config(config)
    shoemark_sets = model.get_multiple_feature_maps_device(shoemark_images, taps=layers)
    shoeprint_sets = model.get_multiple_feature_maps_device(shoeprint_images, taps=layers)
    print("Calculating ranks:")
    cascade = retrieve_cascade(list(zip(shoemark_sets, shoeprint_sets)), config, int(config["mi355x"]["cascade_depth"]), coarse=-1,
                               scorer=scorer)
    ranks = cascade.ranks(matching_shoeprint_ids)
    labels = variant_labels(comp.get("rotations"), comp.get("scales"))
    for i, r in enumerate(ranks):
        print(f"Print {i} true match ranked {r}")
        for p, g in enumerate(cascade.index[i, :k]):
            if g < 0:
                break
            dy, dx = cascade.offset[i, p]
            v = cascade.variant[i, p]
            print(f"    {p + 1}. {gallery_files[g]}  score {cascade.score[i, p]:.4f}  {labels[v] if v >= 0 else 'no variant'}  "
                  f"offset ({dy}, {dx})")
    return ranks


def main(config_file: str = "run.toml") -> list[int]:
    config = load_config(config_file)
    dataloader = Dataloader(config)
    print(f"{dataloader.num_clusters} clusters of image sizes found.")
    all_ranks: list[int] = []
    cache_dir = config["mi355x"].get("gallery_cache", "")
    for cluster, (shoemark_images, shoeprint_images, matching_shoeprint_ids, block) in enumerate(dataloader):
        print(f"Cluster has {len(shoemark_images)} items.")
        model = Model(config, block)
        fuse = config["mi355x"].get("fuse_blocks") or []
        if fuse:
            layers = sorted({t for t in fuse if t < block} | {block})
            print(f"Scoring the feature layers {layers} of features[:{block}].")
            ranks = fused_ranks(model, layers, shoemark_images, shoeprint_images, matching_shoeprint_ids, config)
            cmp_all(list(ranks), total_shoeprints=len(dataloader.shoeprint_files), total_shoemarks=len(dataloader.shoemark_files))
            all_ranks += [int(r) for r in ranks]
            continue
        fine = sorted({t for t in (config["mi355x"].get("cascade_blocks") or []) if t < block})
        if fine:
            depth = int(config["mi355x"]["cascade_depth"])
            print(f"Cascade: features[:{block}] ranks the gallery, its {depth} best prints per query are re-ranked on the "
                  f"feature layers {fine + [block]}.")
            ranks = cascade_ranks(model, fine + [block], shoemark_images, shoeprint_images, matching_shoeprint_ids, config,
                                  sorted(dataloader.shoeprint_files), int(config["mi355x"].get("shortlist", 0) or 0))
            cmp_all(list(ranks), total_shoeprints=len(dataloader.shoeprint_files), total_shoemarks=len(dataloader.shoemark_files))
            all_ranks += [int(r) for r in ranks]
            continue
        resident = bool(config["mi355x"].get("device_resident", False))
        if resident:
            need, ceiling = feature_bytes(model, shoemark_images, shoeprint_images), float(config["mi355x"].get("max_feature_gib", 64.0))
            if need > ceiling * (1 << 30):
                print(f"cluster {cluster}: {need / (1 << 30):.2f} GiB of features exceed [mi355x].max_feature_gib = {ceiling:g}: "
                      "this cluster takes the host route", file=sys.stderr)
                resident = False
        if not resident:
            shoemark_images, shoeprint_images = _host_images(shoemark_images), _host_images(shoeprint_images)
        extract = model.get_multiple_feature_maps_device if resident else model.get_multiple_feature_maps
        shoemark_features = extract(shoemark_images)
        # gallery features depend only on what is in `key`: keep them across runs when [mi355x].gallery_cache is set
        key = {"files": dataloader.shoeprint_files, "scale": dataloader.scales[cluster], "block": block,
               "crop": list(config["dataset"]["crop"]), "model": dict(config["model"]),
               "weights": config["mi355x"].get("weights", ""),
               "extractor_dtype": config["mi355x"].get("extractor_dtype", "float32")}
        path = os.path.join(cache_dir, f"gallery_block{block}_cluster{cluster}.f32") if cache_dir else ""
        shoeprint_features = feature_cache.load_features(path, key) if path else None
        if shoeprint_features is None:
            shoeprint_features = extract(shoeprint_images)
            if path:
                os.makedirs(cache_dir, exist_ok=True)  # (a resident gallery comes down once, to be written)
                feature_cache.save_features(path, shoeprint_features.to_host_list() if resident else shoeprint_features, key)
        else:
            print(f"Gallery features from {path}")
            if resident:
                shoeprint_features = FeatureSet.from_host(model.dev, shoeprint_features)
        print("Calculating ranks:")
        shortlist = int(config["mi355x"].get("shortlist", 0) or 0)
        if shortlist > 0:
            ranks = ranks_with_shortlist(shoemark_features, shoeprint_features, matching_shoeprint_ids, config,
                                         sorted(dataloader.shoeprint_files), shortlist)
        else:
            ranks = compare_maps(shoemark_features, shoeprint_features, matching_shoeprint_ids, config, progress=True)
        cmp_all(list(ranks), total_shoeprints=len(dataloader.shoeprint_files),
                total_shoemarks=len(dataloader.shoemark_files))
        all_ranks += [int(r) for r in ranks]
    if all_ranks:
        print(f"rank-1: {rank1(all_ranks):.4f}  mAP: {mean_average_precision(all_ranks):.4f}  ({len(all_ranks)} queries)")
    return all_ranks


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "run.toml")
