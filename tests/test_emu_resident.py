"""`not gpu`: the device-resident route (csrc/resident.hip, features.py, the scorer's and the extractor's resident forms, the
loader's DeviceImages) on the CPU-emulation build - the checks of resident_cases.py, which tests/test_gpu_resident.py runs
through the real library."""

import pytest

import resident_cases as rc
from emu_util import emu_library, emu_scorer
from host_device import HostDevice


@pytest.fixture(scope="module")
def scorer():
    return emu_scorer("fft")


@pytest.mark.parametrize("n", sorted(rc.INDEXES))
@pytest.mark.parametrize("storage", rc.STORAGES)
@pytest.mark.parametrize("item_elems", rc.ITEM_ELEMS)
def test_emu_gather(scorer, item_elems, storage, n):
    rc.check_gather(scorer, item_elems, storage, rc.INDEXES[n])


def test_emu_gather_grid_stride(scorer):
    rc.check_gather_grid_stride(scorer)


def test_emu_gather_arguments(scorer):
    rc.check_gather_arguments(scorer)


def test_emu_scatter(scorer):
    rc.check_scatter(scorer)


def test_emu_scatter_arguments(scorer):
    rc.check_scatter_arguments(scorer)


def test_emu_feature_set(scorer):
    rc.check_feature_set(scorer)


@pytest.mark.parametrize("sides", rc.SIDES)
@pytest.mark.parametrize("method,storage", rc.METHODS[:2])
def test_emu_surface(method, storage, sides):
    rc.check_surface(emu_scorer, method, storage, sides)


@pytest.mark.parametrize("method,storage", rc.METHODS[2:])
def test_emu_surface_matrix_cores(method, storage):
    """The fused cast (bfloat16 storage) and the float32 matrix-core plans: the score matrix, FeatureSets on both sides."""
    rc.check_surface(emu_scorer, method, storage, "both", only_matrix=True)


def test_emu_resident_call_counts(monkeypatch):
    rc.check_resident_call_counts(emu_scorer, monkeypatch)


def test_emu_nothing_crosses(monkeypatch):
    rc.check_nothing_crosses(emu_scorer, monkeypatch, "fft", "float32")


@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_emu_extractor(rgb):
    rc.check_extractor(HostDevice(), emu_library(), rgb)


def test_emu_extractor_shared_feature_shape():
    rc.check_extractor_shared_feature_shape(HostDevice(), emu_library())


def _emu_resizer():
    from shoeprint_image_retrieval_amd.image_resize import DeviceResizer

    return DeviceResizer(emu_library(), HostDevice())


def _rewrite(root, convert):
    import os

    from PIL import Image

    for sub in ("Gallery", "Query"):
        for name in sorted(os.listdir(os.path.join(root, sub))):
            path = os.path.join(root, sub, name)
            with Image.open(path) as im:
                new = convert(sub, name, im.copy())
            new.save(path)


@pytest.mark.parametrize("name", ["wvu_two_sizes", "impress_uniform"])
def test_emu_loader_yields_device_images(tmp_path, name):
    import dataset_util

    case = next(c for c in dataset_util.CASES if c["name"] == name)
    rc.check_loader(dataset_util.write_dataset(str(tmp_path), case), _emu_resizer())


def test_emu_loader_rgb_and_another_mode(tmp_path):
    """An RGB directory with one palette file, which Pillow resizes (NEAREST) and the loader uploads into its class."""
    import dataset_util
    import numpy as np
    from PIL import Image

    config = dataset_util.write_dataset(str(tmp_path), dataset_util.CASES[0])
    config["model"] = dict(config["model"], maximum_dim=150)  # a downscale: NEAREST and LANCZOS differ

    def convert(sub, name, im):
        if (sub, name) == ("Gallery", "002.png"):
            return im.convert("P")
        a = np.array(im)
        return Image.fromarray(np.stack([a, 255 - a, np.roll(a, 3, axis=1)], axis=-1))

    _rewrite(str(tmp_path), convert)
    device = rc.check_loader(config, _emu_resizer())
    assert all(resident.channels == 3 for chunk in device._kept.values() for _, resident in chunk.groups)


def test_resident_config_keys():
    rc.check_config()
