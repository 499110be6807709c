"""CPU emulation: the device crop + LANCZOS resize (csrc/image_resize.hip) against Pillow, byte for byte - grey and RGB single
images (down, up, one pass skipped, copy, tiny, 181-tap windows, tile extents plus one), the loader's crop, a ragged batch
with shared tables, poison guard bands round the output and the workspace, argument errors; and the host tables alone."""

import numpy as np
import pytest

import image_resize_cases as rc
from emu_util import emu_library


@pytest.fixture(scope="module")
def resizer():
    from host_device import HostDevice

    return rc.DeviceResizer(emu_library(), HostDevice())


@pytest.mark.parametrize("channels", [1, 3], ids=["L", "RGB"])
@pytest.mark.parametrize("case", rc.SINGLE, ids=rc.SINGLE_IDS)
def test_single_image_equals_pillow(resizer, case, channels):
    h, w, scale, clamps = case
    rc.check_single(resizer, h, w, scale, channels, clamps)


@pytest.mark.parametrize("channels", [1, 3], ids=["L", "RGB"])
def test_crop_is_fused(resizer, channels):
    rc.check_crop(resizer, channels)


@pytest.mark.parametrize("channels", [1, 3], ids=["L", "RGB"])
def test_ragged_batch(resizer, channels):
    rc.check_ragged(resizer, channels)


@pytest.mark.parametrize("channels", [1, 3], ids=["L", "RGB"])
def test_guard_bands(resizer, channels):
    rc.check_guard_bands(resizer, channels)


def test_argument_errors(resizer):
    rc.check_argument_errors(resizer)


def test_tables_restate_pillow_without_the_kernels():
    """The integer scheme in numpy with lanczos_tables' coefficients equals Pillow: pins the tables apart from the kernels."""
    a = rc.image(9, 37, 52, 1)
    for size in ((19, 37), (52, 80), (23, 11)):
        cur = a
        for axis, out_size in ((1, size[0]), (0, size[1])):
            if out_size == cur.shape[axis]:
                continue
            bounds, coeffs, _ = rc.lanczos_tables(cur.shape[axis], out_size)
            src = np.moveaxis(cur, axis, 0).astype(np.int64)
            rows = [(1 << 21) + sum(int(coeffs[o, t]) * src[bounds[o, 0] + t] for t in range(bounds[o, 1])) for o in range(out_size)]
            cur = np.moveaxis(np.clip(np.stack(rows) >> 22, 0, 255).astype(np.uint8), 0, axis)
        assert np.array_equal(cur, rc.pillow(a, (0, 0, 52, 37), size)), size
