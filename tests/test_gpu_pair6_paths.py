"""`gpu`: the per-channel paths of the six-wave pair kernel (pair6_path_cases.py) on an MI355X through the C ABI: live-channel
lists of every length and pattern, the Nyquist column, the workgroup tiling (a gallery count past a 16-item tile included), the
four forms - against the float64 oracle."""

import pytest

import pair6_path_cases as p6

pytestmark = pytest.mark.gpu

_FORMS = [c for c in p6.CASES if c.forms]


@pytest.fixture(scope="module")
def scorer():
    from shoeprint_image_retrieval_amd import _lib
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    lib = _lib.load_library()  # raises if the in-tree .so is missing: no fallback
    return lambda method: NccScorer(method=method, library=lib)


@pytest.mark.parametrize("case", p6.CASES, ids=p6.IDS(p6.CASES))
def test_pair6_scores(scorer, case):
    p6.check_plain(scorer, case)


@pytest.mark.parametrize("case", _FORMS, ids=p6.IDS(_FORMS))
def test_pair6_forms(scorer, case):
    p6.check_forms(scorer, case)
