"""`not gpu`: the per-channel paths of the six-wave pair kernel (pair6_path_cases.py) on the CPU emulation of the kernels:
live-channel lists of every length and pattern, the Nyquist column, the workgroup tiling, the four forms - against the float64
oracle, and bit for bit against the scores the parent commit's kernel gave on the same seeds."""

import pytest

import pair6_path_cases as p6
from emu_util import emu_scorer

_FORMS = [c for c in p6.EMU_CASES if c.forms]


@pytest.mark.parametrize("case", p6.EMU_CASES, ids=p6.IDS(p6.EMU_CASES))
def test_emu_pair6_scores(case):
    got = p6.check_plain(emu_scorer, case)
    p6.check_against_parent(case, got)


@pytest.mark.parametrize("case", _FORMS, ids=p6.IDS(_FORMS))
def test_emu_pair6_forms(case):
    p6.check_forms(emu_scorer, case)


def test_emu_pair6_golden_names_its_parent():
    z, commit = p6.golden()
    assert len(commit) == 40 and int(commit, 16) >= 0
    assert {k[:-7] for k in z.files if k.endswith("_scores")} == {c.name for c in p6.EMU_CASES}
