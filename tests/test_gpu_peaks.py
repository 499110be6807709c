"""`gpu`: spr_ncc_score_peaks and its host mirror through the real gfx950 library on an MI355X - the checks of peak_cases.py
(which tests/test_emu_peaks.py runs on the CPU-emulation build) and the torch op against the ctypes route."""

import numpy as np
import pytest

import ncc_map_cases as mc
import peak_cases as pc
import shortlist_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()  # raises if the in-tree .so is missing: no fallback


def _make(lib, method="fft", **kw):
    """A scorer on the ctypes route (the torch op is compared with it below)."""
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    s = NccScorer(method=method, library=lib, **kw)
    s._ops_cache = None
    return s


@pytest.fixture(scope="module")
def scorer(lib):
    return lambda method: _make(lib, method, crop=0)


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", mc.SWEEP_CASES, ids=_ids(mc.SWEEP_CASES))
def test_peaks_sweep(scorer, case, monkeypatch):
    pc.check_sweep(scorer, case, monkeypatch)


@pytest.mark.parametrize("t,i", pc.DIRECT_SWEEPS)
def test_peaks_sweep_direct(scorer, t, i, monkeypatch):
    pc.check_sweep(scorer, pc.direct_sweep_case(t, i), monkeypatch, method="direct")


@pytest.mark.parametrize("case", pc.INSTANCE_CASES, ids=_ids(pc.INSTANCE_CASES))
def test_peaks_instance(scorer, case, monkeypatch):
    pc.check_instance(scorer, case, monkeypatch)


_DIRECT = [c for c in pc.INSTANCE_CASES if c.direct and not c.env and c.method == "fft"]


@pytest.mark.parametrize("case", _DIRECT, ids=_ids(_DIRECT))
def test_peaks_instance_direct(scorer, case, monkeypatch):
    pc.check_instance(scorer, case, monkeypatch, method="direct")


MATRIX = [("fft", 0), ("fft_pow2", 0), ("direct", 0), ("fft", 1), ("fft_pow2", 1), ("direct", 1), ("fft", 2), ("fft_pow2", 2), ("direct", 2)]


@pytest.mark.parametrize("method,case", MATRIX)
def test_peaks_planted_matrix(lib, method, case):
    pc.check_planted_matrix(_make(lib, method), sc.PLANTED_CASES[case])


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_peaks_accumulate_rule(scorer, method):
    pc.check_accumulate_rule(scorer, method)


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_peaks_located_variants(lib, method):
    pc.check_located_variants(_make(lib, method))


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_peaks_ragged(lib, method):
    pc.check_ragged(_make(lib, method))


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_peaks_no_second_pass(lib, method, monkeypatch):
    pc.check_no_second_pass(_make(lib, method), monkeypatch)


def test_peaks_mfma_keeps_the_second_pass(lib, monkeypatch):
    pc.check_mfma_keeps_the_second_pass(_make(lib, "mfma", storage="bfloat16"), monkeypatch)


@pytest.mark.parametrize("method,storage,counted", pc.CALL_COUNT_SCORERS, ids=[c[0] for c in pc.CALL_COUNT_SCORERS])
def test_peaks_call_counts(lib, method, storage, counted, monkeypatch):
    pc.check_call_counts(lambda **kw: _make(lib, method, storage=storage, **kw), monkeypatch, counted)


def test_peaks_plan_has_peaks(scorer):
    pc.check_has_peaks(scorer)


@pytest.mark.parametrize("method,t,i,n", pc.EDGE_SHAPES)
def test_peaks_edges(scorer, method, t, i, n, monkeypatch):
    pc.check_edges(scorer, monkeypatch, method, t, i, n)


@pytest.mark.parametrize("method,t,i", [("fft", (9, 7), (126, 64)), ("direct", (5, 5), (16, 12))])
def test_located_op_equals_the_ctypes_route_bit_for_bit(scorer, method, t, i):
    """torch.ops.shoeprint_mi355x.ncc_scores_located on device tensors against spr_ncc_score_peaks through ctypes; a CPU
    tensor and a method without a peak form are refused."""
    import torch
    from shoeprint_image_retrieval_amd import _torch_ops

    ops = _torch_ops.load()
    assert str(ops.ncc_scores_located.default._schema) == pc.SCHEMA
    templates, items, pos, want, good = mc._sweep_inputs(t, i)
    items = items[:40]
    s = scorer(method)
    plan = s.plan(1, t, i)
    pq, pg = pc.prepare(s, plan, templates[:, None], items[:, None])
    want_s, want_yx, _ = pc.score_peaks(s, plan, pq, len(templates), pg, len(items))
    q_dev, g_dev = s.dev.to_device(np.ascontiguousarray(templates[:, None])), s.dev.to_device(np.ascontiguousarray(items[:, None]))
    got_s, got_yx = ops.ncc_scores_located(q_dev, g_dev, 0, method)
    assert got_s.dtype == torch.float32 and got_yx.dtype == torch.int32 and tuple(got_yx.shape) == (len(templates), len(items), 2)
    np.testing.assert_array_equal(pc.bits(got_s.cpu().numpy()), pc.bits(want_s))
    np.testing.assert_array_equal(got_yx.cpu().numpy(), want_yx)
    small_s, small_yx = ops.ncc_scores_located(q_dev, g_dev, 0, method, 3 * plan.gallery_item_bytes)  # gallery in chunks
    assert torch.equal(small_s.view(torch.int32), got_s.view(torch.int32)) and torch.equal(small_yx, got_yx)
    with pytest.raises(RuntimeError, match="must live in HBM"):
        ops.ncc_scores_located(torch.zeros(2, 3, 8, 6), torch.zeros(2, 3, 16, 8))
    bf = torch.zeros(2, 4, 32, 16, dtype=torch.bfloat16, device=q_dev.device)
    with pytest.raises(RuntimeError, match="keep the maximum only"):
        ops.ncc_scores_located(bf, bf, 2, "mfma")
    s.close()
