"""`gpu`: the float32 matrix-core method ("mfma_f32", SPR_NCC_MFMA_F32) on an MI355X at real widths, against the oracle on
the unrounded float32 inputs, and its rate against the FFT form - what float32 plans of these sizes run otherwise."""

import numpy as np
import pytest

import mfma_f32_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from shoeprint_image_retrieval_amd import _lib

    return _lib.load_library()


def _make_scorer(lib):
    from shoeprint_image_retrieval_amd.similarity import NccScorer

    return lambda method="auto", **kw: NccScorer(method=method, library=lib, **kw)


def test_f32_method_resolution(lib):
    fc.check_resolution(_make_scorer(lib), channels=176)


@pytest.mark.parametrize("channels,nq,ng", [(1024, 5, 3), (64, 70, 4), (17, 129, 2)])
def test_f32_equal_size(lib, channels, nq, ng):
    fc.check_equal_size(_make_scorer(lib), channels, nq, ng)


def test_f32_general_shapes(lib):
    fc.check_general_shapes(_make_scorer(lib), channels=176, nq=5, ng=6)


def test_f32_conditioning_and_degenerate_channels(lib):
    fc.check_conditioning(_make_scorer(lib), channels=64)
    fc.check_degenerate_channels(_make_scorer(lib))
    fc.check_lo_terms_needed(_make_scorer(lib), channels=64)


def test_f32_opt_in_flag_and_config(lib):
    from shoeprint_image_retrieval_amd.similarity import scorer_from_config

    fc.check_opt_in_flag(_make_scorer(lib), channels=16)
    fc.check_config_flag(lambda cfg: scorer_from_config(cfg, library=lib))


def test_f32_table_prep_and_mean_term(lib, monkeypatch):
    fc.check_table_prep(_make_scorer(lib), monkeypatch, channels=176, nq=5, ng=6)
    fc.check_mean_term(_make_scorer(lib), monkeypatch, channels=64)


def test_f32_torch_op(lib):
    """ncc_scores(..., method="mfma_f32") on device tensors equals the C-ABI path of the same method."""
    import torch
    from shoeprint_image_retrieval_amd import _torch_ops

    sc = _make_scorer(lib)("mfma_f32")
    dev = sc.dev
    q = dev.zeros((5, 32, 33, 16), np.float32)
    g = dev.zeros((7, 32, 32, 16), np.float32)
    lib.check(lib.spr_synth_gallery(dev.ptr(g), 0, 7, 32, 32, 16, 5, dev.stream()))
    lib.check(lib.spr_synth_gallery(dev.ptr(q), 900, 5, 32, 33, 16, 5, dev.stream()))
    got = _torch_ops.load().ncc_scores(q, g, 2, "mfma_f32", 0)
    want = dev.zeros((5, 7), np.float32)
    sc.scores_device(q, g, scores=want)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.to_host(got), dev.to_host(want))
    with pytest.raises(RuntimeError, match="28x12"):
        _torch_ops.load().ncc_scores(q.to(torch.bfloat16), g.to(torch.bfloat16), 2, "mfma_f32", 0)


def test_f32_large_gallery(lib, monkeypatch):
    fc.check_large_gallery(_make_scorer(lib), monkeypatch, channels=1024, nq=8, ng=1100)


@pytest.mark.parametrize("channels,q_hw,nq,ng", [(176, (33, 16), 64, 2048), (1024, (32, 16), 64, 5120)])
def test_f32_rate_against_fft(lib, capsys, channels, q_hw, nq, ng):
    """The pair kernel of "mfma_f32" against the FFT form's on the same float32 inputs, in one process: warm-up, then HIP
    events around several repetitions.  Asserts only that the new method is the faster one; both rates are printed."""
    import torch

    reps, rates, outs = 5, {}, {}
    for method in ("mfma_f32", "fft"):
        sc = _make_scorer(lib)(method)
        dev = sc.dev
        g = dev.zeros((ng, channels, 32, 16), np.float32)
        lib.check(lib.spr_synth_gallery(dev.ptr(g), 0, ng, channels, 32, 16, 5, dev.stream()))
        q = dev.zeros((nq, channels, *q_hw), np.float32)
        lib.check(lib.spr_synth_gallery(dev.ptr(q), 5000, nq, channels, *q_hw, 5, dev.stream()))
        plan = sc.plan(channels, q_hw, (32, 16))
        pq, pg = sc.prepare_queries(plan, q), sc.prepare_gallery(plan, g)
        out = dev.zeros((nq, ng), np.float32)
        for _ in range(2):
            sc.score_prepared(plan, pq, nq, pg, ng, out, ng, 0)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            sc.score_prepared(plan, pq, nq, pg, ng, out, ng, 0)
        stop.record()
        torch.cuda.synchronize()
        rates[method] = reps * nq * ng / (start.elapsed_time(stop) * 1e-3)
        outs[method] = dev.to_host(out)
        del pq, pg, g, q
    with capsys.disabled():
        print(f"\n[mfma_f32 rate] {q_hw[0]}x{q_hw[1]} on 32x16 float32, {channels} ch, {nq} x {ng}: matrix cores "
              f"{rates['mfma_f32'] / 1e6:.3f} M pairs/s, FFT form {rates['fft'] / 1e6:.3f} M pairs/s")
    np.testing.assert_allclose(outs["mfma_f32"], outs["fft"], atol=fc.TIGHT, rtol=0)
    assert rates["mfma_f32"] > rates["fft"]
