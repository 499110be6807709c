"""``torch.ops.shoeprint_mi355x`` — the PyTorch-ROCm custom-op face of the C ABI (csrc/torch_ops.cpp).

``load()`` registers the operators (``TORCH_LIBRARY``) by loading ``libshoeprint_torch_ops.so`` (built in-tree next to
``libshoeprint_mi355x.so``, which it links) and returns the op namespace:

* ``ncc_scores(q, g, crop=2, method="auto", max_prepared_bytes=0) -> float32 [Q, G]``   (similarity.py:129-227)
* ``ranks(scores, match) -> int32 [Q]``                                                (similarity.py:378-386)
* ``extract(images, packed, arch, block, mean, std) -> float32 [N, C, h, w]``          (network.py:210-244, plain VGG)
* ``extract_taps(images, packed, arch, block, mean, std, compute, taps) -> [float32 [N, C_t, h_t, w_t]..., out]``  (one pass, the
  activations at the slice ends ``taps`` then the output; arch 0 .. 2 plain VGG, 16 + EfficientNet arch, 32 ResNet50, 48 DenseNet_201)
* ``topk(scores, k) -> (float32 [Q, k], int32 [Q, k])``                                 (the k best items per row, ranker's order)
* ``ncc_scores_located(q, g, crop=2, method="auto", max_prepared_bytes=0) -> (float32 [Q, G], int32 [Q, G, 2])``
  (``ncc_scores`` and the pixel at which every pair's NCC map peaks, (-1, -1) where the score is 0; "fft" / "direct" plans)
* ``surface_peaks(surfaces, n_peaks, ry, rx) -> (float32 [n, n_peaks], int32 [n, n_peaks], float32 [n])``
  (the best separated peaks of every correlation surface, positions packed ``(y << 16) | x``, and the peak-to-sidelobe ratio)

They take GPU tensors, run on PyTorch's current HIP stream and never synchronise; the ctypes route (``_lib.py``) calls the
very same entry points.  ``SPR_TORCH_OPS=0`` keeps the host mirror on the ctypes route (A/B and parity tests).
"""

from __future__ import annotations

import os

_HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(_HERE, "libshoeprint_torch_ops.so")
_ops = None


def load():
    """The op namespace; raises if the extension is not built (``make -C shoeprint-image-retrieval_amd/csrc``)."""
    global _ops
    if _ops is None:
        import torch

        if not os.path.exists(PATH):
            raise RuntimeError(f"{PATH} not found: build it with `make -C shoeprint-image-retrieval_amd/csrc`")
        torch.ops.load_library(PATH)
        _ops = torch.ops.shoeprint_mi355x
    return _ops


def enabled() -> bool:
    """Should the host mirror route through torch.ops?  Yes when the extension is built and not switched off."""
    return os.environ.get("SPR_TORCH_OPS", "1") != "0" and os.path.exists(PATH)
