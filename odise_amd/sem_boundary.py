"""Host restatement of the Boundary IoU counters of detectron2's SemSegEvaluator (numpy), the reference of
`Context.label_boundary` / `Context.semantic_boundary_confusion` (csrc/eval_ops.hip) and the encoder for label maps that live on the host.

`SemSegEvaluator.process` fills `_b_conf_matrix` when OpenCV is importable and the dataset has fewer than 255 classes: prediction and
ground truth both go through

    _mask_to_boundary(mask, dilation_ratio=0.02):
        dilation = max(1, int(round(dilation_ratio * sqrt(h**2 + w**2))))
        padded   = cv2.copyMakeBorder(mask, 1, 1, 1, 1, cv2.BORDER_CONSTANT, value=0)
        eroded   = cv2.erode(padded, np.ones((3, 3), np.uint8), iterations=dilation)[1:-1, 1:-1]
        return mask - eroded

(cv2.erode's default border never contributes to a minimum), and the pairs (boundary(pred), boundary(gt)) are counted like the labels
themselves.  `dilation` 3x3 erosions behind a ring of zeros are one (2 r + 1)^2 minimum that sees zeros outside the picture, which is
the closed form written here: 0 within r of an edge, the window minimum elsewhere.  The result is a label difference, not a binary mask.
"""
from __future__ import annotations

import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MAX_CLASSES = 254   # the evaluator computes Boundary IoU for num_classes < 255: labels 0..K-1 and the ignore label K share a uint8


def boundary_radius(H: int, W: int) -> int:
    if H < 1 or W < 1:
        raise ValueError(f"boundary_radius: bad size {H}x{W}")
    return max(1, int(round(0.02 * math.sqrt(H * H + W * W))))


def clamp_labels(m: np.ndarray, K: int) -> np.ndarray:
    """Values outside [0, K] become the ignore label K (what the evaluator's `gt[gt == ignore_label] = num_classes` leaves)."""
    m = np.asarray(m)
    return np.where((m < 0) | (m > K), K, m).astype(np.int32)


def erode(m: np.ndarray, radius: int) -> np.ndarray:
    m = np.asarray(m)
    H, W = m.shape
    r = int(radius)
    e = np.zeros_like(m)
    if r < 1:
        raise ValueError(f"erode: radius {radius}")
    if 2 * r + 1 > min(H, W):
        return e
    rows = sliding_window_view(m, 2 * r + 1, axis=1).min(axis=2)              # [H, W - 2r]
    e[r:H - r, r:W - r] = sliding_window_view(rows, 2 * r + 1, axis=0).min(axis=2)
    return e


def mask_to_boundary(m: np.ndarray, radius: int | None = None) -> np.ndarray:
    """m [H, W] of non-negative labels -> m - erode(m), same dtype; radius None (or <= 0): the evaluator's formula."""
    m = np.asarray(m)
    r = boundary_radius(*m.shape) if radius is None or radius <= 0 else int(radius)
    return m - erode(m, r)


def boundary_confusion(pred: np.ndarray, gt: np.ndarray, K: int, radius: int | None = None) -> np.ndarray:
    """int64 [(K+1), (K+1)], rows = prediction: the counts one picture adds to `_b_conf_matrix`."""
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"boundary_confusion: K = {K} (the evaluator computes Boundary IoU for 1..{MAX_CLASSES} classes)")
    bp = mask_to_boundary(clamp_labels(pred, K), radius)
    bg = mask_to_boundary(clamp_labels(gt, K), radius)
    n = K + 1
    return np.bincount((n * bp + bg).reshape(-1).astype(np.int64), minlength=n * n).reshape(n, n).astype(np.int64)
