"""Float64 restatement of the semantic test-time augmentation (odise_amd/tta.py, csrc/tta.hip) on tests/post_reference.py: per view the
upsampled fp16-rounded logits, mirrored back for a mirrored view, their sigmoid, and softmax(mask_cls)[:, :K]; summed over the views and
divided by their number - what SemanticSegmentorWithTTA computes with `final_predictions += ...; final_predictions / count`.

Error bound of the device result (`tta_bound`), with A views of Q queries, n = A * Q terms, all of them non-negative:
  * every term is fp16(p) * fp16(s): two roundings of 2^-11 relative each and their product, (1 + 2^-11)^2 - 1 = 2^-10 + 2^-22 of the term,
    hence of the sum;
  * the fp32 summation of n non-negative terms in any order: at most n * 2^-24 of the sum;
  * a probability below the fp16 normal range loses at most 2^-24 absolutely, times a sigmoid <= 1, per term: n * 2^-24 on the sum;
  * the division by A is one fp32 rounding of the mean: 2^-24 of it, and it carries the absolute term as n * 2^-24 / A.
So |device - ref| <= (2^-10 + 2^-22 + (n + 1) * 2^-24) * ref + n * 2^-24 / A for the mean `ref`.
"""
import numpy as np

import post_reference as R


def view_scores(view, K, out_hw) -> np.ndarray:
    """[K, oh, ow] semantic scores of one view at the output size, mirrored back when the view is mirrored."""
    m = R.upsample(R.f16_round(view["logits"]), view["pad"], view["img"], out_hw)
    if view["hflip"]:
        m = m[:, :, ::-1]
    return R.semantic(view["mask_cls"], m, K)


def tta(case) -> np.ndarray:
    total = np.zeros((case["K"],) + tuple(case["out"]), np.float64)
    for v in case["views"]:
        total += view_scores(v, case["K"], case["out"])
    return total / len(case["views"])


def tta_loop(case) -> np.ndarray:
    """The literal loop: each view's [K, h, w] at the output size, np.flip, add, divide."""
    K, out = case["K"], case["out"]
    final, count = np.zeros((K,) + tuple(out), np.float64), 0
    for v in case["views"]:
        count += 1
        sem = R.semantic(v["mask_cls"], R.upsample(R.f16_round(v["logits"]), v["pad"], v["img"], out), K)
        final += np.flip(sem, axis=2) if v["hflip"] else sem
    return final / count


def tta_bound(ref, Q, A) -> np.ndarray:
    n = A * Q
    return (2.0 ** -10 + 2.0 ** -22 + (n + 1) * 2.0 ** -24) * ref + n * 2.0 ** -24 / A


def tta_decided(sem, Q, A, twin=None):
    """(first maximum, decided) per pixel: decided = the top-2 gap exceeds twice the bound (R.semantic_decided's rule).  twin = (a, b): class
    column b repeats a (a < b), the two tie exactly and the first wins; b is left out of the gap."""
    s = np.array(sem, np.float64)
    if twin is not None:
        s[twin[1]] = -np.inf
    top2 = np.partition(s, -2, axis=0)[-2:]
    return s.argmax(0), (top2[1] - top2[0]) > 2 * tta_bound(top2[1], Q, A)
