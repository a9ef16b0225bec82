"""Seeded inputs of COCOeval.accumulate for tests/test_instance_accumulate_cpu.py (which shows that each case has the property it is named
for) and tests/test_gpu_instance_accumulate.py (which holds the device to instance_eval.accumulate byte for byte on them).

A case is {"blocks": [(rows ROW_DTYPE [slots * TOPK], counts int32 [slots]), ..], "npig": int64 [K, 4], "K": K, "flag": 0 or the flag it
raises}: the layout the evaluator keeps on the device, a slot per picture, only the first counts[s] rows of a slot exist (the others
hold junk here, so that reading them shows)."""
import numpy as np

from odise_amd import instance_eval as IE

TOPK = 100
MASK40 = (1 << 40) - 1


def picture(g, image, cats, scores=None, p_match=0.5, p_ignore=0.2):
    """Rows of one picture in descending score; scores default to multiples of 1/16, so ties within and across pictures are common."""
    n = len(cats)
    rows = np.zeros(n, IE.ROW_DTYPE)
    s = (g.integers(0, 17, n) / 16).astype(np.float32) if scores is None else np.asarray(scores, np.float32)
    order = np.argsort(-s, kind="mergesort")
    rows["score"], rows["category"], rows["image"] = s[order], np.asarray(cats, np.int32)[order], image
    rows["area"] = g.integers(1, 20000, n)
    bits = g.random((n, 40))
    rows["matched"] = ((bits < p_match) << np.arange(40, dtype=np.uint64)).sum(1).astype(np.uint64)
    bits = g.random((n, 40))
    rows["ignored"] = ((bits < p_ignore) << np.arange(40, dtype=np.uint64)).sum(1).astype(np.uint64)
    return rows


def block(g, pictures, slots=None):
    """pictures: a list of row arrays (None or empty = a slot with no rows) -> (rows [slots * TOPK], counts [slots])."""
    slots = len(pictures) if slots is None else slots
    rows = np.zeros((slots, TOPK), IE.ROW_DTYPE)
    rows["category"], rows["score"] = 1 << 20, np.nan                  # junk where no row exists: never to be read
    rows["matched"] = rows["ignored"] = np.uint64(MASK40)
    rows["image"] = g.integers(-5, 5, (slots, TOPK))
    counts = np.zeros(slots, np.int32)
    for s, p in enumerate(pictures):
        if p is not None and len(p):
            assert len(p) <= TOPK
            rows[s, :len(p)], counts[s] = p, len(p)
    return rows.reshape(-1), counts


def compact(blocks):
    """The rows that exist, in arrival order: what instance_eval.accumulate takes."""
    out = [r.reshape(len(c), TOPK)[s, :c[s]] for r, c in blocks for s in range(len(c))]
    return np.concatenate(out) if out else np.zeros(0, IE.ROW_DTYPE)


def _npig_for(g, blocks, K):
    """About half of a category's rows in every range (at least 1), so that the recall thresholds are crossed all along the rows."""
    rows = compact(blocks)
    per = np.bincount(rows["category"][(rows["category"] >= 0) & (rows["category"] < K)], minlength=K)
    return np.maximum(1, (per[:, None] * g.uniform(0.2, 0.6, (K, 4))).astype(np.int64))


def _random_blocks(g, n_pictures, K, chunk=None, n_rows=TOPK, first_image=0):
    pics = [picture(g, first_image + i, g.integers(0, K, n_rows)) for i in range(n_pictures)]
    chunk = n_pictures if chunk is None else chunk
    return [block(g, pics[i:i + chunk], chunk) for i in range(0, n_pictures, chunk)]


def _case(blocks, npig, K, flag=0):
    return {"blocks": blocks, "npig": np.asarray(npig, np.int64).reshape(K, 4), "K": K, "flag": flag}


def build(name):
    g = np.random.default_rng(sum(map(ord, name)))
    if name == "no_rows":                     # no block at all
        return _case([], g.integers(1, 9, (3, 4)), 3)
    if name == "empty_slot":                  # a slot with counts == 0 between full ones
        pics = [picture(g, 0, g.integers(0, 3, 100)), None, picture(g, 2, g.integers(0, 3, 100))]
        b = [block(g, pics)]
        return _case(b, _npig_for(g, b, 3), 3)
    if name == "one_category":
        b = _random_blocks(g, 3, 1, n_rows=40)
        return _case(b, _npig_for(g, b, 1), 1)
    if name == "minus_one":                   # category 0: rows, npig == 0 in two ranges; category 1: npig > 0 and no rows; category 3: neither
        b = [block(g, [picture(g, i, g.choice([0, 2], 30)) for i in range(4)])]
        return _case(b, [[9, 0, 5, 0], [4, 1, 2, 1], [30, 10, 0, 20], [0, 0, 0, 0]], 4)
    if name in ("all_ignored", "all_matched", "none_matched"):
        pm, pi = {"all_ignored": (0.5, 2.0), "all_matched": (2.0, 0.0), "none_matched": (-1.0, 0.0)}[name]
        b = [block(g, [picture(g, i, g.integers(0, 2, 50), p_match=pm, p_ignore=pi) for i in range(3)])]
        return _case(b, _npig_for(g, b, 2), 2)
    if name == "fifteen_of_one_category":     # the cuts at 1 and 10 bite
        b = [block(g, [picture(g, 0, [1] * 15 + [0] * 5, p_ignore=0.0), picture(g, 1, g.integers(0, 2, 12), p_ignore=0.0)])]
        return _case(b, [[6, 6, 6, 6], [12, 12, 12, 12]], 2)
    if name == "hundred_of_one_category":
        b = [block(g, [picture(g, 7, [2] * 100), picture(g, 3, g.integers(0, 3, 100))])]
        return _case(b, _npig_for(g, b, 3), 3)
    if name == "ties_descending_images":      # equal scores inside a picture and across pictures; the slots arrive in descending image order
        pics = [picture(g, 40 - 3 * i, g.integers(0, 2, 30), scores=g.choice([0.25, 0.5, 0.75], 30)) for i in range(9)]
        b = [block(g, pics)]
        return _case(b, _npig_for(g, b, 2), 2)
    if name == "interleaved_blocks":          # two blocks whose image numbers interleave
        a = [picture(g, 2 * i, g.integers(0, 2, 30), scores=g.choice([0.25, 0.5], 30)) for i in range(5)]
        c = [picture(g, 2 * i + 1, g.integers(0, 2, 30), scores=g.choice([0.25, 0.5], 30)) for i in range(5)]
        b = [block(g, a), block(g, c)]
        return _case(b, _npig_for(g, b, 2), 2)
    if name == "special_scores":              # +-0, negative, denormal, +-inf, the largest and the smallest finite values
        special = np.array([0.0, -0.0, -1.5, 1e-42, -1e-42, np.inf, -np.inf, 3.4028235e38, -3.4028235e38, 1.1754944e-38, 0.5, -0.0, 0.0],
                           np.float32)
        pics = [picture(g, i, g.integers(0, 2, 26), scores=g.permutation(np.r_[special, special])) for i in range(4)]
        b = [block(g, pics)]
        return _case(b, _npig_for(g, b, 2), 2)
    if name == "block_boundary":              # 65 pictures in chunks of 64, as the evaluator keeps them
        b = _random_blocks(g, 65, 5, chunk=64, n_rows=20)
        return _case(b, _npig_for(g, b, 5), 5)
    if name == "long_category":               # more than 2000 rows in a category: beyond one block-wide scan
        b = _random_blocks(g, 70, 3)
        return _case(b, _npig_for(g, b, 3), 3)
    if name == "wide_key":                    # 30000 rows, no multiple of the sort's tile; the category takes more than one digit
        b = _random_blocks(g, 300, 133, chunk=64)
        return _case(b, _npig_for(g, b, 133), 133)
    if name in ("bad_category", "nan_score"):
        pics = [picture(g, i, g.integers(0, 3, 30)) for i in range(3)]
        if name == "bad_category":
            pics[1]["category"][7] = 3
        else:
            pics[2]["score"][0] = np.nan
        b = [block(g, pics)]
        return _case(b, _npig_for(g, b, 3), 3, flag=IE.ACCUM_FLAG_BAD_CLASS if name == "bad_category" else IE.ACCUM_FLAG_NAN_SCORE)
    raise KeyError(name)


VALID = ["no_rows", "empty_slot", "one_category", "minus_one", "all_ignored", "all_matched", "none_matched", "fifteen_of_one_category",
         "hundred_of_one_category", "ties_descending_images", "interleaved_blocks", "special_scores", "block_boundary", "long_category",
         "wide_key"]
FLAGGED = ["bad_category", "nan_score"]

_cache = {}


def case(name):
    """The case and, for a valid one, instance_eval.accumulate of it under "want": computed once, shared, not to be written to."""
    if name not in _cache:
        c = build(name)
        if not c["flag"]:
            c["want"] = IE.accumulate(compact(c["blocks"]), c["npig"], c["K"])
            for a in c["want"]:
                a.setflags(write=False)
        _cache[name] = c
    return _cache[name]
