"""The host COCO RLE (odise_amd/coco_rle.py), the reference of the device encoder: the string format of maskApi.c rleEncode / rleToString /
rleFrString pinned by hand-derived anchors, round trips, and detectron2's instances_to_coco_json record layout."""
import numpy as np
import pytest

from odise_amd import coco_rle as R


def _checkerboard(h, w):
    y, x = np.mgrid[:h, :w]
    return ((y + x) % 2).astype(np.uint8)


def _single(h, w, y, x):
    m = np.zeros((h, w), np.uint8)
    m[y, x] = 1
    return m


ANCHORS = [   # (mask, counts, string) derived by hand from maskApi.c
    (np.array([[1]], np.uint8), [0, 1], "01"),
    (np.zeros((2, 2), np.uint8), [4], "4"),
    (np.array([[1, 1], [0, 0], [0, 0]], np.uint8), [0, 1, 2, 1, 2], "01200"),   # i = 2 takes no delta
    (_single(4, 4, 3, 3), [15, 1], "?1"),
    (_checkerboard(5, 5), [1] * 25, "111" + "0" * 22),
]


@pytest.mark.parametrize("k", range(len(ANCHORS)))
def test_anchor_masks(k):
    mask, counts, string = ANCHORS[k]
    np.testing.assert_array_equal(R.mask_counts(mask), counts)
    rle = R.encode(mask)
    assert rle == {"size": list(mask.shape), "counts": string}
    np.testing.assert_array_equal(R.decode(rle), mask)
    assert R.area(rle) == int(mask.sum())


@pytest.mark.parametrize("counts,string", [([5, 2, 3, 1], "523O"),            # negative delta (1 - 2)
                                           ([100], "T3"),
                                           ([0, 1000000], "0Pb`n0"),
                                           ([10, 20, 30, 5, 40], ":d0n0A:")])
def test_counts_to_string(counts, string):
    assert R.counts_to_string(counts) == string
    np.testing.assert_array_equal(R.string_to_counts(string), counts)


def test_encode_accepts_any_nonzero_value_and_dtype():
    m = np.array([[0.0, 2.5], [-1.0, 0.0]], np.float32)
    b = m != 0
    assert R.encode(m) == R.encode(b) == R.encode(b.astype(np.uint8))
    assert R.encode(b)["counts"] == R.counts_to_string([1, 2, 1])


def _blobs(h, w, seed):
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    for _ in range(4):
        cy, cx, ry, rx = g.integers(0, h), g.integers(0, w), g.integers(1, max(2, h // 3)), g.integers(1, max(2, w // 3))
        y, x = np.mgrid[:h, :w]
        m |= (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1).astype(np.uint8)
    return m


@pytest.mark.parametrize("h,w", [(1, 1), (1, 97), (97, 1), (7, 9), (64, 64), (65, 63), (130, 70)])
def test_round_trips(h, w):
    g = np.random.default_rng(h * 1000 + w)
    cases = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), _checkerboard(h, w), _blobs(h, w, h + w),
             (g.random((h, w)) < 0.3).astype(np.uint8), (g.random((h, w)) < 0.97).astype(np.uint8)]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        cases.append(_single(h, w, y, x))
    if h >= 3 and w >= 2:   # runs that continue across column boundaries: the bottom of one column and the top of the next
        m = np.zeros((h, w), np.uint8)
        m[h - 2:, 0] = 1
        m[:2, 1] = 1
        cases.append(m)
    for m in cases:
        rle = R.encode(m)
        assert rle["size"] == [h, w]
        np.testing.assert_array_equal(R.decode(rle), m)
        assert R.area(rle) == int(m.sum())
        cnts = R.mask_counts(m)
        assert int(cnts.sum()) == h * w and (cnts[1:] > 0).all()


def test_runs_cross_columns():
    m = np.zeros((3, 2), np.uint8)
    m[2, 0] = m[0, 1] = 1                          # j = 2 and j = 3: one run of two ones across the column boundary
    np.testing.assert_array_equal(R.mask_counts(m), [2, 2, 2])
    assert R.encode(m)["counts"] == "222"


def test_decode_accepts_bytes():
    rle = R.encode(_blobs(40, 50, 1))
    np.testing.assert_array_equal(R.decode({"size": rle["size"], "counts": rle["counts"].encode()}), R.decode(rle))


def test_instances_to_coco_json_records():
    g = np.random.default_rng(0)
    masks = (g.random((3, 20, 30)) < 0.4).astype(np.float32)
    inst = {"pred_masks": masks, "scores": np.array([0.9, 0.5, 0.25], np.float32), "pred_classes": np.array([4, 0, 7]),
            "query_index": np.array([3, 1, 2], np.int32)}
    recs = R.instances_to_coco_json(inst, img_id=42)
    assert len(recs) == 3
    for k, r in enumerate(recs):
        assert set(r) == {"image_id", "category_id", "bbox", "score", "segmentation"}
        assert r["image_id"] == 42 and r["category_id"] == int(inst["pred_classes"][k]) and isinstance(r["category_id"], int)
        assert r["bbox"] == [0.0, 0.0, 0.0, 0.0]
        assert isinstance(r["score"], float) and r["score"] == float(inst["scores"][k])
        assert r["segmentation"] == R.encode(masks[k]) and isinstance(r["segmentation"]["counts"], str)
    # the RLE form of the same result gives the same records
    rle_inst = {"pred_masks_rle": [R.encode(m) for m in masks], "area": masks.reshape(3, -1).sum(1).astype(np.int64),
                "scores": inst["scores"], "pred_classes": inst["pred_classes"], "query_index": inst["query_index"]}
    assert R.instances_to_coco_json(rle_inst, 42) == recs
    empty = {"pred_masks": np.zeros((0, 20, 30), np.float32), "scores": np.zeros((0,), np.float32), "pred_classes": np.zeros((0,), np.int64)}
    assert R.instances_to_coco_json(empty, 1) == []
