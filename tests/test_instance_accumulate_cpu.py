"""CPU: the inputs of tests/accum_cases.py have the properties they are named for (under instance_eval.accumulate, the reference the device is
held to), the ctypes descriptor of odise_hip_instance_accumulate follows the header, and the score key orders floats as -score does."""
import ctypes as C
import re

import numpy as np
import pytest

import accum_cases as AC
from odise_amd import instance_eval as IE
from odise_amd.instance_seg_eval import HipInstanceSegEvaluator


def _rows(name):
    return AC.compact(AC.case(name)["blocks"])


@pytest.mark.parametrize("name", AC.VALID)
def test_every_case_is_well_formed(name):
    c = AC.case(name)
    p, r = c["want"]
    K = c["K"]
    assert p.shape == (10, 101, K, 4, 3) and r.shape == (10, K, 4, 3)
    rows = _rows(name)
    assert ((rows["category"] >= 0) & (rows["category"] < K)).all() and not np.isnan(rows["score"]).any()
    first = [b[0].reshape(-1, AC.TOPK)["image"][s, 0] for b in c["blocks"] for s in range(len(b[1])) if b[1][s]]
    assert len(set(first)) == len(first), "no two slots share an image number"
    for k in range(K):
        for a in range(4):
            assert ((p[:, :, k, a] == -1).all() and (r[:, k, a] == -1).all()) == (c["npig"][k, a] == 0)
    assert sum(len(b[1]) for b in c["blocks"]) * AC.TOPK <= 1 << 24


def test_empty_inputs():
    c = AC.case("no_rows")
    assert c["blocks"] == [] and (c["npig"] > 0).all()
    assert (c["want"][0] == 0).all() and (c["want"][1] == 0).all()
    c = AC.case("empty_slot")
    assert list(c["blocks"][0][1]) == [100, 0, 100]


def test_one_category_and_minus_one_cells():
    assert AC.case("one_category")["K"] == 1
    c = AC.case("minus_one")
    p, r = c["want"]
    rows = _rows("minus_one")
    assert (rows["category"] == 0).any() and (p[:, :, 0, 1] == -1).all() and (p[:, :, 0, 0] > -1).all()      # rows, npig == 0 in a range
    assert not (rows["category"] == 1).any() and (c["npig"][1] > 0).all()
    assert (r[:, 1] == 0).all() and (p[:, :, 1] == 0).all()                                                  # npig > 0 and no rows: recall 0
    assert (p[:, :, 3] == -1).all()


def test_bit_patterns():
    for name, tp, fp in (("all_ignored", False, False), ("all_matched", True, False), ("none_matched", False, True)):
        rows = _rows(name)
        assert ((rows["matched"] & ~rows["ignored"] & AC.MASK40) != 0).any() == tp
        assert ((~rows["matched"] & ~rows["ignored"] & AC.MASK40) != 0).any() == fp
    assert (AC.case("all_ignored")["want"][0] == 0).all()
    assert AC.case("all_matched")["want"][0].max() == 1.0 and AC.case("none_matched")["want"][1].max() == 0


def test_the_max_det_cuts_bite():
    c = AC.case("fifteen_of_one_category")
    rows = _rows("fifteen_of_one_category")
    assert np.count_nonzero((rows["image"] == 0) & (rows["category"] == 1)) == 15
    r = c["want"][1][:, 1, 0]                      # category 1, range "all": [T, M]
    assert (r[:, 0] <= r[:, 1]).all() and (r[:, 1] <= r[:, 2]).all() and (r[:, 0] < r[:, 1]).any() and (r[:, 1] < r[:, 2]).any()
    rows = _rows("hundred_of_one_category")
    assert np.count_nonzero((rows["image"] == 7) & (rows["category"] == 2)) == 100
    r = AC.case("hundred_of_one_category")["want"][1][:, 2, 0]
    assert (r[:, 0] <= r[:, 1]).all() and (r[:, 1] <= r[:, 2]).all() and (r[:, 0] < r[:, 1]).any() and (r[:, 1] < r[:, 2]).any()


def test_ties_are_present_and_their_order_matters():
    for name in ("ties_descending_images", "interleaved_blocks"):
        c = AC.case(name)
        rows = _rows(name)
        for k in range(c["K"]):
            rk = rows[rows["category"] == k]
            s, n = np.unique(rk["score"], return_counts=True)
            assert (n > 1).any()
            tied = rk[rk["score"] == s[np.argmax(n)]]
            assert len(np.unique(tied["image"])) > 1 and np.bincount(tied["image"] - tied["image"].min()).max() > 1   # across and inside pictures
        # with the tie-break turned round (image descending) the result is another one
        flipped = rows.copy()
        flipped["image"] = 1000 - flipped["image"]
        other = IE.accumulate(flipped, c["npig"], c["K"])
        assert other[0].tobytes() != c["want"][0].tobytes()
    img = [b[0].reshape(-1, AC.TOPK)["image"][:, 0] for b in AC.case("ties_descending_images")["blocks"]]
    assert (np.diff(img[0]) < 0).all()
    a, b = [x[0].reshape(-1, AC.TOPK)["image"][:, 0] for x in AC.case("interleaved_blocks")["blocks"]]
    assert a.min() < b.min() < a.max() < b.max()


def test_special_scores_and_sizes():
    s = _rows("special_scores")["score"]
    assert np.isposinf(s).any() and np.isneginf(s).any() and (s < 0).any() and ((s != 0) & (np.abs(s) < 1.1754944e-38)).any()
    assert (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any()
    c = AC.case("block_boundary")
    assert [len(b[1]) for b in c["blocks"]] == [64, 64] and list(c["blocks"][1][1][:2]) == [20, 0]
    assert np.bincount(_rows("long_category")["category"]).max() > 2000
    c = AC.case("wide_key")
    n = sum(len(b[1]) for b in c["blocks"]) * AC.TOPK
    assert c["K"] == 133 and len(_rows("wide_key")) == 30000 and n % 2048 != 0 and n % 256 == 0


def test_flag_cases():
    c = AC.case("bad_category")
    assert (AC.compact(c["blocks"])["category"] == c["K"]).sum() == 1 and c["flag"] == IE.ACCUM_FLAG_BAD_CLASS
    c = AC.case("nan_score")
    assert np.isnan(AC.compact(c["blocks"])["score"]).sum() == 1 and c["flag"] == IE.ACCUM_FLAG_NAN_SCORE
    assert len(IE.accumulate_flag_names(3)) == 2


def test_score_key_orders_as_minus_score():
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-42, 3.4028235e38, -3.4028235e38, 1.1754944e-38, 0.5, 0.5, -0.0, 0.0,
                        0.49999997, 0.50000006], np.float32)
    g = np.random.default_rng(3)
    s = np.concatenate([special, g.permutation(special), g.standard_normal(200).astype(np.float32), g.integers(0, 5, 100).astype(np.float32) / 4])
    key = IE.score_sort_key(s)
    assert key.dtype == np.uint32
    np.testing.assert_array_equal(np.argsort(key, kind="stable"), np.argsort(-s, kind="mergesort"))
    assert key[0] == key[1] and key[4] == key.min() and key[5] == key.max()
    for i in range(len(special)):
        for j in range(len(special)):
            assert (key[i] == key[j]) == (special[i] == special[j]) and (key[i] < key[j]) == (special[i] > special[j])


def test_slots_of_restores_the_pictures_or_declines():
    rows = _rows("block_boundary")
    out, counts = HipInstanceSegEvaluator.slots_of(rows, AC.TOPK)
    assert len(counts) == 65 and (counts == 20).all() and AC.compact([(out, counts)]).tobytes() == rows.tobytes()
    assert HipInstanceSegEvaluator.slots_of(np.concatenate([rows, rows[:20]]), AC.TOPK) is None           # image 0 comes back
    assert HipInstanceSegEvaluator.slots_of(rows, 19) is None
    out, counts = HipInstanceSegEvaluator.slots_of(rows[:0], AC.TOPK)
    assert len(out) == 0 and len(counts) == 0


# ---- the descriptor -----------------------------------------------------------------------------------------------------------------------
def test_descriptor_follows_the_header():
    import __graft_entry__ as entry
    from odise_amd import _lib
    entry.build()
    lib = _lib.load()
    assert lib.odise_hip_sizeof_inst_accum_desc() == C.sizeof(_lib.InstAccumDesc)
    assert hasattr(lib, "odise_hip_instance_accumulate")
    text = _lib._header_text()
    body = re.search(r"typedef struct \{([^}]*)\}\s*odise_inst_accum_desc;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields.append((re.search(r"(\w+)$", decl).group(1), "*" in decl))
    want = [(n, t is C.c_void_p) for n, t in _lib.InstAccumDesc._fields_]
    assert fields == want, (fields, want)
    assert all(t in (C.c_void_p, C.c_int) for _, t in _lib.InstAccumDesc._fields_)
