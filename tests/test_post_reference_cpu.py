"""CPU: tests/post_reference.py (float64 numpy) against oracle.odise_model.postprocess (fp32 torch) wherever the oracle's own margins decide the
outcome, and the caps that tests/test_gpu_postprocess.py relies on, asserted for every crafted case from the reference alone."""
import numpy as np
import pytest
import torch

import post_cases as PC
import post_reference as R
from oracle import odise_model as O

MARGIN = 2.0 ** -20          # top-2 relative margin of score * sigmoid above which the owner of a pixel is decided


@pytest.mark.parametrize("geom,Q,K,seed", [("x4_ragged", 9, 5, 1), ("up", 12, 7, 2), ("down", 6, 4, 3), ("x4_w256", 5, 3, 4)])
def test_restatement_matches_the_fp32_oracle(geom, Q, K, seed):
    c = PC.make("rand", Q, K, geom, seed, dup=False)
    rng = np.random.default_rng(seed)
    c["logits"] = (3 * rng.standard_normal(c["logits"].shape)).astype(np.float16).astype(np.float32)
    pad = (4 * c["h4"], 4 * c["w4"])
    topk = 12                                                              # torch.topk refuses more than Q * K
    ref = R.postprocess(c["mask_cls"], c["logits"], pad, c["img"], c["out"], K, c["thing"], 0.0, 0.8, topk)
    o = O.postprocess(torch.from_numpy(c["mask_cls"])[None], torch.from_numpy(c["logits"])[None], pad, [c["img"]], [c["out"]], K, c["thing"], 0.8, topk)[0]
    np.testing.assert_allclose(o["sem_seg"].numpy(), ref["sem"], rtol=2e-5, atol=1e-6)
    seg, info = o["panoptic_seg"]
    pan = ref["pan"]
    decided = (pan["margin"] > 1e-4) & (np.abs(np.take_along_axis(ref["mask"], np.maximum(pan["owner"], 0)[None], 0)[0]) > 1e-4)
    assert decided.mean() > 0.99
    assert info == pan["info"]
    np.testing.assert_array_equal(seg.numpy()[decided], pan["seg"][decided])
    inst = ref["inst"]
    assert inst["band_count"](1e-5) == 1                                   # the k-th probability stands alone: the oracle's topk picks the same set
    got = sorted(zip(o["instances"]["pred_classes"].tolist(), np.round(o["instances"]["scores"].numpy().astype(np.float64), 5).tolist()))
    want = sorted(zip(inst["cls"].tolist(), np.round(inst["score"], 5).tolist()))
    assert len(got) == len(want)
    for (gc, gs), (wc, ws) in zip(got, want):
        assert gc == wc and abs(gs - ws) <= 2e-5
    # masks, matched through (class, score): wherever no logit of the entry sits at zero
    for i, (q, cl) in enumerate(zip(inst["query"], inst["cls"])):
        j = [j for j in range(len(want)) if int(o["instances"]["pred_classes"][j]) == cl
             and abs(float(o["instances"]["scores"][j]) - inst["score"][i]) <= 2e-5]
        assert j
        far = np.abs(ref["mask"][q]) > 1e-4
        assert any(np.array_equal(o["instances"]["pred_masks"][k].numpy()[far] > 0, inst["masks"][i][far]) for k in j)


def test_taps_of_the_exact_x4_geometry_are_eighths():
    for n in (8, 64, 72):
        i0, i1, t = R.taps(4 * n, n)
        assert set(np.unique(t)) <= {0.0, 0.125, 0.375, 0.625, 0.875}
        assert i0.max() == n - 1 and (i1 - i0).max() == 1


@pytest.mark.parametrize("name", list(PC.sweep()))
def test_sweep_case_margins(name):
    c, ref = PC.sweep()[name], PC.reference(name)
    pan, mask = ref["pan"], ref["mask"]
    exact = c["geom"] in PC.EXACT
    if exact:
        assert np.array_equal(mask * 512, np.round(mask * 512)) and np.abs(mask).max() <= 6
        assert np.abs(mask[mask != 0]).min() >= 1 / 512
    else:                                                                  # the inside / outside flag and the instance masks need |logit| off zero
        near0 = np.abs(mask) < 8 * 2.0 ** -24 * np.abs(mask).max()
        assert near0.mean() <= 1e-3
    # pixels the reference leaves undecided, the deliberate tie between the duplicated queries aside
    und = pan["margin"] <= MARGIN
    if c["dup"]:
        a, b = c["dup"]
        assert pan["keep"][a] and pan["keep"][b]
        assert not (pan["owner"] == b).any() and (pan["owner"] == a).any()          # the lowest index wins the exact tie
        und &= pan["owner"] != a
        und |= pan["margin_distinct"] <= MARGIN                             # ... which the next distinct value must not come close to
    assert und.mean() <= 1e-3, und.mean()
    if exact:                                                              # every pixel is decided: the GPU test compares the area counters and the whole (owner | inside) word
        assert not und.any() and (pan["margin_distinct"] > MARGIN).all()
    assert pan["keep"].sum() >= 2 and 2 <= len(pan["info"]) <= 100, (pan["keep"].sum(), len(pan["info"]))
    # semantic arg-max: top-2 gap against twice the device bound; where the duplicated class column leads, its first copy wins and the gap
    # is the one to the best of the other classes
    sem = ref["sem"]
    if c["twin"]:
        a, b = c["twin"]
        assert np.array_equal(c["mask_cls"][:, a], c["mask_cls"][:, b])
        assert np.abs(sem[a] - sem[b]).max() <= 1e-12 and (sem.argmax(0) == a).mean() > 0.01      # the twin does lead somewhere
    first, decided = R.semantic_decided(sem, c["Q"], c["twin"])
    assert (~decided).mean() <= 1e-2, (name, (~decided).mean())
    # instance head at topk = 100: at most 2 of all Q * K probabilities within the fp32 softmax's band of the k-th (the GPU test holds every
    # other entry to the reference), or everything is selected and there is no k-th to miss
    inst = ref["inst"]
    band = (c["K"] + 8) * 2.0 ** -23
    assert inst["n_selected"] == c["Q"] * c["K"] or inst["band_count"](band) <= 2, (name, inst["band_count"](band))
    assert (inst["gap"] > band).sum() >= 10 or inst["n_selected"] == c["Q"] * c["K"]              # and the things filter leaves entries to check
    assert len(inst["query"]) >= 3


@pytest.mark.parametrize("name", list(PC.decisions()))
def test_decision_cases_say_what_they_claim(name):
    c, pan = PC.decisions()[name], PC.reference(name)["pan"]
    assert pan["margin"].min() > MARGIN                                    # every pixel is decided: the device's map is compared whole
    info, qmap, cnt = pan["info"], pan["qmap"], pan["counts"]
    if name == "all_null":
        assert not pan["keep"].any() and (pan["labels"] == c["K"]).all() and info == [] and not pan["seg"].any()
    elif name == "all_below_threshold":
        assert not pan["keep"].any() and (pan["labels"] != c["K"]).all() and info == []
    elif name == "threshold_between":
        s = pan["scores"]
        assert abs((s[0] - s[1]) - 1e-3) < 1e-5 and pan["keep"].tolist() == [True, False, True, False] and len(info) == 2
    elif name == "kept_loses_all":
        assert pan["keep"].all() and cnt[0, 1] == 0 and cnt[1, 1] > 0 and qmap.tolist() == [1, 0, 2, 3]
    elif name == "stuff_merges_things_do_not":
        assert qmap.tolist() == [1, 2, 1, 3, 4, 5] and [i["category_id"] for i in info] == [1, 2, 2, 3, 0]
    elif name == "overlap_equal":
        a, o = c["expect_ratio"]
        assert (cnt[0, 0], cnt[1, 0]) == (a, o) and 5 * a == 4 * o and a / o == 0.8 and qmap[0] == 1 and len(info) == 2
    elif name == "overlap_below":
        a, o = c["expect_ratio"]
        assert (cnt[0, 0], cnt[1, 0]) == (a, o) and 5 * (a + 1) == 4 * o and qmap[0] == 0 and len(info) == 1
    elif name == "segments_100":
        assert len(info) == 100 and qmap.tolist() == list(range(1, 101))
    elif name == "segments_120":
        uncapped = R.panoptic(c["mask_cls"], PC.reference(name)["mask"], c["K"], c["thing"], 0.0, 0.8, max_segments=10 ** 6)
        assert len(uncapped["info"]) > 100 and len(info) == 100
        assert qmap.max() == 100 and set(np.unique(pan["seg"])) <= set(range(101))
        late = [q for q in range(c["Q"]) if qmap[q] == 0 and uncapped["qmap"][q] > 0]
        merged = [q for q in range(c["Q"]) if q > max(np.flatnonzero(qmap == 100)) and qmap[q] > 0]
        assert late and merged                                             # segments dropped by the cap, and stuff merged into an id from before it


TOPKS = {"levels_q20_k133": (1, 7, 100, 4096), "levels_q7_k3": (1, 7, 100), "levels_q128_k128": (100, 4096), "levels_q128_k129": (100, 4096)}


@pytest.mark.parametrize("name", list(TOPKS))
def test_instance_levels_and_ties(name):
    c = PC.instances()[name]
    p = R.softmax(c["mask_cls"])[:, :c["K"]].reshape(-1)
    u = np.unique(p)[::-1]
    assert ((u[:-1] - u[1:]) / u[:-1]).min() >= 1e-3                        # distinct levels are at least 1e-3 apart
    assert u.size < p.size                                                 # and there are exact ties
    order = np.lexsort((np.arange(p.size), -p))
    straddles = [k for k in TOPKS[name] if k < p.size and p[order[k - 1]] == p[order[k]]]
    assert straddles or name == "levels_q7_k3", "no topk splits a tie block"
    if name == "levels_q20_k133":
        assert set(straddles) >= {1, 7, 100}
    assert any(k > p.size for k in TOPKS[name]) == (name in ("levels_q20_k133", "levels_q7_k3"))


@pytest.mark.parametrize("name", ["dense_q128_k128", "dense_q128_k129"])
def test_instance_dense_band(name):
    c = PC.instances()[name]
    inst = PC.reference(name, 100, False)["inst"]
    band = (c["K"] + 8) * 2.0 ** -23
    assert inst["band_count"](band) <= 2
    p = np.sort(R.softmax(c["mask_cls"])[:, :c["K"]].reshape(-1))[::-1][:110]
    assert ((p[:-1] - p[1:]) / p[:-1]).min() > 2 * band                    # the order inside the selection is decided as well
    assert (c["Q"] * c["K"] <= 16384) == (name == "dense_q128_k128")


def test_entry_case_statistics_are_robust():
    c = PC.entry_case()
    mask = PC.reference(c["name"])["mask"]
    assert np.abs(c["logits"]).max() <= 2.0
    assert R.inst_stats(mask)[2] == 0


def test_rotation_images_differ():
    cs = PC.rotation()
    assert len(cs) == 6 and len({(c["img"], c["out"]) for c in cs}) >= 4
    assert len({c["logits"].tobytes() for c in cs}) == 6
