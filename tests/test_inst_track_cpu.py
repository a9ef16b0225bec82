"""CPU: odise_amd.video.InstanceColorTracker - the numpy restatement the device instance tracker (csrc/inst_track.hip) is held to - against
a literal sequential formulation of detectron2's _assign_colors on box-less instances, against ColorTracker where the masks do not
overlap, and on the crafted situations of tests/inst_track_cases.py; the demo's rules for --track-masks.  Everything is exact."""
import numpy as np
import pytest

import inst_track_cases as IC
import track_cases as TC
from odise_amd import demo
from odise_amd import video as VD
from odise_amd import visualize as V

CASES = IC.cases()


# ---- the literal formulation: a list of instances, pycocotools-style IoU by plain boolean sums, the sequential walk with a matched set ----
class Literal:
    def __init__(self, ttl, pool):
        self.ttl, self.pool, self.old, self.counter, self.frame = ttl, np.asarray(pool, np.uint8).reshape(-1, 3), [], 0, 0

    def assign(self, classes, scores, masks, min_score, colors):
        colors = np.array(colors, np.uint8)
        new = []
        for i in range(len(masks)):
            if np.float32(scores[i]) >= np.float32(min_score) and masks[i].any():
                new.append({"index": i, "frame": self.frame, "label": int(classes[i]), "mask": masks[i].astype(bool), "color": None, "ttl": self.ttl})
        ious = np.zeros((len(self.old), len(new)), np.float64)
        for a, o in enumerate(self.old):
            for b, n in enumerate(new):
                inter = int(np.logical_and(o["mask"], n["mask"]).sum())
                union = int(o["mask"].sum()) + int(n["mask"].sum()) - inter
                ious[a, b] = float(inter) / float(union) if o["label"] == n["label"] else 0.0
        matched, extra = set(), []
        for a, o in enumerate(self.old):                                   # in list order
            if len(new):
                j = int(np.argmax(ious[a]))
                if ious[a, j] > 0.5 and j not in matched:
                    matched.add(j)
                    new[j]["color"] = o["color"]
                    continue
            o["ttl"] -= 1
            if o["ttl"] > 0:
                extra.append(o)
        for n in new:
            if n["color"] is None:
                n["color"] = tuple(int(v) for v in self.pool[self.counter % len(self.pool)])
                self.counter += 1
            colors[n["index"]] = n["color"]
        self.old = new + extra
        self.frame += 1
        return colors, ious

    def rows(self):
        return [(o["frame"], o["index"], o["label"], int(o["mask"].sum()), o["ttl"], VD.pack_rgb(o["color"])) for o in self.old]


def run_both(case):
    lit, trk = Literal(case.ttl, case.pool), VD.InstanceColorTracker(case.ttl, case.pool)
    for t, (classes, scores, masks) in enumerate(case.frames):
        pre = IC.prefill(case.topk)
        want, ious = lit.assign(classes, scores, masks, case.min_score, pre)
        got = trk.assign(classes, scores, masks, case.min_score, pre)
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), t
        assert trk.last_iou.tobytes() == ious.tobytes(), t
        assert [tuple(int(v) for v in r)[:6] for r in trk.live_rows()] == lit.rows(), t
        assert trk.counter == lit.counter and len(trk.live) <= 8 * 100
        assert got.tobytes() == IC.expected(case)[t]["colors"].tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_tracker_equals_the_literal_formulation(name):
    run_both(CASES[name])


def test_tracker_equals_the_literal_formulation_on_random_sequences():
    for seed in range(60):
        rng = np.random.default_rng(100 + seed)
        hw, topk = (int(rng.integers(3, 12)), int(rng.integers(3, 12))), int(rng.integers(1, 9))
        pool = rng.integers(0, 256, (int(rng.integers(1, 6)), 3))
        run_case = IC.Case(f"r{seed}", hw, topk, int(rng.integers(1, 9)), IC._random(hw, topk, int(rng.integers(3, 12)), seed, classes=2),
                           min_score=float(rng.random()) * 0.6, pool=pool)
        lit, trk = Literal(run_case.ttl, run_case.pool), VD.InstanceColorTracker(run_case.ttl, run_case.pool)
        for classes, scores, masks in run_case.frames:
            pre = IC.prefill(topk)
            want, ious = lit.assign(classes, scores, masks, run_case.min_score, pre)
            assert trk.assign(classes, scores, masks, run_case.min_score, pre).tobytes() == want.tobytes()
            assert trk.last_iou.tobytes() == ious.tobytes()
            assert [tuple(int(v) for v in r)[:6] for r in trk.live_rows()] == lit.rows()


def as_instances(ids, tab):
    """the things of a panoptic frame as an instance selection: one entry per table row (stuff rows and rows without a pixel: empty masks)"""
    rows = VD.frame_instances(ids, tab)
    masks = np.zeros((len(tab),) + ids.shape, bool)
    for r, _, _, m in rows:
        masks[r] = m
    return tab[:, 2].copy(), np.ones(len(tab), np.float32), masks


@pytest.mark.parametrize("name", ["moving", "two_claim", "three_back", "tie", "gone7_ttl8", "gone3_ttl3", "pool3", "long", "hundred", "empty_frame"])
def test_disjoint_masks_give_what_the_panoptic_tracker_gives(name):
    """On frames whose instance masks do not overlap and are all kept both trackers walk the same list: same colours, same live rows
    (a panoptic row's id is the segment id, an instance row's the table index: compared through the table)."""
    case = TC.cases()[name]
    pan, inst = VD.ColorTracker(case.ttl, case.pool), VD.InstanceColorTracker(case.ttl, case.pool)
    history = []
    for t, (ids, tab) in enumerate(case.frames):
        history.append(tab)
        pre = TC.prefill()[:len(tab)]
        want = pan.assign(ids, tab, pre)
        classes, scores, masks = as_instances(ids, tab)
        got = inst.assign(classes, scores, masks, 0.5, pre) if len(tab) else inst.assign(classes, scores, np.zeros((0,) + ids.shape, bool), 0.5, pre)
        assert got.tobytes() == want.tobytes(), t
        assert inst.last_iou.tobytes() == pan.last_iou.tobytes(), t
        a, b = pan.live_rows(), inst.live_rows()
        assert len(a) == len(b)
        for f in ("frame", "category", "area", "ttl", "rgb"):
            assert a[f].tobytes() == b[f].tobytes(), (t, f)
        assert [int(history[r["frame"]][r["id"], 0]) for r in b] == a["id"].tolist(), t


# ---- the crafted situations, by hand -------------------------------------------------------------------------------------------------------
def colours(case):
    return [e["colors"] for e in IC.expected(case)]


def pool_rgb(case, k):
    return tuple(int(v) for v in case.pool[k % len(case.pool)])


def test_heavily_overlapping_masks_of_one_class_each_keep_their_colour():
    case = CASES["overlap_one_class"]
    exp = IC.expected(case)
    assert (exp[1]["iou"] > 0.5).sum(axis=1).min() >= 2                      # every live row has several candidates above 0.5
    first = exp[0]["colors"]
    assert len({tuple(c) for c in first}) == 7
    for e in exp[1:]:
        assert e["colors"].tobytes() == first.tobytes() and len(e["live"]) == 7 and (e["live"]["ttl"] == 3).all()


def test_equal_masks_of_different_classes_have_iou_zero():
    case = CASES["equal_masks_other_class"]
    exp = IC.expected(case)
    assert exp[1]["iou"].tolist() == [[0.0, 1.0]]
    assert tuple(exp[1]["colors"][1]) == tuple(exp[0]["colors"][0]) == pool_rgb(case, 0) and tuple(exp[1]["colors"][0]) == pool_rgb(case, 1)
    assert exp[2]["iou"].tolist() == [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]


def test_iou_of_exactly_one_half_is_no_match_and_five_sevenths_is():
    case = CASES["iou_half"]
    exp = IC.expected(case)
    assert exp[1]["iou"].tolist() == [[0.5]] and tuple(exp[1]["colors"][0]) == pool_rgb(case, 1)
    assert exp[2]["iou"][0].tolist() == [5 / 7] and tuple(exp[2]["colors"][0]) == pool_rgb(case, 1)
    assert exp[2]["iou"][1].tolist() == [np.float64(3) / np.float64(9)]


def test_the_first_of_two_equal_maxima_wins():
    case = CASES["tie"]
    exp = IC.expected(case)
    assert exp[1]["iou"].tolist() == [[0.0, 1.0, 1.0]]
    c = exp[1]["colors"]
    assert tuple(c[1]) == pool_rgb(case, 0) and tuple(c[0]) == pool_rgb(case, 1) and tuple(c[2]) == pool_rgb(case, 2)


def test_two_claims_go_to_the_earlier_list_position():
    case = CASES["two_claim"]
    exp = IC.expected(case)
    assert exp[1]["iou"][:, 0].tolist() == [40 / 44, 40 / 44]
    assert tuple(exp[1]["colors"][0]) == pool_rgb(case, 0)
    live = exp[1]["live"]
    assert [(int(r["frame"]), int(r["id"]), int(r["ttl"])) for r in live] == [(1, 0, 3), (0, 1, 2)]
    # frame 2 = (B's mask, A's mask): N ties between them at 40 / 44 and takes the first; old B has 1.0 with its own mask, which is taken:
    # it does not fall back on A's mask (36 / 44), which takes the next pool colour
    assert exp[2]["iou"].tolist() == [[40 / 44, 40 / 44], [1.0, 36 / 44]]
    assert tuple(exp[2]["colors"][0]) == pool_rgb(case, 0) and tuple(exp[2]["colors"][1]) == pool_rgb(case, 2)


@pytest.mark.parametrize("ttl", [1, 3, 8])
def test_a_colour_returns_in_the_last_possible_frame_and_not_one_later(ttl):
    case = CASES[f"gone_ttl{ttl}"]
    exp = IC.expected(case)
    back = ttl                                                               # frame 0, ttl - 1 frames without A, A in frame ttl
    assert tuple(exp[back]["colors"][0]) == tuple(exp[0]["colors"][0]) == pool_rgb(case, 0)
    before = exp[back - 1]["live"] if back > 1 else exp[0]["live"]
    assert ttl == 1 or (before["ttl"][before["frame"] == 0] == 1).all()      # down to its last frame
    assert tuple(exp[back + 1]["colors"][0]) not in (tuple(exp[0]["colors"][1]),)   # B comes one frame too late: a new colour
    assert (exp[back]["live"]["frame"] >= 1).all()                           # B left the list in the frame that matched A


def test_empty_frames_cost_one_ttl_and_write_no_colour():
    case = CASES["empty_frames"]
    exp = IC.expected(case)
    for t in (3, 4):
        assert exp[t]["colors"].tobytes() == IC.prefill(case.topk).tobytes() and exp[t]["iou"].shape[1] == 0
    assert exp[3]["live"]["ttl"].tolist() == [2] and exp[4]["live"]["ttl"].tolist() == [1]
    assert tuple(exp[5]["colors"][0]) == tuple(exp[2]["colors"][0])          # two frames unseen, ttl 3: the colour is back
    assert len(exp[-1]["live"]) == 0


def test_entries_below_the_score_and_empty_masks_are_no_instances():
    case = CASES["min_score_and_holes"]
    exp = IC.expected(case)
    pre = IC.prefill(case.topk)
    for e in exp:
        assert e["live"]["id"][:3].tolist() == [0, 3, 6]
        for i in (1, 2, 4, 5):
            assert e["colors"][i].tobytes() == pre[i].tobytes()
    assert all(e["colors"].tobytes() == exp[0]["colors"].tobytes() for e in exp)


def test_the_live_list_fills_to_its_cap_and_nothing_matches():
    case = CASES["cap"]
    exp = IC.expected(case)
    assert [len(e["live"]) for e in exp] == [100, 200, 300, 400, 500, 600, 700, 800, 800, 800]
    assert all(not e["iou"].any() for e in exp)
    assert exp[-1]["live"]["frame"].tolist() == [f for f in range(9, 1, -1) for _ in range(100)]
    case = CASES["class_free"]
    assert all(not e["iou"].any() for e in IC.expected(case)) and len(IC.expected(case)[-1]["live"]) == 56


def test_size_change_reset_and_bad_arguments():
    trk = VD.InstanceColorTracker(3)
    m = np.ones((2, 4, 5), bool)
    first = trk.assign([1, 1], [0.9, 0.9], m)
    with pytest.raises(ValueError):
        trk.assign([1, 1], [0.9, 0.9], np.ones((2, 5, 4), bool))
    with pytest.raises(ValueError):
        trk.assign([1], [0.9, 0.9], m)
    with pytest.raises(ValueError):
        trk.assign([1, 1], [0.9, 0.9], m, colors=np.zeros((1, 3), np.uint8))
    trk.reset()
    assert trk.assign([1, 1], [0.9, 0.9], np.ones((2, 5, 4), bool)).tobytes() == first.tobytes()
    assert VD.InstanceColorTracker(3).assign([1, 1], None, np.ones((2, 5, 4), bool)).tobytes() == first.tobytes()   # no scores: no score test
    with pytest.raises(ValueError):
        VD.InstanceColorTracker(9)
    with pytest.raises(ValueError):
        VD.InstanceColorTracker(0)


def test_draw_instance_predictions_is_the_picture_call_with_the_trackers_colours():
    case = CASES["random_ragged"]
    md = {"thing_classes": ["a", "b", "c"], "thing_colors": [(250, 10, 10), (10, 250, 10), (10, 10, 250)]}
    rng = np.random.default_rng(3)
    twin, ref = VD.InstanceColorTracker(case.ttl), VD.InstanceColorTracker(case.ttl)
    for classes, scores, masks in case.frames[:4]:
        image = rng.integers(0, 256, case.hw + (3,)).astype(np.uint8)
        got = VD.draw_instance_predictions(image, masks, classes, scores, twin, md, 128, case.min_score, labels=False)
        colors = ref.assign(classes, scores, masks, case.min_score, V.instance_colors(classes, md))
        want = V.instance_overlay(image, masks, colors, V.instance_edge_colors(colors), 128, scores, case.min_score)
        assert got.tobytes() == want.tobytes()
        labelled = VD.draw_instance_predictions(image, masks, classes, scores, VD.InstanceColorTracker(case.ttl), md, 128, case.min_score)
        assert labelled.shape == image.shape and labelled.dtype == np.uint8


# ---- the demo's arguments ------------------------------------------------------------------------------------------------------------------
def test_demo_accepts_instances_on_video_with_track_masks():
    a = demo.parse_args(["--video-input", "clip", "--output", "out", "--task", "instance", "--track-masks", "--confidence-threshold", "0.3", "--ttl", "4"])
    assert a.track_masks and a.task == "instance" and a.video_input == "clip" and a.confidence_threshold == 0.3 and a.ttl == 4
    assert not demo.parse_args(["--video-input", "clip", "--output", "out"]).track_masks


@pytest.mark.parametrize("argv,word", [(["--input", "a.jpg", "--output", "out", "--task", "instance", "--track-masks"], "--video-input"),
                                       (["--video-input", "clip", "--output", "out", "--track-masks"], "instance"),
                                       (["--video-input", "clip", "--output", "out", "--task", "semantic", "--track-masks"], "instance"),
                                       (["--video-input", "clip", "--output", "out", "--task", "instance"], "pred_boxes")])
def test_demo_refuses_track_masks_where_there_is_nothing_to_track(argv, word, capsys):
    with pytest.raises(SystemExit):
        demo.parse_args(argv)
    assert word in capsys.readouterr().err


def test_run_on_video_hands_the_threshold_to_every_frame(monkeypatch):
    seen = []
    monkeypatch.setattr(demo, "run_on_image", lambda ctx, model, vis, image, task, video=False, confidence_threshold=None: seen.append((task, confidence_threshold, video)) or image)

    class Frame:
        shape = (4, 5, 3)

    list(demo.run_on_video(None, None, None, [("a", lambda ctx: Frame()), ("b", lambda ctx: Frame())], "instance", 0.25))
    assert seen == [("instance", 0.25, True)] * 2
