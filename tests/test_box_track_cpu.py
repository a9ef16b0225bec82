"""CPU: odise_amd.video.BoxColorTracker - the numpy restatement the device box tracker (csrc/box_track.hip) is held to - against a literal
sequential formulation of detectron2's _assign_colors on instances with boxes (a `matched` set, the loop over the old instances, the
threshold 0.6), match_winners at 0.6, hand-worked colours on the crafted sequences of tests/box_track_cases.py, the box IoU against
instance_eval's host box IoU, and the demo's rules for --track-boxes / --draw-boxes.  Everything is exact."""
import numpy as np
import pytest

import box_track_cases as BC
from odise_amd import demo
from odise_amd import instance_eval as IE
from odise_amd import video as VD

CASES = BC.cases()


def geometric_iou(a, b):
    """the IoU of two XYXY float32 boxes through instance_eval.box_iou on their XYWH doubles"""
    return IE.box_iou(IE.xyxy_to_xywh(np.asarray(a, np.float32)[None]), IE.xyxy_to_xywh(np.asarray(b, np.float32)[None]))[0, 0]


class Literal:
    """_assign_colors, written as detectron2 writes it: instances with (label, bbox, color, ttl), the IoU matrix, then the walk"""

    def __init__(self, ttl, pool):
        self.ttl, self.pool, self.old, self.counter, self.frame = ttl, np.asarray(pool, np.uint8).reshape(-1, 3), [], 0, 0

    def assign(self, classes, scores, boxes, min_score, colors):
        colors = np.array(colors, np.uint8)
        new = []
        for i in range(len(boxes)):
            b = np.asarray(boxes[i], np.float32)
            if np.float32(scores[i]) >= np.float32(min_score) and np.isfinite(b).all() and b[2] > b[0] and b[3] > b[1]:
                new.append({"index": i, "frame": self.frame, "label": int(classes[i]), "bbox": b, "color": None, "ttl": self.ttl})
        ious = np.zeros((len(self.old), len(new)), np.float64)
        for a, o in enumerate(self.old):
            for k, n in enumerate(new):
                ious[a, k] = geometric_iou(o["bbox"], n["bbox"]) if o["label"] == n["label"] else 0.0
        threshold = 0.6
        matched_new_per_old = np.asarray(ious).argmax(axis=1) if len(new) else []
        max_iou_per_old = np.asarray(ious).max(axis=1) if len(new) else []
        matched, extra = set(), []
        for idx, o in enumerate(self.old):
            if len(new) and max_iou_per_old[idx] > threshold:
                newidx = int(matched_new_per_old[idx])
                if newidx not in matched:
                    matched.add(newidx)
                    new[newidx]["color"] = o["color"]
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
        area = lambda b: int(min((float(b[2]) - float(b[0])) * (float(b[3]) - float(b[1])), 2147483647.0))
        return [(o["frame"], o["index"], o["label"], area(o["bbox"]), o["ttl"], VD.pack_rgb(o["color"])) for o in self.old]


def run_both(topk, ttl, pool, frames, min_score):
    lit, trk = Literal(ttl, pool), VD.BoxColorTracker(ttl, pool)
    for t, (classes, scores, boxes) in enumerate(frames):
        pre = BC.prefill(topk)
        want, ious = lit.assign(classes, scores, boxes, min_score, pre)
        got = trk.assign(classes, scores, boxes, min_score, pre)
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), t
        assert trk.last_iou.tobytes() == ious.tobytes(), t
        assert [tuple(int(v) for v in r)[:6] for r in trk.live_rows()] == lit.rows(), t
        assert trk.counter == lit.counter and len(trk.live) <= 800
        yield got


@pytest.mark.parametrize("name", sorted(CASES))
def test_tracker_equals_the_literal_formulation(name):
    case = CASES[name]
    for t, got in enumerate(run_both(case.topk, case.ttl, case.pool, case.frames, case.min_score)):
        assert got.tobytes() == BC.expected(case)[t]["colors"].tobytes()


def test_tracker_equals_the_literal_formulation_on_300_random_sequences():
    count = 0
    for topk, ttl, frames in BC.random_sequences(300):
        list(run_both(topk, ttl, VD.default_pool(5), frames, 0.3))
        count += 1
    assert count == 300


def test_the_cases_cover_the_limits_they_are_meant_to():
    assert {c.topk for c in CASES.values()} == {1, 7, 100} and {c.ttl for c in CASES.values()} == {1, 3, 8}
    assert max(len(e["live"]) for e in BC.expected(CASES["cap"])) == 800
    assert any(e["n_before"] > 64 and e["iou"].shape[1] > 32 and (e["iou"] > 0.6).any() for e in BC.expected(CASES["random_hundred"]))
    assert any(e["iou"].shape[1] == 0 for e in BC.expected(CASES["empty_frames"]))


def test_match_winners_at_the_box_threshold():
    iou = np.array([[0.6, 0.59], [0.61, 0.61], [0.0, 0.7], [0.65, 0.9]])
    choice, winner = VD.match_winners(iou, 0.6)
    assert choice == [-1, 0, 1, 1] and winner == {0: 1, 1: 2}                # 0.6 itself is no match; the first of two maxima; the earlier row
    assert VD.match_winners(iou)[0] == [0, 0, 1, 1]                          # the mask trackers' 0.5 is the default, as before
    assert VD.match_winners(np.zeros((2, 0)), 0.6) == ([-1, -1], {})


def pool_rgb(case, k):
    return tuple(int(v) for v in case.pool[k % len(case.pool)])


def test_iou_of_exactly_three_fifths_is_no_match_and_seven_elevenths_is():
    case = CASES["iou_threshold"]
    exp = BC.expected(case)
    assert exp[1]["iou"].tolist() == [[0.6]] and tuple(exp[1]["colors"][0]) == pool_rgb(case, 1)          # a new colour
    assert exp[2]["iou"][0].tolist() == [1.0] and tuple(exp[2]["colors"][0]) == pool_rgb(case, 1)
    assert exp[4]["iou"][0].tolist() == [7 / 11] and tuple(exp[4]["colors"][0]) == tuple(exp[3]["colors"][0]) == pool_rgb(case, 2)
    assert 0.5 < 7 / 11                                                     # and between the mask threshold and this one nothing matches:
    trk = VD.BoxColorTracker(3)
    a = trk.assign([1], [0.9], np.array([[0, 0, 20, 1]], np.float32))
    b = trk.assign([1], [0.9], np.array([[5, 0, 25, 1]], np.float32))       # 15 / 25 = 0.6 again
    c = trk.assign([1], [0.9], np.array([[9, 0, 29, 1]], np.float32))       # 16 / 24 with the second, 11 / 29 with the first
    assert trk.last_iou[0].tolist() == [16 / 24] and a.tobytes() != b.tobytes() and c.tobytes() == b.tobytes()


def test_class_mismatch_tie_and_two_claims():
    case = CASES["class_mismatch"]
    exp = BC.expected(case)
    assert exp[1]["iou"].tolist() == [[0.0, 1.0]]
    assert tuple(exp[1]["colors"][1]) == tuple(exp[0]["colors"][0]) == pool_rgb(case, 0) and tuple(exp[1]["colors"][0]) == pool_rgb(case, 1)
    case = CASES["tie"]
    exp = BC.expected(case)
    assert exp[1]["iou"].tolist() == [[0.0, 1.0, 1.0]]
    c = exp[1]["colors"]
    assert tuple(c[1]) == pool_rgb(case, 0) and tuple(c[0]) == pool_rgb(case, 1) and tuple(c[2]) == pool_rgb(case, 2)
    case = CASES["two_claim"]
    exp = BC.expected(case)
    assert exp[1]["iou"][:, 0].tolist() == [200 / 210, 200 / 210] and tuple(exp[1]["colors"][0]) == pool_rgb(case, 0)
    assert [(int(r["frame"]), int(r["id"]), int(r["ttl"])) for r in exp[1]["live"]] == [(1, 0, 3), (0, 1, 2)]
    assert exp[2]["iou"].tolist() == [[200 / 210, 200 / 210], [1.0, 190 / 210]]
    assert tuple(exp[2]["colors"][0]) == pool_rgb(case, 0) and tuple(exp[2]["colors"][1]) == pool_rgb(case, 2)


@pytest.mark.parametrize("ttl", [1, 3, 8])
def test_a_colour_returns_in_the_last_possible_frame_and_not_one_later(ttl):
    case = CASES[f"gone_ttl{ttl}"]
    exp = BC.expected(case)
    assert tuple(exp[ttl]["colors"][0]) == tuple(exp[0]["colors"][0]) == pool_rgb(case, 0)
    assert tuple(exp[ttl + 1]["colors"][0]) != tuple(exp[0]["colors"][1])    # B comes one frame too late: a new colour
    assert (exp[ttl]["live"]["frame"] >= 1).all()


def test_boxes_without_area_or_with_non_finite_members_are_no_instances():
    case = CASES["bad_boxes"]
    exp, pre = BC.expected(case), BC.prefill(case.topk)
    for e in exp[:6]:
        assert e["live"]["id"][:2].tolist() == [0, 3] and e["live"]["area"][:2].tolist() == [81, 81]
        for i in (1, 2, 4, 5, 6):
            assert e["colors"][i].tobytes() == pre[i].tobytes()
    assert exp[6]["colors"].tobytes() == pre.tobytes() and exp[6]["iou"].shape[1] == 0
    frac = BC.expected(CASES["fractional"])
    assert frac[0]["live"]["area"].tolist() == [0, 127, 2147483647]         # 0.5 x 0.5 is an instance; (int32) of 19.625 x 6.5; the clamp
    assert frac[1]["iou"][0, 0] == 0.25 / 0.28125 and tuple(frac[1]["colors"][0]) == tuple(frac[0]["colors"][0])


def test_the_live_list_fills_to_its_cap_and_nothing_matches():
    exp = BC.expected(CASES["cap"])
    assert [len(e["live"]) for e in exp] == [100, 200, 300, 400, 500, 600, 700, 800, 800, 800]
    assert all((e["iou"] <= 0.6).all() for e in exp)
    assert exp[1]["iou"].max() == 133 / 227 > 0.5                            # neighbours of one class: a mask tracker's match, not a box tracker's


def test_the_box_iou_is_the_host_box_iou_of_instance_eval():
    rng = np.random.default_rng(0)
    a = rng.random((40, 2)).astype(np.float32) * 50
    boxes = np.concatenate([a, a + rng.random((40, 2)).astype(np.float32) * 30 + 0.5], axis=1).astype(np.float32)
    want = IE.box_iou(IE.xyxy_to_xywh(boxes[:20]), IE.xyxy_to_xywh(boxes[20:]))
    trk = VD.BoxColorTracker(3)
    trk.assign(np.zeros(20, np.int32), None, boxes[:20])
    trk.assign(np.zeros(20, np.int32), None, boxes[20:])
    assert trk.last_iou.shape == (20, 20) and trk.last_iou.tobytes() == want.tobytes() and (want > 0).any()


def test_reset_and_bad_arguments():
    trk = VD.BoxColorTracker(3)
    b = np.array([[0, 0, 4, 4], [10, 10, 14, 14]], np.float32)
    first = trk.assign([1, 1], [0.9, 0.9], b)
    with pytest.raises(ValueError):
        trk.assign([1], [0.9, 0.9], b)
    with pytest.raises(ValueError):
        trk.assign([1, 1], [0.9, 0.9], b, colors=np.zeros((1, 3), np.uint8))
    trk.reset()
    assert trk.assign([1, 1], None, b).tobytes() == first.tobytes()
    with pytest.raises(ValueError):
        VD.BoxColorTracker(9)


# ---- the demo's arguments ------------------------------------------------------------------------------------------------------------------
def test_demo_accepts_the_two_flags():
    a = demo.parse_args(["--video-input", "clip", "--output", "out", "--task", "instance", "--track-boxes", "--ttl", "4"])
    assert a.track_boxes and a.draw_boxes and not a.track_masks and a.ttl == 4                  # --track-boxes implies --draw-boxes
    a = demo.parse_args(["--video-input", "clip", "--output", "out", "--task", "instance", "--track-masks", "--draw-boxes"])
    assert a.track_masks and a.draw_boxes and not a.track_boxes
    a = demo.parse_args(["--input", "a.jpg", "--output", "out", "--task", "instance", "--draw-boxes"])
    assert a.draw_boxes and not a.track_boxes
    a = demo.parse_args(["--input", "a.jpg", "--output", "out", "--task", "instance"])
    assert not a.draw_boxes and not a.track_boxes


@pytest.mark.parametrize("argv,word", [(["--input", "a.jpg", "--output", "out", "--task", "instance", "--track-boxes"], "--video-input"),
                                       (["--video-input", "clip", "--output", "out", "--track-boxes"], "instance"),
                                       (["--video-input", "clip", "--output", "out", "--task", "semantic", "--track-boxes"], "instance"),
                                       (["--video-input", "clip", "--output", "out", "--task", "instance", "--track-boxes", "--track-masks"], "--track-masks"),
                                       (["--input", "a.jpg", "--output", "out", "--draw-boxes"], "instance"),
                                       (["--video-input", "clip", "--output", "out", "--task", "instance", "--draw-boxes"], "pred_boxes")])
def test_demo_refuses_the_flags_where_they_mean_nothing(argv, word, capsys):
    with pytest.raises(SystemExit):
        demo.parse_args(argv)
    assert word in capsys.readouterr().err


def test_run_on_video_hands_the_box_options_to_every_frame(monkeypatch):
    seen = []
    monkeypatch.setattr(demo, "run_on_image", lambda ctx, model, vis, image, task, **kw: seen.append(kw) or image)

    class Frame:
        shape = (4, 5, 3)

    list(demo.run_on_video(None, None, None, [("a", lambda ctx: Frame())], "instance", 0.25, True, True))
    list(demo.run_on_video(None, None, None, [("a", lambda ctx: Frame())], "instance", 0.25))
    assert seen == [dict(video=True, confidence_threshold=0.25, draw_boxes=True, track_boxes=True), dict(video=True, confidence_threshold=0.25)]
