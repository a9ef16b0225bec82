"""CPU: the colour tracker's rule (odise_amd/video.py ColorTracker: the reference csrc/track.hip is held to) against a literal sequential
formulation written here, the hand-worked expectations of the crafted sequences of tests/track_cases.py, and the demo's video arguments
and frame sources."""
import os

import numpy as np
import pytest

import track_cases as TC
from odise_amd import demo
from odise_amd import video as VD

CASES = TC.cases()


# ---- the literal formulation: lists of boolean masks, np.argmax over a dense float64 matrix, the sequential walk ---------------------------
class Literal:
    def __init__(self, ttl, pool):
        self.ttl, self.pool, self.old, self.counter, self.frame = ttl, np.asarray(pool, np.uint8).reshape(-1, 3), [], 0, 0

    def assign(self, ids, tab, colors):
        colors = np.array(colors, np.uint8)
        seen, new = set(), []
        for r, (i, isthing, cat) in enumerate(np.asarray(tab).reshape(-1, 3).tolist()):
            first = i not in seen
            seen.add(i)
            if first and isthing != 0 and i > 0 and (ids == i).any():
                new.append({"row": r, "frame": self.frame, "id": i, "label": cat, "mask": ids == i, "color": None, "ttl": self.ttl})
        ious = np.zeros((len(self.old), len(new)), np.float64)
        for a, o in enumerate(self.old):
            for b, n in enumerate(new):
                inter = np.count_nonzero(o["mask"] & n["mask"])
                union = np.count_nonzero(o["mask"]) + np.count_nonzero(n["mask"]) - inter
                ious[a, b] = (float(inter) / float(union)) if o["label"] == n["label"] else 0.0
        extra = []
        for a, o in enumerate(self.old):                                   # in list order
            if len(new) == 0:
                o["ttl"] -= 1
                if o["ttl"] > 0:
                    extra.append(o)
                continue
            j = int(np.argmax(ious[a]))
            if ious[a, j] > 0.5 and new[j]["color"] is None:
                new[j]["color"] = o["color"]
                continue
            o["ttl"] -= 1
            if o["ttl"] > 0:
                extra.append(o)
        for n in new:
            if n["color"] is None:
                n["color"] = tuple(int(v) for v in self.pool[self.counter % len(self.pool)])
                self.counter += 1
            colors[n["row"]] = n["color"]
        self.old = new + extra
        self.frame += 1
        return colors, ious

    def rows(self):
        return [(o["frame"], o["id"], o["label"], int(o["mask"].sum()), o["ttl"], VD.pack_rgb(o["color"])) for o in self.old]


def sequential_matches(iou):
    """the sequential walk on a bare matrix -> the set of matched (live row, new instance) pairs"""
    taken, pairs = set(), set()
    for o, row in enumerate(np.asarray(iou, np.float64)):
        if row.size == 0:
            continue
        j = int(np.argmax(row))
        if row[j] > 0.5 and j not in taken:
            taken.add(j)
            pairs.add((o, j))
    return pairs


def winner_matches(iou):
    choice, winner = VD.match_winners(iou)
    return {(o, j) for o, j in enumerate(choice) if j >= 0 and winner[j] == o}


def run_both(frames, ttl, pool):
    lit, trk = Literal(ttl, pool), VD.ColorTracker(ttl, pool)
    for t, (ids, tab) in enumerate(frames):
        pre = TC.prefill()[:len(tab)]
        want, ious = lit.assign(ids, tab, pre)
        got = trk.assign(ids, tab, pre)
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), t
        assert trk.last_iou.tobytes() == ious.tobytes(), t
        assert [tuple(int(v) for v in r)[:6] for r in trk.live_rows()] == lit.rows(), t
        assert sequential_matches(ious) == winner_matches(ious), t
        assert trk.counter == lit.counter


@pytest.mark.parametrize("name", sorted(CASES))
def test_tracker_equals_the_literal_formulation(name):
    case = CASES[name]
    run_both(case.frames, case.ttl, case.pool)


def random_sequence(rng):
    hw = (int(rng.integers(6, 14)), int(rng.integers(6, 18)))
    things = [(int(i), 1, int(rng.integers(0, 2))) for i in rng.choice(np.arange(2, 12), int(rng.integers(1, 6)), replace=False)]
    pos = {i: (int(rng.integers(0, hw[0] - 3)), int(rng.integers(0, hw[1] - 3))) for i, _, _ in things}
    frames = []
    for _ in range(int(rng.integers(3, 14))):
        rects, rows = [], [TC.STUFF]
        for i, _, cat in things:
            y, x = pos[i]
            pos[i] = (min(max(y + int(rng.integers(-1, 2)), 0), hw[0] - 3), min(max(x + int(rng.integers(-2, 3)), 0), hw[1] - 3))
            if rng.random() < 0.75:
                rects.append((i, y, x, y + int(rng.integers(2, 6)), x + int(rng.integers(2, 7))))
                rows.append((i, 1, cat if rng.random() < 0.9 else 1 - cat))
        order = rng.permutation(len(rows))
        frames.append((TC.paint(hw, rects), TC.table(*[rows[k] for k in order])))
    return frames


def test_tracker_equals_the_literal_formulation_on_random_sequences():
    rng = np.random.default_rng(7)
    for _ in range(300):
        pool = rng.integers(0, 256, (int(rng.integers(1, 6)), 3))
        run_both(random_sequence(rng), int(rng.integers(1, 9)), pool)


def test_winner_form_equals_the_sequential_walk_on_bare_matrices():
    """Also what disjoint masks cannot produce: several entries of a row above 0.5, ties above 0.5."""
    rng = np.random.default_rng(11)
    for _ in range(400):
        iou = rng.choice([0.0, 0.2, 0.5, 0.5000001, 0.6, 0.6, 0.9, 1.0], (int(rng.integers(0, 9)), int(rng.integers(0, 6))))
        assert sequential_matches(iou) == winner_matches(iou)
    # a live row whose best is taken and whose second-best is above 0.5 stays unmatched
    assert winner_matches([[0.9, 0.0], [0.8, 0.7]]) == {(0, 0)} == sequential_matches([[0.9, 0.0], [0.8, 0.7]])
    # an arg-max tie goes to the lower index; row 1 then finds its choice taken
    assert winner_matches([[0.7, 0.7], [0.7, 0.7]]) == {(0, 0)} == sequential_matches([[0.7, 0.7], [0.7, 0.7]])
    # two rows claim one instance: the earlier list position wins
    assert winner_matches([[0.0, 0.6], [0.0, 0.9]]) == {(0, 1)}
    assert winner_matches([[0.5, 0.5]]) == set() and winner_matches(np.zeros((3, 0))) == set()


# ---- the hand-worked expectations ---------------------------------------------------------------------------------------------------------
P = [VD.pack_rgb(c) for c in VD.default_pool()]
ROW = 1                                            # the thing's table row in the one-thing cases


def thing_colors(name, row=ROW):
    return [VD.pack_rgb(f["colors"][row]) for f in TC.expected(CASES[name])]


def live(name, t):
    return [tuple(int(v) for v in r)[:6] for r in TC.expected(CASES[name])[t]["live"]]


def test_a_moving_thing_keeps_its_colour_across_the_ring_wrap():
    for name in ("moving", "moving_square"):
        assert thing_colors(name) == [P[0]] * 12
        for t in range(12):
            assert live(name, t) == [(t, 5, 2, 48, 8, P[0])]
        assert [f["iou"].tolist() for f in TC.expected(CASES[name])[1:]] == [[[40 / 56]]] * 11


def test_iou_of_exactly_one_half_is_no_match():
    assert TC.expected(CASES["iou_half"])[1]["iou"].tolist() == [[0.5]]
    assert thing_colors("iou_half") == [P[0], P[1]]
    assert live("iou_half", 1) == [(1, 5, 2, 6, 8, P[1]), (0, 5, 2, 6, 7, P[0])]
    assert TC.expected(CASES["iou_above_half"])[1]["iou"].tolist() == [[5 / 7]]
    assert thing_colors("iou_above_half") == [P[0], P[0]]
    assert live("iou_above_half", 1) == [(1, 5, 2, 6, 8, P[0])]
    # frame 2 is 5 / 7 from frame 1 and 3 / 9 from frame 0
    assert thing_colors("iou_half_small") == [P[0], P[1], P[1]]
    assert TC.expected(CASES["iou_half_small"])[2]["iou"].tolist() == [[5 / 7], [3 / 9]]


def test_another_category_on_the_same_pixels_is_no_match():
    assert TC.expected(CASES["category"])[1]["iou"].tolist() == [[0.0]]
    assert thing_colors("category") == [P[0], P[1]]


def test_two_claims_go_to_the_earlier_list_position():
    for name in ("two_claim", "two_claim_small"):
        assert TC.expected(CASES[name])[2]["iou"].tolist() == [[32 / 48], [32 / 48]]
        assert thing_colors(name) == [P[0], P[1], P[1]]
        assert live(name, 1) == [(1, 5, 2, 40, 8, P[1]), (0, 5, 2, 40, 7, P[0])]
        assert live(name, 2) == [(2, 5, 2, 40, 8, P[1]), (0, 5, 2, 40, 6, P[0])]


def test_a_row_whose_best_is_taken_stays_unmatched():
    f = TC.expected(CASES["taken_best"])[2]
    assert f["iou"].tolist() == [[32 / 48, 8 / 48], [32 / 48, 0.0]]
    assert [VD.pack_rgb(f["colors"][r]) for r in (1, 2)] == [P[1], P[2]]
    assert live("taken_best", 2) == [(2, 5, 2, 40, 8, P[1]), (2, 6, 2, 16, 8, P[2]), (0, 5, 2, 40, 6, P[0])]


def test_an_argmax_tie_takes_the_first_instance():
    f = TC.expected(CASES["tie"])[1]
    assert f["iou"].tolist() == [[16 / 48, 16 / 48]]
    assert VD.match_winners(f["iou"]) == ([-1], {})
    assert live("tie", 1) == [(1, 9, 2, 16, 8, P[1]), (1, 8, 2, 16, 8, P[2]), (0, 5, 2, 48, 7, P[0])]


@pytest.mark.parametrize("ttl,gap,back", [(8, 7, True), (8, 8, False), (3, 2, True), (3, 3, False), (1, 0, True), (1, 1, False)])
def test_a_colour_returns_within_ttl_frames_and_not_after(ttl, gap, back):
    name = f"gone{gap}_ttl{ttl}"
    got = thing_colors(name)
    pre = VD.pack_rgb(TC.prefill()[ROW])
    assert got == [P[0]] + [pre] * gap + [P[0] if back else P[1]]           # in between the row does not exist: its bytes stay
    if gap:
        assert live(name, gap) == ([(0, 5, 2, 40, ttl - gap, P[0])] if back else [])


def test_an_instance_from_three_frames_back_is_matched_past_a_newer_overlapping_one():
    e = TC.expected(CASES["three_back"])
    assert live("three_back", 3) == [(3, 5, 2, 40, 8, P[2]), (3, 6, 2, 60, 8, P[1]), (0, 5, 2, 40, 5, P[0])]
    assert e[4]["iou"].tolist() == [[20 / 60, 0.0], [0.0, 1.0], [36 / 44, 0.0]]
    assert VD.pack_rgb(e[4]["colors"][1]) == P[0]
    assert live("three_back", 4) == [(4, 5, 2, 40, 8, P[0]), (4, 6, 2, 60, 8, P[1]), (3, 5, 2, 40, 7, P[2])]


def test_the_live_list_fills_to_its_cap_in_order():
    e = TC.expected(CASES["hundred"])
    assert [len(f["live"]) for f in e] == [100, 200, 300, 400, 500, 600, 700] + [800] * 4
    last = e[-1]["live"]
    assert last["frame"].tolist() == [f for f in range(10, 2, -1) for _ in range(100)]
    assert last["id"].tolist() == list(range(1, 101)) * 8
    assert last["ttl"].tolist() == [t for t in range(8, 0, -1) for _ in range(100)]
    assert [VD.pack_rgb(c) for c in e[-1]["colors"]] == [P[(1000 + k) % 74] for k in range(100)]


def test_rows_that_are_no_instances_keep_their_bytes():
    for f in TC.expected(CASES["table_edges"]):
        want = TC.prefill()
        want[1] = VD.default_pool()[0]
        assert f["colors"].tobytes() == want.tobytes()
        assert [tuple(int(v) for v in r)[:4] for r in f["live"]] == [(f["live"]["frame"][0], 5, 2, 40)]


def test_empty_and_all_stuff_frames_cost_one_ttl():
    for name in ("empty_frame", "all_stuff"):
        assert live(name, 1) == [(0, 5, 2, 40, 7, P[0])]
        assert TC.expected(CASES[name])[1]["colors"].tobytes() == TC.prefill().tobytes()
        assert live(name, 2) == [(2, 5, 2, 40, 8, P[0])]


def test_the_pool_counter_wraps():
    e = TC.expected(CASES["pool3"])
    pool = [VD.pack_rgb(c) for c in CASES["pool3"].pool]
    assert [VD.pack_rgb(c) for c in e[0]["colors"][1:6]] == [pool[k % 3] for k in range(5)]
    assert [VD.pack_rgb(c) for c in e[1]["colors"][1:6]] == [pool[(5 + k) % 3] for k in range(5)]
    assert e[2]["colors"].tobytes() == e[1]["colors"].tobytes()


def test_the_long_sequence_keeps_and_renews_colours_as_planned():
    e = TC.expected(CASES["long"])
    tabs = [tab for _, tab in CASES["long"].frames]
    color_of = lambda t, i: VD.pack_rgb(e[t]["colors"][[int(v) for v in tabs[t][:, 0]].index(i)])
    assert len({color_of(t, 10) for t in range(20)}) == 1                              # always matched
    assert color_of(11, 11) == color_of(5, 11)                                         # back after five frames
    assert color_of(13, 12) != color_of(12, 12) and color_of(14, 12) == color_of(12, 12) != color_of(13, 12)
    assert color_of(3, 13) == color_of(10, 13) == color_of(17, 13)                     # six frames away each time: inside ttl 8


def test_size_change_reset_and_bad_arguments():
    trk = VD.ColorTracker(pool=[(1, 2, 3)])
    ids, tab = TC.band((8, 20), 2, 9)
    first = trk.assign(ids, tab)
    assert first[1].tolist() == [1, 2, 3] and first[0].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        trk.assign(np.zeros((8, 21), np.int32), tab)
    trk.reset()
    assert trk.live == [] and trk.counter == 0 and trk.frame == 0
    trk.assign(np.zeros((8, 21), np.int32), tab)                                        # after a reset another size is fine
    for bad in (0, 9):
        with pytest.raises(ValueError):
            VD.ColorTracker(ttl=bad)
    with pytest.raises(ValueError):
        VD.ColorTracker(pool=np.zeros((0, 3), np.uint8))
    assert VD.default_pool().shape == (74, 3) and VD.TRACK_ROW_DTYPE.itemsize == 32


def test_draw_panoptic_seg_predictions_is_draw_panoptic_seg_with_the_trackers_colours():
    from odise_amd import visualize as V
    case = CASES["moving"]
    trk, twin = VD.ColorTracker(), VD.ColorTracker()
    image = np.random.default_rng(3).integers(0, 256, case.hw + (3,)).astype(np.uint8)
    for ids, tab in case.frames[:3]:
        got = VD.draw_panoptic_seg_predictions(image, ids, tab, trk, None, labels=False)
        colors = twin.assign(ids, tab, V.segment_colors(tab, None))
        assert colors[0].tolist() == V.segment_colors(tab, None)[0].tolist()             # stuff keeps its colour
        assert got.tobytes() == V.panoptic_overlay(image, ids, tab, colors).tobytes()
    assert VD.draw_panoptic_seg_predictions(image, *case.frames[3], trk).shape == image.shape


# ---- the demo's video arguments and frame sources ------------------------------------------------------------------------------------------
def test_demo_video_arguments():
    args = demo.parse_args(["--video-input", "clip", "--output", "out", "--vocab", "a; b", "--synthetic"])
    assert args.video_input == "clip" and args.input is None and args.ttl == 8 and args.task == "panoptic"
    assert demo.parse_args(["--video-input", "clip", "--output", "out.gif", "--ttl", "3", "--task", "semantic"]).ttl == 3
    assert demo.parse_args(["--input", "a.jpg", "--output", "out"]).video_input is None
    for bad in (["--output", "out"], ["--input", "a.jpg", "--video-input", "clip", "--output", "out"],
                ["--video-input", "clip", "--output", "out", "--ttl", "9"], ["--video-input", "clip", "--output", "out", "--ttl", "0"]):
        with pytest.raises(SystemExit):
            demo.parse_args(bad)
    assert demo.frame_path("out", 7) == os.path.join("out", "frame_000007.png")


def test_demo_refuses_instances_on_video(capsys):
    with pytest.raises(SystemExit) as e:
        demo.parse_args(["--video-input", "clip", "--output", "out", "--task", "instance"])
    assert e.value.code != 0 and "pred_boxes" in capsys.readouterr().err
    assert demo.parse_args(["--input", "a.jpg", "--output", "out", "--task", "instance"]).task == "instance"


class FakeCtx:
    def to_device(self, a):
        return a


def test_demo_frame_sources(tmp_path, monkeypatch):
    from PIL import Image
    rng = np.random.default_rng(5)
    d = tmp_path / "frames"
    d.mkdir()
    for name in ("b_2.png", "a_10.png", "a_02.png"):
        Image.fromarray(rng.integers(0, 256, (6, 8, 3)).astype(np.uint8)).save(d / name)
    monkeypatch.setattr(demo, "read_picture", lambda ctx, path: path)
    frames = demo.video_frames(str(d))
    assert [os.path.basename(n) for n, _ in frames] == ["a_02.png", "a_10.png", "b_2.png"]            # sorted by name
    assert [load(None) for _, load in frames] == [n for n, _ in frames]
    pictures = [np.full((6, 8, 3), 40 * k, np.uint8) for k in range(4)]
    gif = str(tmp_path / "clip.gif")
    Image.fromarray(pictures[0]).save(gif, save_all=True, append_images=[Image.fromarray(p) for p in pictures[1:]], duration=50, loop=0)
    frames = demo.video_frames(gif)
    assert [n for n, _ in frames] == [f"{gif}#{k}" for k in range(4)]
    for (_, load), want in zip(frames, pictures):
        got = load(FakeCtx())
        assert got.dtype == np.uint8 and got.shape == (6, 8, 3) and np.array_equal(got, want)


def test_run_on_video_refuses_a_frame_of_another_size_by_name(monkeypatch):
    class Arr:
        def __init__(self, hw):
            self.shape = hw + (3,)
    monkeypatch.setattr(demo, "run_on_image", lambda ctx, model, vis, image, task, video=False: ("drawn", image.shape, video))
    frames = [("f0", lambda ctx: Arr((4, 6))), ("f1", lambda ctx: Arr((4, 6))), ("f2", lambda ctx: Arr((4, 7)))]
    it = demo.run_on_video(None, None, None, frames)
    assert next(it) == ("drawn", (4, 6, 3), True) and next(it) == ("drawn", (4, 6, 3), True)
    with pytest.raises(SystemExit) as e:
        next(it)
    assert "f2" in str(e.value)
