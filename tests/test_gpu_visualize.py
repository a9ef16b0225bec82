"""GPU: odise_hip_connected_components / odise_hip_segment_anchors / odise_hip_panoptic_overlay (csrc/vis.hip) against the numpy
restatement odise_amd.visualize on the case set of tests/vis_cases.py.  Everything is integers and bytes: all comparisons are exact, and
every call is made twice and must give the same bytes."""
import ctypes as C

import numpy as np
import pytest

from odise_amd import visualize as V
from odise_amd._lib import MAX_SEGMENTS, AnchorDesc, OverlayDesc
from record_helpers import upload_record
from vis_cases import cases, hand_cases

pytestmark = pytest.mark.gpu

CASES = cases()
GUARD = 3          # anchor rows behind `cap` that must stay as they were


def device_anchors(ctx, case, cap=64, unaligned=False):
    _, ids, table = upload_record(ctx, case.record(), case.hw, unaligned)
    rows = []
    for _ in range(2):
        guard = np.zeros(cap + GUARD, V.ANCHOR_DTYPE)
        guard["segment_row"], guard["area"] = -5, -6
        buf = ctx.to_device(guard)
        _, n = ctx.segment_anchors(ids, table, case.small_area, case.large_area, cap, anchors=buf)
        rows.append((buf.numpy(), int(n.numpy()[0])))
        assert rows[-1][0][cap:].tobytes() == guard[cap:].tobytes(), "rows behind cap were written"
    assert rows[0][1] == rows[1][1] and rows[0][0].tobytes() == rows[1][0].tobytes(), "not the same from run to run"
    return rows[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_connected_components(ctx, name):
    case = CASES[name]
    labels = ctx.to_device(case.ids)
    first = ctx.connected_components(labels).numpy()
    second = ctx.connected_components(labels).numpy()
    print(name, case.hw, "components", len(np.unique(case.roots())), "differing", int((first != case.roots()).sum()))
    assert first.tobytes() == case.roots().tobytes()
    assert second.tobytes() == first.tobytes()


def test_connected_components_with_negative_labels_and_an_unaligned_map(ctx):
    case = CASES["ragged"]
    ids = case.ids.copy()
    ids[ids == 2] = -3                                           # VOID like 0
    buf = ctx.to_device(np.concatenate([np.zeros(1, np.int32), ids.reshape(-1)]))
    got = ctx.connected_components(buf.view(ids.shape, np.int32, 4)).numpy()
    assert np.array_equal(got, V.connected_roots(ids)) and (got[ids < 0] == -1).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_anchors(ctx, name):
    case = CASES[name]
    want = case.anchors()
    got, n = device_anchors(ctx, case)
    print(name, "anchors", n, got[:n].tolist())
    assert n == len(want) <= 64
    assert got[:n].tobytes() == want.tobytes()


def test_hand_worked_pictures_on_the_device(ctx):
    for case, want in hand_cases():
        got, n = device_anchors(ctx, case)
        assert [tuple(int(v) for v in a) for a in got[:n]] == want, case.name


def test_more_anchors_than_cap(ctx):
    case = CASES["many_anchors"]
    want = case.anchors()
    for cap in (0, 1, 5, 31, 32):
        got, n = device_anchors(ctx, case, cap)
        assert n == len(want) == 32
        assert got[:cap].tobytes() == want[:cap].tobytes(), cap


def test_anchors_of_a_record_that_is_not_16_byte_aligned(ctx):
    for name in ("ragged", "thresholds"):
        got, n = device_anchors(ctx, CASES[name], unaligned=True)
        assert got[:n].tobytes() == CASES[name].anchors().tobytes()


def device_overlay(ctx, case, alpha256=128, edge=(255, 255, 255), in_place=False, unaligned=False):
    _, ids, table = upload_record(ctx, case.record(), case.hw, unaligned)
    h, w = case.hw
    image, colors = case.image(), ctx.to_device(case.colors())
    off = 1 if unaligned else 0
    outs = []
    for _ in range(2):
        src = ctx.to_device(np.concatenate([np.full(off, 9, np.uint8), image.reshape(-1)]))
        dst = src if in_place else ctx.to_device(np.full(off + image.size + 5, 77, np.uint8))
        ctx.panoptic_overlay(src.view((h, w, 3), np.uint8, off), ids, table, colors, alpha256, edge, out=dst.view((h, w, 3), np.uint8, off))
        outs.append(dst.numpy())
        assert (outs[-1][:off] == (9 if in_place else 77)).all()
        if not in_place:
            assert (outs[-1][off + image.size:] == 77).all(), "bytes behind the picture were written"
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0][off:off + image.size].reshape(h, w, 3)


@pytest.mark.parametrize("name", sorted(CASES))
def test_overlay(ctx, name):
    case = CASES[name]
    got = device_overlay(ctx, case)
    assert got.tobytes() == case.overlay().tobytes()


@pytest.mark.parametrize("alpha256", [0, 256])
@pytest.mark.parametrize("in_place,unaligned", [(False, False), (True, False), (False, True), (True, True)])
def test_overlay_options(ctx, alpha256, in_place, unaligned):
    for name in ("ragged", "mismatch"):
        case = CASES[name]
        edge = (1, 2, 250)
        got = device_overlay(ctx, case, alpha256, edge, in_place, unaligned)
        assert got.tobytes() == case.overlay(alpha256, edge).tobytes(), name
    known = np.isin(CASES["mismatch"].ids, [s[0] for s in CASES["mismatch"].segments])
    assert (got[~known] == CASES["mismatch"].image()[~known]).all()          # VOID and ids without a row are untouched


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    case = CASES["thresholds"]
    h, w = case.hw
    _, ids, table = upload_record(ctx, case.record(), case.hw)
    lib = ctx.lib
    roots = ctx.to_device(np.full((h, w), -9, np.int32))
    assert lib.odise_hip_connected_components(ctx.h, None, h, w, roots.ptr) == -1
    assert lib.odise_hip_connected_components(ctx.h, ids.ptr, h, w, None) == -1
    assert lib.odise_hip_connected_components(ctx.h, ids.ptr, 0, w, roots.ptr) == -1
    assert lib.odise_hip_connected_components(ctx.h, ids.ptr, 1 << 15, 1 << 14, roots.ptr) == -1       # 2^29 pixels
    rows = ctx.to_device(np.full(4 * 8, -1, np.int32).view(V.ANCHOR_DTYPE))
    count = ctx.to_device(np.full(1, -4, np.int32))

    def anchor_desc(**kw):
        d = AnchorDesc()
        d.H, d.W, d.pred_ids, d.pred_segments, d.small_area, d.large_area, d.anchors, d.cap, d.n_anchors = h, w, ids.ptr, table.ptr, 4, 50, rows.ptr, 4, count.ptr
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw in ({"pred_ids": None}, {"pred_segments": None}, {"anchors": None}, {"n_anchors": None}, {"cap": -1}, {"H": 0}, {"W": -3},
               {"H": 1 << 15, "W": 1 << 14}):
        assert lib.odise_hip_segment_anchors(ctx.h, C.byref(anchor_desc(**kw))) == -1, kw
    assert lib.odise_hip_segment_anchors(ctx.h, None) == -1
    image = ctx.to_device(case.image())
    out = ctx.to_device(np.full((h, w, 3), 55, np.uint8))
    colors = ctx.to_device(case.colors())

    def overlay_desc(**kw):
        d = OverlayDesc()
        d.H, d.W, d.image, d.pred_ids, d.pred_segments, d.colors, d.alpha256, d.out = h, w, image.ptr, ids.ptr, table.ptr, colors.ptr, 128, out.ptr
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw in ({"image": None}, {"pred_ids": None}, {"pred_segments": None}, {"colors": None}, {"out": None}, {"alpha256": -1}, {"alpha256": 257},
               {"H": 0}, {"H": 1 << 15, "W": 1 << 14}):
        assert lib.odise_hip_panoptic_overlay(ctx.h, C.byref(overlay_desc(**kw))) == -1, kw
    assert lib.odise_hip_panoptic_overlay(ctx.h, None) == -1
    ctx.sync()
    assert (roots.numpy() == -9).all() and (rows.numpy().view(np.int32) == -1).all() and count.numpy()[0] == -4 and (out.numpy() == 55).all()
    assert lib.odise_hip_segment_anchors(ctx.h, C.byref(anchor_desc())) == 0 and lib.odise_hip_panoptic_overlay(ctx.h, C.byref(overlay_desc())) == 0
    ctx.sync()
    assert count.numpy()[0] == len(case.anchors())


def test_the_models_own_record_is_drawn_as_the_restatement_draws_it(ctx):
    """odise_hip_infer (small model, panoptic_on) writes its record into a caller-owned buffer; HipVisualizer draws from that buffer and
    must return what the restatement makes of the record read back."""
    from small_model import GROUPS, THINGS, build_small, image_u8
    hip = build_small(ctx, semantic_on=False, instance_on=False)
    h, w = 192, 256                                    # the size the result is asked for; the network sees 512 x 512
    big = np.ascontiguousarray(image_u8(512, 512, seed=3).numpy())
    chw = np.ascontiguousarray(big[:, :2 * h:2, ::2])
    rec = ctx.empty((h * w + 1 + 3 * MAX_SEGMENTS,), np.int32)
    hip.infer_device([ctx.to_device(big)], 1, [(512, 512)], [(h, w)], pan_out=[rec])
    names = [f"class {c}" for c in range(len(GROUPS))]
    md = {"stuff_classes": names, "thing_classes": names, "stuff_colors": [(10 * c, 255 - 20 * c, 40 + c) for c in range(len(GROUPS))],
          "thing_colors": [(255 - 9 * c, 30 + c, 11 * c) for c in range(len(GROUPS))], "thing_ids": sorted(THINGS)}
    hwc = np.ascontiguousarray(chw.transpose(1, 2, 0))
    vis = V.HipVisualizer(ctx, md, alpha=0.5, small_area=50, large_area=2000)
    got = vis.draw_panoptic_seg(ctx.to_device(hwc), rec, (h, w))
    host = rec.numpy()
    n = int(host[h * w])
    assert n >= 1
    segments = host[h * w + 1:h * w + 1 + 3 * n].reshape(n, 3)
    want = V.draw_panoptic_seg(hwc, host[:h * w].reshape(h, w), segments, md, 128, (0, 0, 0), 50, 2000)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert got.tobytes() == want.tobytes()
    assert (got != hwc).any()
