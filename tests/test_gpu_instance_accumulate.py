"""GPU: odise_hip_instance_accumulate (csrc/inst_accum.hip, csrc/radix_sort.h) against instance_eval.accumulate, byte for byte, on the inputs
of tests/accum_cases.py; the flags; `HipInstanceSegEvaluator.evaluate` on the device and on the host."""
import math

import numpy as np
import pytest
import torch

import accum_cases as AC
import inst_cases as IC
from odise_amd import instance_eval as IE
from odise_amd.instance_seg_eval import HipInstanceSegEvaluator
from odise_amd.runtime import InstanceAccumulateError
from small_model import GROUPS, build_small, image_u8

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.mark.parametrize("name", AC.VALID)
def test_device_equals_the_host_function_byte_for_byte(ctx, name):
    c = AC.case(name)
    blocks = [(ctx.to_device(r), ctx.to_device(n)) for r, n in c["blocks"]]
    p, r = ctx.instance_accumulate(blocks, c["npig"], c["K"], AC.TOPK)
    assert p.shape == c["want"][0].shape and r.shape == c["want"][1].shape
    bad = np.argwhere(p != c["want"][0])
    assert p.tobytes() == c["want"][0].tobytes(), (len(bad), bad[:5].tolist(), [float(p[tuple(b)]) for b in bad[:5]],
                                                   [float(c["want"][0][tuple(b)]) for b in bad[:5]])
    assert r.tobytes() == c["want"][1].tobytes(), np.argwhere(r != c["want"][1])[:5].tolist()
    p2, r2 = ctx.instance_accumulate(blocks, c["npig"], c["K"], AC.TOPK)
    assert p2.tobytes() == p.tobytes() and r2.tobytes() == r.tobytes()


@pytest.mark.parametrize("name", AC.FLAGGED)
def test_flags_raise_and_leave_minus_one(ctx, name):
    c = AC.case(name)
    with pytest.raises(InstanceAccumulateError) as e:
        ctx.instance_accumulate(c["blocks"], c["npig"], c["K"], AC.TOPK)
    assert e.value.flags == c["flag"] and IE.ACCUM_FLAG_NAMES[c["flag"]] in str(e.value)
    assert e.value.precision.shape == (10, 101, c["K"], 4, 3) and (e.value.precision == -1).all() and (e.value.recall == -1).all()
    # the context is as good as before
    ok = AC.case("one_category")
    p, r = ctx.instance_accumulate(ok["blocks"], ok["npig"], ok["K"], AC.TOPK)
    assert p.tobytes() == ok["want"][0].tobytes() and r.tobytes() == ok["want"][1].tobytes()


def test_limits_are_checked_and_nothing_is_written(ctx):
    c = AC.case("one_category")
    wide = [(np.zeros(101, IE.ROW_DTYPE), np.zeros(1, np.int32))]
    for kw, blocks in ((dict(topk=101), wide), (dict(topk=AC.TOPK, rec_thrs=np.linspace(0, 1, 102)), c["blocks"])):
        with pytest.raises(RuntimeError, match="instance_accumulate"):
            ctx.instance_accumulate(blocks, c["npig"], 1, **kw)
    # another table of recall thresholds, and a short slot size
    thr = IE.REC_THRS[[0, 30, 30, 90, 100]]
    rows = AC.compact(c["blocks"])[:17]
    rows["image"] = np.arange(17) // 4
    out, counts = HipInstanceSegEvaluator.slots_of(rows, 4)
    p, r = ctx.instance_accumulate([(out, counts)], c["npig"], 1, 4, rec_thrs=thr)
    want = IE.accumulate(rows, c["npig"], 1)
    assert r.tobytes() == want[1].tobytes() and p.shape == (10, 5, 1, 4, 3)
    assert (p[:, [0, 1, 3, 4]] == want[0][:, [0, 30, 90, 100]]).all() and (p[:, 1] == p[:, 2]).all()


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    return build_small(ctx)


def _same(a: dict, b: dict):
    assert set(a) == set(b)
    for k in a:
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def test_evaluator_on_the_device_and_on_the_host(small, ctx, monkeypatch):
    hip, K = small, len(GROUPS)
    names = [f"class{k}" for k in range(K)]
    ev = HipInstanceSegEvaluator(ctx, {k: k for k in range(K)}, names, topk=int(hip.test_topk_per_image))
    ev.CHUNK = 2                                                            # three pictures cross a block of the row buffer
    ev.reset()
    hip.keep_instance_selection = True
    kept = []
    try:
        for i, (h, w) in enumerate(((320, 448), (256, 256), (300, 302))):
            inst = hip.forward([{"image": image_u8(h, w, seed=70 + i)}])[0]["instances"]
            m, cls = inst["pred_masks"] > 0.5, inst["pred_classes"]
            anns = [IC.ann(np.roll(m[j], 2 + j, axis=1), int(cls[j])) for j in range(min(6, len(m)))] + [IC.ann(m[0] | m[1], int(cls[1]), iscrowd=1)]
            kept.append((hip.last_selection, anns))
            ev.process_selection(hip.last_selection, [anns], [5 - i])      # descending image numbers
    finally:
        hip.keep_instance_selection = False
    calls = []
    real = ctx.instance_accumulate
    monkeypatch.setattr(ctx, "instance_accumulate", lambda *a, **k: calls.append(1) or real(*a, **k))
    dev = ev.evaluate(accumulate_on="device")
    p, r = ev.precision, ev.recall
    assert calls == [1]
    host = ev.evaluate(accumulate_on="host")
    assert calls == [1]
    _same(dev, host)
    assert p.tobytes() == ev.precision.tobytes() and r.tobytes() == ev.recall.tobytes()
    assert not math.isnan(dev["AP"]) and dev["AP"] > 0
    _same(ev.evaluate(), dev)
    assert calls == [1, 1]
    # a repeated image number: the host path, whatever was asked
    sel, anns = kept[-1]
    ev.process_selection(sel, [anns], [5])
    again = ev.evaluate(accumulate_on="device")
    assert calls == [1, 1]
    _same(again, IE.results(*IE.accumulate(ev.rows(), ev._npig, K), names))
