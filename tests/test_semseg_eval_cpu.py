"""CPU: odise_amd/semseg_eval.py, the host restatement of SemSegEvaluator (encode_json_sem_seg, the arithmetic of evaluate(), the exchange
step at world size 2 over gloo)."""
import math
import os
import socket

import numpy as np
import pytest

from odise_amd import coco_rle
from odise_amd import semseg_eval as SE
from semseg_cases import CASES


@pytest.mark.parametrize("name", sorted(CASES))
def test_encode_json_sem_seg_partitions_the_picture(name):
    case = CASES[name]
    rows = SE.encode_json_sem_seg(case.labels, "a/b.png")
    ids = [r["category_id"] for r in rows]
    assert ids == sorted(set(int(v) for v in case.labels.reshape(-1)))               # np.unique's order: ascending, each label once
    assert all(r["file_name"] == "a/b.png" and r["segmentation"]["size"] == list(case.hw) for r in rows)
    cover = np.zeros(case.hw, np.int32)
    for r in rows:
        m = coco_rle.decode(r["segmentation"])
        assert np.array_equal(m.astype(bool), case.labels == r["category_id"])
        cover += m
    assert (cover == 1).all()                                                         # every pixel lies in exactly one class
    classes, strings, area = case.expected()                                          # the labels in [0, K) of the same map
    kept = [r for r in rows if 0 <= r["category_id"] < case.K]
    assert [r["category_id"] for r in kept] == classes.tolist() and [r["segmentation"]["counts"] for r in kept] == strings
    assert [coco_rle.area(r["segmentation"]) for r in kept] == area.tolist() and int(area.sum()) == int(case.valid().sum())


def test_encode_json_sem_seg_applies_the_mapping_and_rejects_a_label_outside_it():
    case = CASES["five_of_max2_K150"]
    mapping = {c: 1000 + 3 * c for c in range(150)}
    rows = SE.encode_json_sem_seg(case.labels, "x", mapping)
    assert [r["category_id"] for r in rows] == [1000 + 3 * c for c in (7, 37, 67, 97, 127)]
    plain = SE.encode_json_sem_seg(case.labels, "x")
    assert [r["segmentation"] for r in rows] == [r["segmentation"] for r in plain]
    del mapping[67]
    with pytest.raises(AssertionError):
        SE.encode_json_sem_seg(case.labels, "x", mapping)
    with pytest.raises(AssertionError):
        SE.encode_json_sem_seg(CASES["bad_minus1_K150"].labels, "x", {c: c for c in range(150)})


# rows = prediction, columns = ground truth, the last row / column = the ignore label (never predicted: its row is zero)
CONF = np.array([[6, 1, 0, 2],     # predicted 0: 6 right, 1 of gt 1, 2 ignored pixels
                 [2, 3, 0, 1],     # predicted 1
                 [1, 0, 0, 4],     # predicted 2: a class that is predicted but never in the ground truth
                 [0, 0, 0, 0]], np.int64)
B_CONF = np.array([[50, 2, 0, 1],
                   [3, 4, 0, 0],
                   [0, 0, 0, 0],   # class 2 has no boundary pixel on either side: its Boundary IoU is NaN
                   [0, 0, 0, 0]], np.int64)


def test_results_against_hand_worked_matrices():
    res = SE.results(CONF, B_CONF, ["a", "b", "c"])
    # pos_gt = (9, 4, 0), pos_pred = (7, 5, 1), tp = (6, 3, 0): the ignore column and row take no part
    iou_a, iou_b = 6 / (9 + 7 - 6), 3 / (4 + 5 - 3)
    acc_a, acc_b = 6 / 9, 3 / 4
    assert res["IoU-a"] == 100 * iou_a and res["IoU-b"] == 100 * iou_b and math.isnan(res["IoU-c"])
    assert res["ACC-a"] == 100 * acc_a and res["ACC-b"] == 100 * acc_b and math.isnan(res["ACC-c"])
    assert res["mIoU"] == pytest.approx(100 * (iou_a + iou_b) / 2, rel=1e-15)          # class c is left out of both means
    assert res["mACC"] == pytest.approx(100 * (acc_a + acc_b) / 2, rel=1e-15)
    assert res["fwIoU"] == pytest.approx(100 * (iou_a * 9 / 13 + iou_b * 4 / 13), rel=1e-15)
    assert res["pACC"] == pytest.approx(100 * 9 / 13, rel=1e-15)
    # boundary: b_pos_gt = (53, 6, 0), b_pos_pred = (52, 7, 0), b_tp = (50, 4, 0)
    b_a, b_b = 50 / (53 + 52 - 50), 4 / (6 + 7 - 4)
    assert res["BoundaryIoU-a"] == 100 * b_a and res["BoundaryIoU-b"] == 100 * b_b and math.isnan(res["BoundaryIoU-c"])
    assert res["min(IoU, B-Iou)-a"] == 100 * min(iou_a, b_a) and res["min(IoU, B-Iou)-b"] == 100 * min(iou_b, b_b)
    assert math.isnan(res["min(IoU, B-Iou)-c"])
    assert list(res) == ["mIoU", "fwIoU", "IoU-a", "BoundaryIoU-a", "min(IoU, B-Iou)-a", "IoU-b", "BoundaryIoU-b", "min(IoU, B-Iou)-b",
                         "IoU-c", "BoundaryIoU-c", "min(IoU, B-Iou)-c", "mACC", "pACC", "ACC-a", "ACC-b", "ACC-c"]


def test_results_without_boundary_and_a_class_in_gt_that_is_never_predicted():
    conf = np.array([[5, 2, 3, 0],
                     [0, 0, 0, 0],     # class b is in the ground truth (2 pixels) and never predicted: IoU 0, ACC 0, both valid
                     [1, 0, 4, 9],
                     [0, 0, 0, 0]], np.int64)
    res = SE.results(conf, None, ["a", "b", "c"])
    assert list(res) == ["mIoU", "fwIoU", "IoU-a", "IoU-b", "IoU-c", "mACC", "pACC", "ACC-a", "ACC-b", "ACC-c"]
    iou = [5 / (6 + 10 - 5), 0.0, 4 / (7 + 5 - 4)]
    assert [res["IoU-a"], res["IoU-b"], res["IoU-c"]] == [100 * v for v in iou]
    assert [res["ACC-a"], res["ACC-b"], res["ACC-c"]] == [100 * (5 / 6), 0.0, 100 * (4 / 7)]
    assert res["mIoU"] == pytest.approx(100 * sum(iou) / 3, rel=1e-15) and res["pACC"] == pytest.approx(100 * 9 / 15, rel=1e-15)
    assert res["fwIoU"] == pytest.approx(100 * (iou[0] * 6 + iou[2] * 7) / 15, rel=1e-15)


def test_result_key_gets_the_underscore_of_the_wrapper():
    assert SE.result_key("ade20k_sem_seg_val") == "ade20k_sem_seg_val/sem_seg"
    assert SE.result_key("d", "open") == "d/open_sem_seg" and SE.result_key("d", "open_") == "d/open_sem_seg"


def test_confusion_restatement_equals_the_oracle_on_mapped_ground_truth():
    from oracle.eval_ops import semantic_confusion
    rng = np.random.default_rng(2)
    sem = rng.standard_normal((4, 9, 11)).astype(np.float32)
    gt = rng.integers(0, 5, (9, 11))
    assert np.array_equal(SE.confusion(sem.argmax(0), gt, 4), semantic_confusion(sem, gt, ignore_label=255))
    gt255 = np.where(gt == 4, 255, gt)
    assert np.array_equal(SE.confusion(sem.argmax(0), gt255, 4), semantic_confusion(sem, gt255, ignore_label=255))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_inputs(rank):
    rng = np.random.default_rng(40 + rank)
    conf, b_conf = rng.integers(0, 1000, (4, 4)), rng.integers(0, 1000, (4, 4))
    rows = [{"file_name": f"rank{rank}_{i}", "category_id": i, "segmentation": {"size": [1, 1], "counts": "1"}} for i in range(2 + rank)]
    return conf.astype(np.int64), b_conf.astype(np.int64), rows, 0


def _gather_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    conf, b_conf, rows, flags = _rank_inputs(rank)
    with_b = SE.gather(conf, b_conf, rows, flags)
    without = SE.gather(conf, None, rows, rank)                                       # rank 1 saw flag 1: every rank must see it
    q.put((rank, (with_b[0].copy(), with_b[1].copy(), with_b[2], with_b[3], without[0].copy(), without[1], without[3])))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_sums_the_matrices_and_keeps_the_rows_in_rank_order_gloo_world2():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ins = [_rank_inputs(r) for r in range(world)]
    for r in range(world):
        conf, b_conf, rows, flags, conf2, none, flags2 = got[r]
        assert np.array_equal(conf, ins[0][0] + ins[1][0]) and np.array_equal(b_conf, ins[0][1] + ins[1][1]) and conf.dtype == np.int64
        assert rows == ins[0][2] + ins[1][2] and flags == 0
        assert np.array_equal(conf2, conf) and none is None and flags2 == 1
    one = SE.gather(*ins[0])                                                          # no process group: the arguments as they are
    assert one[0] is ins[0][0] and one[2] is ins[0][2]
