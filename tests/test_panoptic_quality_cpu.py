"""CPU: the host restatement of the panoptic quality statistics (odise_amd/panoptic_quality.py) - hand-built pictures with known answers,
random pictures against an independent dense formulation (tests/pq_cases.py), the metric arithmetic - and the cross-rank sum
(odise_amd.distributed.sum_pq_stats) over gloo at world size 2."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from odise_amd import distributed as D
from odise_amd import panoptic_quality as PQ
from pq_cases import blocky_case, dense_stats, expected_stats, hand_cases

HAND = hand_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_pictures(name):
    case = HAND[name]
    stats, flags = case.stats()
    assert flags == case.flags
    assert stats == expected_stats(case), (stats, expected_stats(case))
    dense, dflags = dense_stats(case)
    assert dflags == flags and dense == stats


def test_hand_built_pictures_say_what_they_claim():
    assert HAND["perfect"].stats()[0].iou[1] == 1.0
    # exactly 0.5, twice: the candidate is rejected, and the crowd region does not absorb pred 8
    tr = {}
    HAND["iou_exactly_half"].stats(tr)
    assert tr == dict(rejected=1, skipped_void=0, skipped_crowd=0)
    HAND["crowd"].stats(tr)
    assert tr["skipped_crowd"] == 1 and HAND["crowd"].stats()[0].fp[1] == 1
    HAND["last_crowd_wins_swapped"].stats(tr)
    assert tr["skipped_crowd"] == 1
    HAND["prediction_in_void"].stats(tr)
    assert tr["skipped_void"] == 1
    # the flagged pictures would count something if they were not flagged
    for name, fix in (("flag_missing_id", dict(pan_pred=[9, 9, 9, 9])), ("flag_empty_row", dict(pred_rows=[(9, 1, 1)])),
                      ("flag_bad_category", dict(pred_rows=[(9, 1, 1)]))):
        c = HAND[name]
        args = dict(pan_gt=c.pan_gt, gt_segments=c.gt_rows, pan_pred=c.pan_pred, pred_segments=c.pred_rows, C=c.C)
        args.update({("pred_segments" if k == "pred_rows" else k): v for k, v in fix.items()})
        stats, flags = PQ.image_stats(**args)
        assert flags == 0 and stats.tp[1] == 1


# (seed, h, w, n_gt, n): the pictures of the device tests and a few more
RANDOM = [(1, 67, 131, 37, 20), (2, 200, 333, 37, 100), (3, 200, 333, 254, 100), (4, 200, 333, 1, 1), (5, 200, 333, 0, 100), (6, 200, 333, 254, 0),
          (7, 5, 7, 3, 2), (8, 1, 1, 1, 1), (9, 96, 160, 30, 20), (10, 64, 64, 12, 7), (11, 512, 512, 37, 20), (12, 200, 333, 37, 20)]


@pytest.mark.parametrize("seed,h,w,n_gt,n", RANDOM)
def test_restatement_equals_dense_formulation(seed, h, w, n_gt, n):
    case = blocky_case(seed, h, w, n_gt, n)
    stats, flags = case.stats()
    dense, dflags = dense_stats(case)
    assert flags == dflags == 0
    assert np.array_equal(stats.tp, dense.tp) and np.array_equal(stats.fp, dense.fp) and np.array_equal(stats.fn, dense.fn)
    assert stats.iou.tobytes() == dense.iou.tobytes()           # both add in ascending (g, p) order
    if min(h, w) >= 64 and n_gt >= 12 and n >= 7:                # the generator makes every rule fire on a picture with room for it
        case.assert_every_rule_fires()


def test_a_stream_of_pictures_adds_pair_by_pair():
    cases = [blocky_case(s, h, w, n_gt, n) for s, h, w, n_gt, n in RANDOM[:3]]
    acc = PQ.PQStats(6)
    for c in cases:
        out, flags = c.stats(into=acc)
        assert out is acc and flags == 0
    totals = [c.stats()[0] for c in cases]
    assert np.array_equal(acc.tp, sum(t.tp for t in totals)) and np.array_equal(acc.fn, sum(t.fn for t in totals))
    np.testing.assert_allclose(acc.iou, sum(t.iou for t in totals), rtol=1e-14)
    before = acc.to_records().tobytes()
    HAND["flag_missing_id"].stats(into=(small := PQ.PQStats(3)))
    assert not small.to_records().view(np.uint8).any() and acc.to_records().tobytes() == before


def test_rgb2id():
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (9, 11, 3)).astype(np.uint8)
    rgb[0, 0], rgb[0, 1] = (255, 255, 255), (1, 0, 0)
    ids = PQ.rgb2id(rgb)
    assert ids.dtype == np.int32 and ids[0, 0] == 2 ** 24 - 1 and ids[0, 1] == 1
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    np.testing.assert_array_equal(ids, r + 256 * g + 65536 * b)
    case = HAND["crowd"]
    np.testing.assert_array_equal(PQ.rgb2id(case.rgb()), case.pan_gt)


def test_pq_average_and_results_on_a_hand_computed_table():
    # category: 0 thing (iou 1.5, tp 2, fp 1, fn 1), 1 thing without samples, 2 stuff (tp 0, fp 2), 3 stuff (iou 0.8, tp 1)
    s = PQ.PQStats(4)
    s.iou[:], s.tp[:], s.fp[:], s.fn[:] = [1.5, 0.0, 0.0, 0.8], [2, 0, 0, 1], [1, 0, 2, 0], [1, 0, 0, 0]
    isthing = [True, True, False, False]
    th = PQ.pq_average(s, isthing, "things")
    assert th == {"pq": 1.5 / 3, "sq": 0.75, "rq": 2 / 3, "n": 1}                 # category 1 has no sample: not in n
    st = PQ.pq_average(s, isthing, "stuff")
    assert st == {"pq": (0.0 + 0.8) / 2, "sq": (0 + 0.8) / 2, "rq": (0.0 + 1.0) / 2, "n": 2}   # tp = 0: sq 0, pq 0, rq 0
    al = PQ.pq_average(s, isthing, "all")
    assert al["n"] == 3 and al["pq"] == (0.5 + 0.0 + 0.8) / 3 and al["sq"] == (0.75 + 0 + 0.8) / 3 and al["rq"] == (2 / 3 + 0.0 + 1.0) / 3
    res = PQ.results(s, isthing)
    assert sorted(res) == sorted(["PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st"])
    assert res["PQ"] == 100 * al["pq"] and res["SQ_th"] == 100 * 0.75 and res["RQ_st"] == 100 * 0.5 and res["PQ_st"] == 100 * 0.4
    assert PQ.pq_average(PQ.PQStats(4), isthing, "all") == {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}


def test_pqstats_addition_and_records():
    a, _ = blocky_case(9, 96, 160, 30, 20).stats()
    b, _ = blocky_case(10, 64, 64, 12, 7).stats()
    c = a + b
    assert np.array_equal(c.tp, a.tp + b.tp) and np.array_equal(c.fp, a.fp + b.fp) and np.array_equal(c.fn, a.fn + b.fn)
    assert c.iou.tobytes() == (a.iou + b.iou).tobytes()
    acc = PQ.PQStats(len(a))
    acc += a
    acc += b
    assert acc == c and not (a == c)
    rec = c.to_records()
    assert rec.dtype == PQ.STAT_DTYPE and rec.dtype.itemsize == 32 and rec.nbytes == 32 * len(c)
    assert PQ.PQStats.from_records(rec) == c
    assert PQ.flag_names(5) == ["bit 0: " + PQ.FLAG_NAMES[1], "bit 2: " + PQ.FLAG_NAMES[4]]


def test_abi_mirrors_match_the_library():
    import __graft_entry__ as entry
    from odise_amd import _lib
    entry.build()
    lib = _lib.load()
    assert lib.odise_hip_sizeof_pq_desc() == C.sizeof(_lib.PqDesc)
    assert lib.odise_hip_sizeof_pq_stat() == C.sizeof(_lib.PqStat) == PQ.STAT_DTYPE.itemsize == 32
    assert [PQ.STAT_DTYPE.fields[k][1] for k in ("iou", "tp", "fp", "fn")] == [getattr(_lib.PqStat, k).offset for k in ("iou", "tp", "fp", "fn")]
    assert lib.odise_hip_panoptic_quality(None, None) == -1       # refused before anything is touched


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_stats(rank):
    total = PQ.PQStats(6)
    for seed in ((9, 10) if rank == 0 else (1,)):
        h, w, n_gt, n = {9: (96, 160, 30, 20), 10: (64, 64, 12, 7), 1: (67, 131, 37, 20)}[seed]
        total += blocky_case(seed, h, w, n_gt, n).stats()[0]
    return total


def _sum_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    total, flags = D.sum_pq_stats(_rank_stats(rank), 1 << rank)                  # rank 0 raises bit 0, rank 1 bit 1
    q.put((rank, (D.sum_pq_stats(_rank_stats(rank)).to_records().tobytes(), total.to_records().tobytes(), flags)))
    dist.barrier()
    dist.destroy_process_group()


def test_sum_pq_stats_gloo_world2():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sum_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    r0, r1 = _rank_stats(0), _rank_stats(1)
    assert r0.tp.sum() > 0 and r1.tp.sum() > 0 and (r0.iou * r1.iou).any()      # some category has a sum on both ranks
    ref = r0 + r1
    for r in range(world):
        plain, with_flags, flags = got[r]
        assert plain == with_flags and flags == 3                                # the same sums; every rank sees every rank's bits
        total = PQ.PQStats.from_records(np.frombuffer(plain, PQ.STAT_DTYPE))
        assert np.array_equal(total.tp, r0.tp + r1.tp) and np.array_equal(total.fp, r0.fp + r1.fp) and np.array_equal(total.fn, r0.fn + r1.fn)
        assert total.iou.tobytes() == (r0.iou + r1.iou).tobytes() and total == ref


def test_sum_pq_stats_is_the_identity_outside_a_process_group():
    s = _rank_stats(1)
    assert D.sum_pq_stats(s) is s
    total, flags = D.sum_pq_stats(s, 5)
    assert total is s and flags == 5
