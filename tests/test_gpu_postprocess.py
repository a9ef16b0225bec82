"""GPU: the post-processing kernels (csrc/classify_ops.hip, driven by odise_hip_postprocess_batch) against the float64 reference of
tests/post_reference.py on the crafted inputs of tests/post_cases.py, whose margins tests/test_post_reference_cpu.py asserts.

The mask logits are handed over with odise_hip_set_head_masks, so no network runs: a context of the module's own holds nothing but
category_head.text_proj / null_embed (dim 16) and a vocabulary of K random embeddings.  Which kernel a case launches follows from the
dispatcher's conditions (launch_postprocess_pixels, postprocess_batch, launch_semantic_argmax, instance_topk_kernel's `small`):
  tiled pixel pass <7> (fused semantic)   exact geometry, ow % 32 == 0, Q <= 101: q7_k3, q20_k133, q100_k133, q101_k133
  tiled pixel pass <0> + column_fold      the same cases with sem_argmax instead of sem_seg; q100_k133_ragged, q100_k164_w276
  thread-per-cell x4 form + column_stats  Q >= 102 (tile > 64 KiB): q104_k164, q150_k847, q300_k1203; post_generic(2)
  generic form                            the "up" / "down" cases; post_generic(1)
  (test_pixel_pass_exact calls odise_hip_postprocess_pixels for every exact case under each of the three forms and compares its counters)
  semantic GEMM                           every sem_seg that is not fused;  semantic_argmax <7> / <13> / <19>: Q <= 112 / 150 / 300
  instance_topk register / global path    levels_q128_k128 and everything smaller / levels_q128_k129, dense_q128_k129, q300_k1203
  instance_masks x4 / generic             ow % 4 == 0 exact geometries / x4_ragged and the generic ones
"""
import ctypes as C

import numpy as np
import pytest

import post_cases as PC
import post_reference as R
from odise_amd._lib import MAX_SEGMENTS, PostDesc, check
from odise_amd.runtime import Context

pytestmark = pytest.mark.gpu
MARGIN = 2.0 ** -20
ERR_STATE = -3             # ODISE_ERR_STATE


class Rig:
    def __init__(self):
        self.ctx = Context(0)
        rng = np.random.default_rng(11)
        for key, arr in (("category_head.text_proj.weight", rng.standard_normal((16, 16)) / 4), ("category_head.text_proj.bias", np.zeros(16)),
                         ("category_head.null_embed", rng.standard_normal((1, 16)))):
            arr = np.ascontiguousarray(arr, np.float32)
            shape = (C.c_int64 * arr.ndim)(*arr.shape)
            check(self.ctx.lib.odise_hip_load_weight(self.ctx.h, key.encode(), arr.ctypes.data_as(C.POINTER(C.c_float)), shape, arr.ndim), key)
        check(self.ctx.lib.odise_hip_classify_build(self.ctx.h), "classify_build")
        self.K = None

    def vocabulary(self, K):
        if K == self.K:
            return
        rng = np.random.default_rng(K)
        cat, clp = (np.ascontiguousarray(rng.standard_normal((K, 16)), np.float32) for _ in range(2))
        gs, ov = np.ones(K, np.int32), np.zeros(K, np.int32)
        check(self.ctx.lib.odise_hip_set_vocabulary(self.ctx.h, cat.ctypes.data_as(C.c_void_p), clp.ctypes.data_as(C.c_void_p), K, 16,
                                                     gs.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p), K, C.c_float(0.3), C.c_float(0.7)),
              "set_vocabulary")
        self.K = K

    def set_masks(self, cases):
        lg = np.ascontiguousarray(np.stack([c["logits"] for c in cases]), np.float32)
        self.logits_dev = self.ctx.to_device(lg)
        B, Q, h4, w4 = lg.shape
        check(self.ctx.lib.odise_hip_set_head_masks(self.ctx.h, self.logits_dev, B, Q, h4, w4), "set_head_masks")

    def run(self, cases, sem="seg", pan=True, inst=True, topk=100, panoptic_on=None, masks=True):
        """One odise_hip_postprocess_batch over `cases` (same Q, K, logits resolution) -> list of dicts of host arrays."""
        ctx, c0 = self.ctx, cases[0]
        B, Q, K = len(cases), c0["Q"], c0["K"]
        self.vocabulary(K)
        self.set_masks(cases)
        d = PostDesc()
        cls = ctx.to_device(np.ascontiguousarray(np.stack([c["mask_cls"] for c in cases]), np.float32))
        ihw = (C.c_int * (2 * B))(*[v for c in cases for v in c["img"]])
        ohw = (C.c_int * (2 * B))(*[v for c in cases for v in c["out"]])
        thing = (C.c_uint8 * K)(*[1 if k in c0["thing"] else 0 for k in range(K)])
        d.B, d.pad_h, d.pad_w, d.mask_cls = B, 4 * c0["h4"], 4 * c0["w4"], cls.ptr
        d.img_hw, d.out_hw, d.isthing = C.cast(ihw, C.c_void_p), C.cast(ohw, C.c_void_p), C.cast(thing, C.c_void_p)
        pan_flag = pan if panoptic_on is None else panoptic_on
        d.semantic_on, d.panoptic_on, d.instance_on = int(sem is not None), int(pan_flag), int(inst)
        d.object_mask_threshold, d.overlap_threshold, d.topk = c0["object_mask_threshold"], c0["overlap_threshold"], topk
        npix = [c["out"][0] * c["out"][1] for c in cases]
        bufs = {"seg": [ctx.empty((K, n), np.float32) if sem == "seg" else None for n in npix],
                "amax": [ctx.empty((n,), np.int32) if sem == "argmax" else None for n in npix],
                "pan": [ctx.empty((n + 1 + 3 * MAX_SEGMENTS,), np.int32) if pan else None for n in npix],
                "masks": [ctx.zeros((min(topk, Q * K), n), np.float32) if inst and masks else None for n in npix]}
        keep = []

        def parr(lst):
            a = (C.c_void_p * B)(*[b.ptr for b in lst])
            keep.append(a)
            return C.cast(a, C.c_void_p)

        if sem == "seg":
            d.sem_seg = parr(bufs["seg"])
        if sem == "argmax":
            d.sem_argmax = parr(bufs["amax"])
        if pan:
            d.panoptic = parr(bufs["pan"])
        if inst:
            table, scores = ctx.empty((B, 1 + 2 * topk), np.int32), ctx.empty((B, topk), np.float32)
            d.inst_table, d.inst_scores = table.ptr, scores.ptr
            if masks:
                d.inst_masks = parr(bufs["masks"])
        check(ctx.lib.odise_hip_postprocess_batch(ctx.h, C.byref(d)), "postprocess_batch")
        ctx.sync()
        out = []
        for b, c in enumerate(cases):
            oh, ow = c["out"]
            r = {}
            if sem == "seg":
                r["sem"] = bufs["seg"][b].numpy().reshape(K, oh, ow)
            if sem == "argmax":
                r["amax"] = bufs["amax"][b].numpy().reshape(oh, ow)
            if pan:
                rec = bufs["pan"][b].numpy()
                r["seg"], r["n"], r["rows"] = rec[:oh * ow].reshape(oh, ow), int(rec[oh * ow]), rec[oh * ow + 1:].reshape(MAX_SEGMENTS, 3)
            if inst:
                t = table.numpy()[b]
                r["n_inst"], r["query"], r["cls"], r["scores"] = int(t[0]), t[1:1 + topk], t[1 + topk:], scores.numpy()[b]
                if masks:
                    r["masks"] = bufs["masks"][b].numpy().reshape(-1, oh, ow)
            out.append(r)
        return out


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.ctx.lib.odise_hip_post_generic(0)
    r.ctx.close()


def check_panoptic(got, ref, c):
    """segments_info, the table tail and n exactly; the map wherever the reference decides the owner (everywhere on a crafted decision case)."""
    pan = ref["pan"]
    info = [{"id": int(a), "isthing": bool(b), "category_id": int(k)} for a, b, k in got["rows"][:got["n"]]]
    assert info == pan["info"], c["name"]
    assert not got["rows"][got["n"]:].any()
    decided = pan["margin_distinct" if c["dup"] else "margin"] > MARGIN      # a duplicated query ties bitwise: the lowest index wins
    if c["geom"] not in PC.EXACT and c["geom"] != "x4_small":
        own = np.take_along_axis(ref["mask"], np.maximum(pan["owner"], 0)[None], 0)[0]
        decided &= np.abs(own) >= 8 * 2.0 ** -24 * np.abs(ref["mask"]).max()
    assert decided.mean() >= 0.999
    np.testing.assert_array_equal(got["seg"][decided], pan["seg"][decided], err_msg=c["name"])
    assert set(np.unique(got["seg"])) <= {0} | {i["id"] for i in info}      # no id without a row
    return decided


def check_entries(got, ref, c):
    """Scores, masks and tails of the instance table, every entry held to the reference of its own (query, class): the score to rtol 2^-10
    (one fp16 rounding of each sigmoid, integer-exact sums), the mask exactly wherever an fp32 interpolation cannot take the sign of the logit
    differently (everywhere in the exact geometries), zeros past n."""
    n, K = got["n_inst"], c["K"]
    q, k = got["query"][:n], got["cls"][:n]
    assert ((0 <= q) & (q < c["Q"]) & (0 <= k) & (k < K)).all()
    want = R.softmax(c["mask_cls"])[q, k] * R.mask_scores(ref["mask"])[q]
    np.testing.assert_allclose(got["scores"][:n], want, rtol=2.0 ** -10, atol=0, err_msg=c["name"])
    assert not got["query"][n:].any() and not got["cls"][n:].any() and not got["scores"][n:].any()      # entries past n are zero
    if "masks" in got:
        m = got["masks"][:n]
        assert set(np.unique(m)) <= {0.0, 1.0}
        firm = ~R.loose_pixels(ref["mask"], c["geom"] in PC.EXACT)[q]
        np.testing.assert_array_equal((m > 0)[firm], (ref["mask"][q] > 0)[firm], err_msg=c["name"])


def check_instances(got, ref, c):
    """The table equals the lexsort reference exactly."""
    inst = ref["inst"]
    n = len(inst["query"])
    assert got["n_inst"] == n, c["name"]
    assert list(zip(got["query"][:n].tolist(), got["cls"][:n].tolist())) == list(zip(inst["query"].tolist(), inst["cls"].tolist())), c["name"]
    check_entries(got, ref, c)


def check_instances_banded(got, ref, c, things_only, ordered):
    """Random class rows: an entry may differ from the reference only inside the band of (K + 8) 2^-23 relative to the k-th float64
    probability (worst-case fp32 softmax of K + 1 terms; tests/test_post_reference_cpu.py caps the entries in it at 2).  Every reference
    entry outside the band is in the table - in the reference's order where the case separates neighbours by twice the band (`ordered`) -
    and whatever else the table holds lies inside the band; then every entry against the reference of its own (query, class)."""
    inst, K = ref["inst"], c["K"]
    band = (K + 8) * 2.0 ** -23
    n = got["n_inst"]
    g = list(zip(got["query"][:n].tolist(), got["cls"][:n].tolist()))
    w = list(zip(inst["query"].tolist(), inst["cls"].tolist()))
    assert len(set(g)) == n, c["name"]
    whole = inst["n_selected"] == c["Q"] * K                               # topk >= Q * K: there is no k-th to miss
    firm = [e for e, gap in zip(w, inst["gap"]) if whole or gap > band]
    if ordered:
        assert [e for e in g if e in set(firm)] == firm, c["name"]
    else:
        assert set(firm) <= set(g), c["name"]
    p = R.softmax(c["mask_cls"])
    for q, k in set(g) - set(w):
        assert abs(p[q, k] - inst["kth"]) <= band * inst["kth"] and (k in c["thing"] or not things_only), (c["name"], q, k)
    if not things_only:
        assert n == inst["n_selected"]
    check_entries(got, ref, c)


def check_semantic(got, ref, c):
    bound = R.semantic_bound(ref["sem"], c["Q"])
    err = np.abs(got["sem"].astype(np.float64) - ref["sem"])
    worst = (err / bound).max()
    print(f"{c['name']}: semantic worst error / bound = {worst:.3f}")
    assert worst <= 1.0, c["name"]


def check_argmax(got, ref, c):
    first, decided = R.semantic_decided(ref["sem"], c["Q"], c["twin"])      # of the duplicated class column the first copy wins
    assert decided.mean() >= 0.99
    np.testing.assert_array_equal(got["amax"][decided], first[decided], err_msg=c["name"])


@pytest.mark.parametrize("name", list(PC.sweep()))
def test_sweep(rig, name):
    """Every head of one image against the reference: fused or GEMM semantic scores, arg-max, panoptic record, instance table and masks."""
    c, ref = PC.sweep()[name], PC.reference(name)
    got = rig.run([c], sem="seg")[0]
    check_semantic(got, ref, c)
    check_panoptic(got, ref, c)
    check_instances_banded(got, ref, c, things_only=True, ordered=False)   # the order is pinned by the level and the dense cases
    got2 = rig.run([c], sem="argmax", inst=False)[0]
    check_argmax(got2, ref, c)
    np.testing.assert_array_equal(got2["seg"], got["seg"])
    np.testing.assert_array_equal(got2["rows"], got["rows"])


@pytest.mark.parametrize("name", list(PC.decisions()))
def test_decisions(rig, name):
    """Crafted decision cases, compared exactly: segments_info, the map, n and the table tails."""
    c, ref = PC.decisions()[name], PC.reference(name)
    got = rig.run([c], sem=None, inst=False)[0]
    decided = check_panoptic(got, ref, c)
    assert got["n"] == len(ref["pan"]["info"])
    assert decided.all()
    np.testing.assert_array_equal(got["seg"], ref["pan"]["seg"])


@pytest.mark.parametrize("name,topk", [(n, k) for n, ks in (("levels_q20_k133", (1, 7, 100, 4096)), ("levels_q7_k3", (1, 7, 100)),
                                                           ("levels_q128_k128", (100, 4096)), ("levels_q128_k129", (100, 4096))) for k in ks])
@pytest.mark.parametrize("panoptic_on", [0, 1])
def test_instance_levels(rig, name, topk, panoptic_on):
    """Separated probability levels with exact ties: the table equals the lexsort reference exactly, with and without the things filter."""
    c = PC.instances()[name]
    ref = PC.reference(name, topk, bool(panoptic_on))
    got = rig.run([c], sem=None, pan=False, inst=True, topk=topk, panoptic_on=bool(panoptic_on), masks=topk <= 100)[0]
    check_instances(got, ref, c)


@pytest.mark.parametrize("name", ["dense_q128_k128", "dense_q128_k129"])
def test_instance_dense(rig, name):
    """Dense random probabilities at the register and the global-memory path: entries may differ only inside the band around the k-th."""
    c = PC.instances()[name]
    ref = PC.reference(name, 100, False)
    got = rig.run([c], sem=None, pan=False, inst=True, topk=100, panoptic_on=False)[0]
    assert got["n_inst"] == 100
    check_instances_banded(got, ref, c, things_only=False, ordered=True)


def test_forms_agree(rig):
    """odise_hip_post_generic 0 / 1 / 2 on an exact and the ragged case: ids, tables and masks bitwise, sem_seg within 2e-5."""
    lib = rig.ctx.lib
    for name in ("q20_k133", "q100_k133_ragged"):
        c = PC.sweep()[name]
        res = []
        try:
            for form in (0, 1, 2):
                lib.odise_hip_post_generic(form)
                res.append(rig.run([c], sem="seg")[0])
        finally:
            lib.odise_hip_post_generic(0)
        for r in res[1:]:
            for key in ("seg", "rows", "query", "cls", "scores", "masks"):
                np.testing.assert_array_equal(r[key], res[0][key], err_msg=f"{name} {key}")
            assert r["n"] == res[0]["n"] and r["n_inst"] == res[0]["n_inst"]
            np.testing.assert_allclose(r["sem"], res[0]["sem"], rtol=0, atol=2e-5)
            check_semantic(r, PC.reference(name), c)


def test_more_images_than_sets(rig):
    """Six distinct images of mixed sizes in one call (four (S, ids) sets rotate between the two streams): every output bitwise equal to
    the same image run alone."""
    cases = PC.rotation()
    together = rig.run(cases, sem="seg")
    for c, r in zip(cases, together):
        alone = rig.run([c], sem="seg")[0]
        for key in ("sem", "seg", "rows", "query", "cls", "scores", "masks"):
            np.testing.assert_array_equal(r[key], alone[key], err_msg=f"{c['name']} {key}")
        assert r["n"] == alone["n"] and r["n_inst"] == alone["n_inst"]


def test_per_image_entry_points(rig):
    """odise_hip_postprocess_pixels / _panoptic_write / _instance_masks called directly give what the batch call gives; counts equal the
    reference exactly and inst_stats equal (integer sum / 2048, count) of the reference's fp16-rounded sigmoids."""
    ctx, lib = rig.ctx, rig.ctx.lib
    c = PC.entry_case()
    ref = PC.reference(c["name"])
    batch = rig.run([c], sem="seg")[0]
    Q, K, (oh, ow) = c["Q"], c["K"], c["out"]
    Qpad, npix = -(-Q // 8) * 8, oh * ow
    pan = ref["pan"]
    kscore = ctx.to_device(np.where(pan["keep"], pan["scores"], -1.0).astype(np.float32))
    semT = ctx.to_device(np.ascontiguousarray(R.softmax(c["mask_cls"])[:, :K].T, np.float32))
    sem, ids, counts, stats = ctx.empty((K, npix), np.float32), ctx.empty((npix,), np.int32), ctx.empty((3 * Q,), np.int32), ctx.empty((2 * Qpad,), np.float32)
    check(lib.odise_hip_postprocess_pixels(ctx.h, 0, kscore, semT, K, 4 * c["h4"], 4 * c["w4"], c["img"][0], c["img"][1], oh, ow, sem, ids, counts, stats),
          "postprocess_pixels")
    ctx.sync()
    np.testing.assert_array_equal(counts.numpy().reshape(3, Q), pan["counts"])
    idv = ids.numpy().reshape(oh, ow)
    decided = pan["margin_distinct"] > MARGIN
    np.testing.assert_array_equal((idv & 0xffff)[decided], pan["owner"][decided])
    np.testing.assert_array_equal((idv >> 16 & 1).astype(bool)[decided], pan["inside"][decided])
    units, count, fragile = R.inst_stats(ref["mask"])
    assert fragile == 0
    st = stats.numpy().reshape(2, Qpad)
    np.testing.assert_array_equal(st[0, :Q], (units / 2048.0).astype(np.float32))
    np.testing.assert_array_equal(st[1, :Q], count.astype(np.float32))
    assert not st[:, Q:].any()
    check_semantic({"sem": sem.numpy().reshape(K, oh, ow)}, ref, c)
    qmap, seg = ctx.to_device(pan["qmap"].astype(np.int32)), ctx.empty((npix,), np.int32)
    check(lib.odise_hip_panoptic_write(ctx.h, ids, qmap, seg, npix), "panoptic_write")
    np.testing.assert_array_equal(seg.numpy().reshape(oh, ow), batch["seg"])
    n = batch["n_inst"]
    idx, out = ctx.to_device(np.ascontiguousarray(batch["query"][:n], np.int32)), ctx.empty((n, npix), np.float32)
    check(lib.odise_hip_instance_masks(ctx.h, 0, idx, n, 4 * c["h4"], 4 * c["w4"], c["img"][0], c["img"][1], oh, ow, out), "instance_masks")
    np.testing.assert_array_equal(out.numpy().reshape(n, oh, ow), batch["masks"][:n])
    np.testing.assert_array_equal(out.numpy().reshape(n, oh, ow) > 0, ref["inst"]["masks"])


def run_pixels(rig, c, ref, form):
    """odise_hip_postprocess_pixels of one case under odise_hip_post_generic(form) -> ids [oh, ow], counts [3, Q], inst_stats [2, Qpad]."""
    ctx, lib = rig.ctx, rig.ctx.lib
    Q, (oh, ow), pan = c["Q"], c["out"], ref["pan"]
    Qpad = -(-Q // 8) * 8
    rig.set_masks([c])
    kscore = ctx.to_device(np.where(pan["keep"], pan["scores"], -1.0).astype(np.float32))
    ids, counts, stats = ctx.empty((oh * ow,), np.int32), ctx.empty((3 * Q,), np.int32), ctx.empty((2 * Qpad,), np.float32)
    try:
        lib.odise_hip_post_generic(form)
        check(lib.odise_hip_postprocess_pixels(ctx.h, 0, kscore, None, 0, 4 * c["h4"], 4 * c["w4"], c["img"][0], c["img"][1], oh, ow, None, ids, counts,
                                               stats), "postprocess_pixels")
        ctx.sync()
    finally:
        lib.odise_hip_post_generic(0)
    return ids.numpy().reshape(oh, ow), counts.numpy().reshape(3, Q), stats.numpy().reshape(2, Qpad)


EXACT_SWEEP = [n for n, c in PC.sweep().items() if c["geom"] in PC.EXACT]
GENERIC_SWEEP = [n for n, c in PC.sweep().items() if c["geom"] not in PC.EXACT]


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("name", EXACT_SWEEP)
def test_pixel_pass_exact(rig, name, form):
    """Every form of the per-pixel pass on every exact case (form 0: the tiled pass <0> up to Q = 101, the thread-per-cell x4 form from Q = 104
    on; 1: the generic form; 2: the thread-per-cell x4 form): the reference decides every pixel (tests/test_post_reference_cpu.py), so the three
    area counters and the whole (owner | inside) word equal it exactly, and so does the count of positive logits per query."""
    c, ref = PC.sweep()[name], PC.reference(name)
    pan, Q = ref["pan"], c["Q"]
    ids, counts, st = run_pixels(rig, c, ref, form)
    np.testing.assert_array_equal(counts, pan["counts"], err_msg=name)
    np.testing.assert_array_equal(ids, pan["owner"] | (pan["inside"].astype(np.int64) << 16), err_msg=name)
    np.testing.assert_array_equal(st[1, :Q], (ref["mask"] > 0).reshape(Q, -1).sum(1).astype(np.float32))
    assert not st[:, Q:].any()


@pytest.mark.parametrize("name", GENERIC_SWEEP)
def test_pixel_pass_generic(rig, name):
    """The generic form where the output differs from the image: the (owner | inside) word wherever the reference decides it, and every
    counter within the number of pixels that it leaves open (at most 0.1 % of them, tests/test_post_reference_cpu.py)."""
    c, ref = PC.sweep()[name], PC.reference(name)
    pan, Q = ref["pan"], c["Q"]
    ids, counts, st = run_pixels(rig, c, ref, 0)
    loose = R.loose_pixels(ref["mask"], False)
    owned = pan["margin_distinct"] > MARGIN
    decided = owned & ~np.take_along_axis(loose, pan["owner"][None], 0)[0]
    np.testing.assert_array_equal(ids[decided], (pan["owner"] | (pan["inside"].astype(np.int64) << 16))[decided], err_msg=name)
    assert (ids[~decided] & 0xffff < Q).all() and (ids >= 0).all()
    open_owner, open_word = int((~owned).sum()), int((~decided).sum())
    per_query = loose.reshape(Q, -1).sum(1)
    print(f"{name}: pixels left open by the reference: owner {open_owner}, word {open_word}, sign {int(per_query.sum())}")
    assert np.abs(counts[0] - pan["counts"][0]).max() <= open_owner
    assert (np.abs(counts[1] - pan["counts"][1]) <= per_query * pan["keep"]).all()
    assert np.abs(counts[2] - pan["counts"][2]).max() <= open_word
    assert np.abs(st[1, :Q] - (ref["mask"] > 0).reshape(Q, -1).sum(1)).max() <= per_query.max()


def test_injected_masks_refuse_classification(rig):
    """There are no mask embeddings behind injected logits: odise_hip_classify refuses on the host."""
    ctx = rig.ctx
    rig.vocabulary(3)
    rig.set_masks([PC.sweep()["q7_k3"]])
    img, out = ctx.zeros((1, 3, 32, 256), np.float32), ctx.empty((1, 7, 4), np.float32)
    rc = ctx.lib.odise_hip_classify(ctx.h, img, 1, 32, 256, out, None)
    assert rc == ERR_STATE, rc
    assert b"odise_hip_set_head_masks" in ctx.lib.odise_hip_last_error()
