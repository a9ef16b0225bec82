"""GPU: the semantic test-time augmentation (csrc/tta.hip, odise_amd/tta.py) against the float64 reference of tests/tta_reference.py on the
crafted views of tests/tta_cases.py, whose margins tests/test_tta_cpu.py asserts.  The mask logits of every view are handed over with
odise_hip_set_head_masks, so no network runs (the context holds a 16-wide category head and a vocabulary of K random embeddings, as in
tests/test_gpu_postprocess.py); the end-to-end test runs the narrow synthetic model of tests/test_gpu_model.py."""
import ctypes as C

import numpy as np
import pytest

import tta_cases as TC
import tta_reference as TR
from odise_amd._lib import PostDesc, check
from odise_amd.runtime import Context

pytestmark = pytest.mark.gpu
ERR_ARG = -1


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

    def set_masks(self, logits):
        lg = np.ascontiguousarray(logits[None], np.float32)
        self.logits_dev = self.ctx.to_device(lg)
        _, Q, h4, w4 = lg.shape
        check(self.ctx.lib.odise_hip_set_head_masks(self.ctx.h, self.logits_dev, 1, Q, h4, w4), "set_head_masks")

    def add(self, handle, view):
        self.set_masks(view["logits"])
        cls = self.ctx.to_device(np.ascontiguousarray(view["mask_cls"], np.float32))
        handle.add_view(0, cls, view["pad"], view["img"], view["hflip"])
        self.ctx.sync()                                                    # cls and the logits are read by the launch

    def tta(self, case, views=None, sem=True, amax=True, handle=None):
        """The views through one handle -> (sem_seg [K,oh,ow] or None, arg-max [oh,ow] or None)."""
        ctx, K, (oh, ow) = self.ctx, case["K"], case["out"]
        views = case["views"] if views is None else views
        self.vocabulary(K)
        own = handle is None
        if own:
            handle = ctx.tta_create((oh, ow), K, case["Q"], len(views))
        for v in views:
            self.add(handle, v)
        s = ctx.empty((K, oh, ow), np.float32) if sem else None
        a = ctx.empty((oh, ow), np.int32) if amax else None
        handle.finish(s, a)
        ctx.sync()
        out = (s.numpy() if sem else None, a.numpy() if amax else None)
        if own:
            handle.close()
        return out

    def single(self, case, view, sem):
        """odise_hip_postprocess_batch of one view: sem_seg or the fused arg-max of the existing single-view path."""
        ctx, K, (oh, ow) = self.ctx, case["K"], case["out"]
        self.vocabulary(K)
        self.set_masks(view["logits"])
        d = PostDesc()
        cls = ctx.to_device(np.ascontiguousarray(view["mask_cls"][None], np.float32))
        ihw, ohw = (C.c_int * 2)(*view["img"]), (C.c_int * 2)(oh, ow)
        d.B, d.pad_h, d.pad_w, d.mask_cls = 1, view["pad"][0], view["pad"][1], cls.ptr
        d.img_hw, d.out_hw, d.semantic_on = C.cast(ihw, C.c_void_p), C.cast(ohw, C.c_void_p), 1
        buf = ctx.empty((K, oh, ow), np.float32) if sem else ctx.empty((oh, ow), np.int32)
        arr = (C.c_void_p * 1)(buf.ptr)
        if sem:
            d.sem_seg = C.cast(arr, C.c_void_p)
        else:
            d.sem_argmax = C.cast(arr, C.c_void_p)
        check(ctx.lib.odise_hip_postprocess_batch(ctx.h, C.byref(d)), "postprocess_batch")
        ctx.sync()
        return buf.numpy()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.ctx.close()


@pytest.mark.parametrize("name", TC.NAMES)
def test_matches_reference(rig, name):
    """sem_seg within the derived bound on every pixel and class; the arg-max equal on every decided pixel (both outputs of one launch)."""
    c, ref = TC.case(name)
    A = len(c["views"])
    sem, amax = rig.tta(c)
    bound = TR.tta_bound(ref, c["Q"], A)
    err = np.abs(sem.astype(np.float64) - ref)
    print(f"{name}: worst error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    first, decided = TR.tta_decided(ref, c["Q"], A, c["twin"])
    print(f"{name}: decided share {decided.mean():.4f}, arg-max agreement overall {(amax == first).mean():.4f}")
    np.testing.assert_array_equal(amax[decided], first[decided])
    if c["twin"] is not None:
        assert not (amax == c["twin"][1]).any() and (amax == c["twin"][0]).any()     # the tie goes to the first index, across tiles and passes
    only = rig.tta(c, sem=False)[1]                                       # the arg-max-only kernel sees the same sums
    np.testing.assert_array_equal(only, amax)


@pytest.mark.parametrize("name", TC.NAMES)
def test_one_view_equals_the_single_view_path(rig, name):
    """A = 1 without flip: the arg-max bit-identical to odise_hip_postprocess_batch's (the S and PT bits are shared, the products and their
    order too); sem_seg within the two fp32 accumulation terms (Q terms each, in different orders)."""
    c, _ = TC.case(name)
    v = c["views"][0]
    assert not v["hflip"]
    sem, amax = rig.tta(c, views=[v])
    np.testing.assert_array_equal(amax, rig.single(c, v, sem=False))
    want = rig.single(c, v, sem=True).astype(np.float64)
    tol = 2 * c["Q"] * 2.0 ** -24 * np.maximum(want, sem)
    assert (np.abs(sem - want) <= tol).all()


def test_mirrored_twin_view(rig):
    """The same view twice, the second as mirrored logits with hflip: in the exact x4 geometry (4 * w4 = out_w) the mirrored taps carry the
    same weights, so the mean equals the single view up to rounding: equal arg-max on the decided pixels, sem_seg within the bound."""
    c, _ = TC.case("q7_k3_a1")
    v = c["views"][0]
    assert 4 * v["w4"] == c["out"][1] and v["img"] == c["out"]
    twin = {**v, "logits": np.ascontiguousarray(v["logits"][:, :, ::-1]), "hflip": True}
    sem1, amax1 = rig.tta(c, views=[v])
    sem2, amax2 = rig.tta(c, views=[v, twin])
    ref = TR.view_scores(v, c["K"], c["out"])
    _, decided = TR.tta_decided(ref, c["Q"], 2)
    np.testing.assert_array_equal(amax2[decided], amax1[decided])
    assert (np.abs(sem2.astype(np.float64) - ref) <= TR.tta_bound(ref, c["Q"], 2)).all()
    assert (np.abs(sem1.astype(np.float64) - ref) <= TR.tta_bound(ref, c["Q"], 1)).all()


@pytest.mark.parametrize("W", [1, 5, 64, 1023])
def test_hflip_u8_hwc(rig, W):
    img = np.random.default_rng(W).integers(0, 256, (7, W, 3), dtype=np.uint8)
    out = rig.ctx.hflip_u8_hwc(rig.ctx.to_device(img))
    rig.ctx.sync()
    np.testing.assert_array_equal(out.numpy(), np.flip(img, axis=1))


def test_argument_refusals(rig):
    ctx = rig.ctx
    c, _ = TC.case("q7_k3_a2")
    rig.vocabulary(c["K"])
    t = ctx.tta_create(c["out"], c["K"], c["Q"], 1)
    empty = ctx.empty(c["out"], np.int32)
    assert ctx.lib.odise_hip_tta_finish(ctx.h, C.c_void_p(t.handle), None, empty.ptr) == ERR_ARG          # no view yet
    rig.add(t, c["views"][0])
    rig.set_masks(c["views"][1]["logits"])
    cls = ctx.to_device(c["views"][1]["mask_cls"])

    def add(handle, pad=c["views"][1]["pad"], img=c["views"][1]["img"], b=0):
        return ctx.lib.odise_hip_tta_add_view(ctx.h, C.c_void_p(handle.handle), b, cls.ptr, pad[0], pad[1], img[0], img[1], 1)

    assert add(t) == ERR_ARG and b"views already" in ctx.lib.odise_hip_last_error()                       # beyond max_views
    wrong_k, wrong_q = ctx.tta_create(c["out"], c["K"] + 1, c["Q"], 2), ctx.tta_create(c["out"], c["K"], c["Q"] + 1, 2)
    assert add(wrong_k) == ERR_ARG and add(wrong_q) == ERR_ARG
    for h in (wrong_k, wrong_q):                                                                           # ... and left unchanged: still no view
        assert ctx.lib.odise_hip_tta_finish(ctx.h, C.c_void_p(h.handle), None, empty.ptr) == ERR_ARG
    ok = ctx.tta_create(c["out"], c["K"], c["Q"], 2)
    assert add(ok, b=1) == ERR_ARG and add(ok, img=(c["views"][1]["pad"][0] + 1, 8)) == ERR_ARG
    assert ctx.lib.odise_hip_tta_finish(ctx.h, C.c_void_p(t.handle), None, None) == ERR_ARG               # neither output
    h = C.c_void_p()
    assert ctx.lib.odise_hip_tta_create(ctx.h, 1 << 15, 1 << 14, 847, 304, 64, C.byref(h)) == ERR_ARG and not h.value   # 20 TB of S
    first = rig.tta(c, views=[c["views"][0]], sem=False)[1]                                               # the full handle still gives its one view
    got = ctx.empty(c["out"], np.int32)
    t.finish(None, got)
    ctx.sync()
    np.testing.assert_array_equal(got.numpy(), first)
    for x in (t, wrong_k, wrong_q, ok):
        x.close()


def test_reset_between_pictures(rig):
    """One handle, two pictures: after reset the second picture's result is that of a fresh handle (nothing of the first is left)."""
    a, _ = TC.case("q7_k3_a2")
    b, _ = TC.case("q7_k3_a1")
    assert (a["out"], a["K"], a["Q"]) == (b["out"], b["K"], b["Q"])
    rig.vocabulary(a["K"])
    h = rig.ctx.tta_create(a["out"], a["K"], a["Q"], 2)
    rig.tta(a, handle=h)
    h.reset()
    sem, amax = rig.tta(b, handle=h)
    fresh_sem, fresh_amax = rig.tta(b)
    np.testing.assert_array_equal(sem, fresh_sem)
    np.testing.assert_array_equal(amax, fresh_amax)
    h.close()


@pytest.fixture(scope="module")
def narrow(ctx):
    """The narrow synthetic model of tests/test_gpu_model.py with its semantic head on, a smooth 200 x 300 picture on the device and on the
    host, and the text banks of its 11 classes."""
    import torch
    from odise_amd.pipeline import HipCategoryODISE
    from oracle import odise_model as om
    from oracle.backbone import FeatureExtractorBackbone
    from oracle.ldm_extractor import ImplicitCaptionerExtractor
    from oracle.m2f import SemSegHead, init_synthetic_
    small = dict(unet_div=5, vae_div=4, clip_kw=dict(image_size=336, patch_size=14, width=128, layers=2, heads=2, output_dim=64))
    groups, things = [1, 2, 1, 3, 1, 1, 2, 1, 1, 2, 1], {0, 2, 3, 5, 8}
    torch.manual_seed(0)
    ext = ImplicitCaptionerExtractor(**small)
    bb = FeatureExtractorBackbone(ext, [128, 128, 512, 384, 192, 128, 128, 128])
    head = init_synthetic_(SemSegHead(small=True, num_classes=len(groups)))
    heads = om.OpenVocabHeads(ext.clip, groups, projection_dim=64)
    state = ext.export_state()
    state.update({"backbone.feature_projections." + k: v for k, v in bb.feature_projections.state_dict().items()})
    state.update({"sem_seg_head." + k: v for k, v in head.state_dict().items()})
    state["category_head.text_proj.weight"] = heads.text_proj.weight.detach()
    state["category_head.text_proj.bias"] = heads.text_proj.bias.detach()
    state["category_head.null_embed"] = heads.null_embed.detach()
    hip = HipCategoryODISE(ctx, state, semantic_on=True, panoptic_on=False, instance_on=False)
    hip.set_vocabulary(heads.text_embed.numpy(), heads.clip_text_embed.numpy(), groups, heads.category_overlapping_mask.numpy(), things,
                       heads.alpha, heads.beta)
    H, W = 200, 300
    g = torch.Generator().manual_seed(5)
    x = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(torch.rand(1, 3, H, W, generator=g), (4, 4, 4, 4), mode="reflect"), 9, stride=1)
    host = np.ascontiguousarray(((x[0] - x.amin()) / (x.amax() - x.amin()) * 255).round().byte().permute(1, 2, 0).numpy())
    return dict(hip=hip, host=host, picture=ctx.to_device(host), hw=(H, W), heads=heads, groups=groups)


def test_end_to_end_on_the_synthetic_model(ctx, narrow):
    """HipSemanticTTA(min_sizes=(256, 320), flip) on a 200 x 300 picture against the float64 mean of the four views' sem_seg from the existing
    single-view device path, the mirrored ones flipped back on the host.  The S and PT bits are shared, so the difference is accumulation order
    only: Q * 2^-24 of each view's scores, A * Q * 2^-24 of the sum here, and the fp32 rounding of the division."""
    from odise_amd.tta import HipSemanticTTA
    hip, picture, (H, W) = narrow["hip"], narrow["picture"], narrow["hw"]
    tta = HipSemanticTTA(hip, (256, 320), 4000, flip=True)
    views = tta.views(H, W)
    assert views == [((256, 384), False), ((256, 384), True), ((320, 480), False), ((320, 480), True)]
    got = tta([{"image": picture, "height": H, "width": W}])[0]["sem_seg"]
    assert hip.semantic_on and not hip.panoptic_on and not hip.instance_on          # the model's switches are back
    hip.semantic_argmax = True
    got_amax = tta([{"image": picture, "height": H, "width": W}])[0]["sem_seg_argmax"]
    hip.semantic_argmax = False
    tta.close()
    mean = np.zeros(got.shape, np.float64)
    for hw, mirrored in views:
        img = ctx.resize_bilinear_u8(picture, hw[0], hw[1])
        if mirrored:
            img = ctx.hflip_u8_hwc(img)
        s = hip.infer_device([img], 0, [hw], [(H, W)], to_host=True)[0]["sem_seg"].astype(np.float64)
        mean += np.flip(s, axis=2) if mirrored else s
    mean /= len(views)
    Q, A = hip.num_queries, len(views)
    tol = (Q + A * Q + 1) * 2.0 ** -24 * mean + 1e-30
    err = np.abs(got - mean)
    print(f"end to end: worst error / tolerance = {(err / tol).max():.3f}, Q = {Q}")
    assert (err <= tol).all()
    top2 = np.partition(mean, -2, axis=0)[-2:]
    clear = (top2[1] - top2[0]) > 2 * tol.max(0)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(got_amax[clear], mean.argmax(0)[clear])


def _overlay_module():
    import importlib.util
    import os
    from odise_amd import _lib
    path = os.path.join(os.path.dirname(_lib.HERE), "odise_amd", "dropin", "overlay", "mask2former", "test_time_augmentation.py")
    spec = importlib.util.spec_from_file_location("overlay_tta", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_overlay_segmentor_runs_the_views(narrow, tmp_path):
    """The overlay's SemanticSegmentorWithTTA: over the engine itself (a CHW host tensor in, a CPU tensor out, HipSemanticTTA's values), over
    a module with the overlay ODISE's surface and over an OpenPanopticInference-style module around one (the wrapper's switches for the
    call, the module's own afterwards), on the device when the module lives there, from a file, and refusing anything else."""
    import torch
    from torch import nn
    from types import SimpleNamespace as NS
    from PIL import Image
    from odise_amd.tta import HipSemanticTTA
    mod = _overlay_module()
    hip, host, picture, (H, W) = narrow["hip"], narrow["host"], narrow["picture"], narrow["hw"]
    cfg = NS(TEST=NS(AUG=NS(MIN_SIZES=(256,), MAX_SIZE=4000, FLIP=True)))
    direct = HipSemanticTTA(hip, (256,), 4000, flip=True)
    want = torch.from_numpy(direct([{"image": picture, "height": H, "width": W}])[0]["sem_seg"])
    direct.close()
    chw = torch.from_numpy(np.ascontiguousarray(host.transpose(2, 0, 1)))
    inputs = [{"image": chw, "height": H, "width": W}]
    got = mod.SemanticSegmentorWithTTA(cfg, hip)(inputs)[0]["sem_seg"]
    assert not got.is_cuda and torch.equal(got, want)
    got = mod.SemanticSegmentorWithTTA(cfg, hip)([{"image": chw.float() + 0.4, "height": H, "width": W}])[0]["sem_seg"]
    assert torch.equal(got, want)                                         # a float picture is rounded, not truncated

    class Odise(nn.Module):                                               # what the segmentor uses of the overlay's ODISE
        def __init__(self, where):
            super().__init__()
            self.category_head, self.where, self.log = nn.Identity(), where, []

        device = property(lambda self: torch.device(self.where))

        def open_state_dict(self):
            return {"semantic_on": hip.semantic_on}

        def load_open_state_dict(self, state):
            self.log.append(dict(state))
            hip.semantic_on = state["semantic_on"]

        def _engine(self):
            return hip

        def _set_vocabulary(self, engine, text_head):
            self.log.append((engine, text_head))

    class Wrapper(nn.Module):                                             # pano_wrapper.py's OpenPanopticInference: .model + .open_state_dict
        def __init__(self, model):
            super().__init__()
            self.model, self.open_state_dict = model, {"semantic_on": True}

    odise = Odise("cpu")
    assert torch.equal(mod.SemanticSegmentorWithTTA(cfg, odise)(inputs)[0]["sem_seg"], want)
    assert odise.log == [(hip, odise.category_head)]                      # the vocabulary is set on the engine, no open state is touched
    hip.semantic_on = False
    try:
        got = mod.SemanticSegmentorWithTTA(cfg, Wrapper(odise))(inputs)[0]["sem_seg"]
        assert not hip.semantic_on and odise.log[1:] == [{"semantic_on": True}, (hip, odise.category_head), {"semantic_on": False}]
    finally:
        hip.semantic_on = True
    assert torch.equal(got, want)
    if torch.cuda.is_available():                                         # a module on the device gets device tensors, the same values
        got = mod.SemanticSegmentorWithTTA(cfg, Odise("cuda"))(inputs)[0]["sem_seg"]
        assert got.is_cuda and torch.equal(got.cpu(), want)
    Image.fromarray(host).save(tmp_path / "picture.png")
    got = mod.SemanticSegmentorWithTTA(cfg, hip)([{"file_name": str(tmp_path / "picture.png")}])[0]["sem_seg"]
    assert torch.equal(got, want)
    with pytest.raises(TypeError):
        mod.SemanticSegmentorWithTTA(cfg, nn.Linear(2, 2))(inputs)


def test_demo_draws_a_tta_picture(ctx, narrow):
    """The demo's `--task semantic --tta` branch of run_on_image over a HipOpenPanopticInference: the drawn picture is draw_sem_seg of the
    wrapper's test-time-augmented arg-max, and the model's own vocabulary and switches are back afterwards."""
    from odise_amd import demo
    from odise_amd.pipeline import HipOpenPanopticInference
    from odise_amd.tta import HipSemanticTTA
    from odise_amd.visualize import HipVisualizer
    hip, picture, (H, W), heads = narrow["hip"], narrow["picture"], narrow["hw"], narrow["heads"]

    class Text(demo._SeededText):                                         # seeded rows of the narrow model's text width
        def build_text_embed(self, strings):
            return super().build_text_embed(strings)[:, :heads.text_embed.shape[1]]

    labels = [[f"class {k}"] for k in range(7)]
    hip.attach_text(Text(), Text(), train_labels=labels)
    model = HipOpenPanopticInference(hip, labels, demo.demo_metadata(labels, 3), semantic_on=True, instance_on=False, panoptic_on=False)
    visualizer = HipVisualizer(ctx, model.metadata)
    tta = HipSemanticTTA(model, (256,), 2560, flip=True)
    before = hip.open_state_dict()
    drawn = demo.run_on_image(ctx, model, visualizer, picture, "semantic", tta=tta)
    assert drawn.dtype == np.uint8 and drawn.shape == (H, W, 3)
    assert hip.num_classes == len(narrow["groups"]) and not hip.semantic_argmax and hip.open_state_dict()["semantic_on"] == before["semantic_on"]
    hip.semantic_argmax = True
    try:
        amax = tta([{"image": picture, "height": H, "width": W}], to_host=False)[0]["sem_seg_argmax"]
        assert 0 <= amax.numpy().min() and amax.numpy().max() < len(labels)    # the wrapper's vocabulary, not the model's 11 classes
        want = visualizer.draw_sem_seg(picture, amax, hip.num_classes)     # run_on_image draws after the model's own state is back
    finally:
        hip.semantic_argmax = False
    np.testing.assert_array_equal(drawn, want if isinstance(want, np.ndarray) else want.numpy())
    tta.close()


def test_add_view_refuses_a_stale_padded_size(rig):
    """The padded size must be the one the current mask logits were produced at (4 x the logit grid), as odise_hip_postprocess_batch asks."""
    c, _ = TC.case("q7_k3_a2")
    ctx, v = rig.ctx, c["views"][0]
    rig.vocabulary(c["K"])
    rig.set_masks(v["logits"])
    cls = ctx.to_device(v["mask_cls"])
    t = ctx.tta_create(c["out"], c["K"], c["Q"], 1)
    for pad in ((v["pad"][0] + 64, v["pad"][1]), (v["pad"][0], v["pad"][1] - 4)):
        rc = ctx.lib.odise_hip_tta_add_view(ctx.h, C.c_void_p(t.handle), 0, cls.ptr, pad[0], pad[1], 8, 8, 0)
        assert rc == ERR_ARG and b"does not match the mask logits" in ctx.lib.odise_hip_last_error()
    empty = ctx.empty(c["out"], np.int32)
    assert ctx.lib.odise_hip_tta_finish(ctx.h, C.c_void_p(t.handle), None, empty.ptr) == ERR_ARG          # left unchanged: still no view
    t.close()
