"""CPU: the float64 reference of the semantic test-time augmentation against the literal loop, the margins of the crafted cases, the view
list of HipSemanticTTA and the demo's --tta arguments."""
import numpy as np
import pytest

import tta_cases as TC
import tta_reference as TR
from odise_amd import _lib


@pytest.mark.parametrize("name", TC.NAMES)
def test_reference_equals_the_literal_loop(name):
    c, ref = TC.case(name)
    loop = TR.tta_loop(c)
    np.testing.assert_allclose(ref, loop, rtol=1e-13, atol=1e-300)
    assert ref.shape == (c["K"],) + c["out"] and (ref >= 0).all()


@pytest.mark.parametrize("name", TC.NAMES)
def test_cases_are_decided(name):
    """The GPU test compares the arg-max on the decided pixels only: the share is a property of the inputs, asserted here on the reference alone."""
    c, ref = TC.case(name)
    first, decided = TR.tta_decided(ref, c["Q"], len(c["views"]), c["twin"])
    print(f"{name}: decided share {decided.mean():.4f}")
    assert decided.mean() >= 0.99
    if c["twin"] is not None:
        a, b = c["twin"]
        np.testing.assert_array_equal(ref[a], ref[b])
        assert (first == a).mean() > 0.02 and not (first == b).any()      # the tie is exercised, and the first index wins it


def test_mirrored_views_agree():
    """A view and its mirror see the same field: the mirrored view's scores, flipped back, are close to the plain view's (the inputs are
    built that way; a wrong mirror direction in the reference would break the decided share too, this names it)."""
    c, _ = TC.case("q7_k3_a2")
    a, b = (TR.view_scores(v, c["K"], c["out"]) for v in c["views"])
    assert np.abs(a - b).max() < 0.1 * a.max()
    wrong = TR.view_scores({**c["views"][1], "hflip": False}, c["K"], c["out"])
    assert np.abs(a - wrong).max() > np.abs(a - b).max()


def test_bound_terms():
    ref = np.array([0.0, 0.5, 1.0])
    b1, b6 = TR.tta_bound(ref, 100, 1), TR.tta_bound(ref, 100, 6)
    assert b1[0] == 100 * 2.0 ** -24 and b6[0] == 100 * 2.0 ** -24        # the absolute term is n * 2^-24 / A = Q * 2^-24
    assert b1[2] == 2.0 ** -10 + 2.0 ** -22 + 101 * 2.0 ** -24 + 100 * 2.0 ** -24
    assert (b6 >= b1).all() and b6[2] - b1[2] == 500 * 2.0 ** -24


def test_view_list_and_order():
    from odise_amd.tta import HipSemanticTTA, tta_views
    # 200 x 300: short edge 200 -> 256 gives 256 x 384, -> 384 gives 384 x 576; each size followed by its mirror
    t = HipSemanticTTA(None, (256, 384), 4000, flip=True)
    assert t.views(200, 300) == [((256, 384), False), ((256, 384), True), ((384, 576), False), ((384, 576), True)]
    t = HipSemanticTTA(None, (256, 384), 4000, flip=False)
    assert t.views(200, 300) == [((256, 384), False), ((384, 576), False)]
    # max_size caps the long edge: 384 * 300 / 200 = 576 > 500 -> scale 500 / 576: (333, 500)
    assert tta_views(200, 300, (256, 384), 500) == [((256, 384), False), ((256, 384), True), ((333, 500), False), ((333, 500), True)]
    # a portrait picture: the short edge is the width
    assert tta_views(300, 200, (256,), 4000, flip=False) == [((384, 256), False)]


def test_demo_tta_arguments(capsys):
    from odise_amd.demo import parse_args
    base = ["--input", "a.jpg", "--output", "out"]
    a = parse_args(base + ["--task", "semantic", "--tta", "768,1024,1280"])
    assert a.tta == (768, 1024, 1280) and not a.no_tta_flip
    a = parse_args(base + ["--task", "semantic", "--tta", "512", "--no-tta-flip"])
    assert a.tta == (512,) and a.no_tta_flip
    assert parse_args(base).tta is None and parse_args(base + ["--task", "semantic"]).tta is None
    for bad in (["--tta", "768"], ["--task", "instance", "--tta", "768"], ["--task", "semantic", "--tta", "big"],
                ["--task", "semantic", "--tta", "0"], ["--task", "semantic", "--no-tta-flip"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    capsys.readouterr()


def test_header_declares_the_calls():
    names = {"odise_hip_tta_create", "odise_hip_tta_reset", "odise_hip_tta_destroy", "odise_hip_tta_add_view", "odise_hip_tta_finish",
             "odise_hip_hflip_u8_hwc"}
    assert names <= set(_lib.header_symbols())
    protos = _lib.header_prototypes()
    assert [len(protos[n]) for n in sorted(names)] == [6, 9, 7, 2, 4, 2]


def test_overlay_reads_cfg_and_refuses_a_custom_mapper():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(_lib.HERE), "odise_amd", "dropin", "overlay", "mask2former", "test_time_augmentation.py")
    spec = importlib.util.spec_from_file_location("overlay_tta", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from types import SimpleNamespace as NS
    cfg = NS(TEST=NS(AUG=NS(MIN_SIZES=(256, 384), MAX_SIZE=1000, FLIP=False)))
    t = mod.SemanticSegmentorWithTTA(cfg, object())
    assert (t.min_sizes, t.max_size, t.flip) == ((256, 384), 1000, False)
    t = mod.SemanticSegmentorWithTTA(NS(), object())
    assert t.min_sizes[0] == 400 and t.max_size == 4000 and t.flip
    with pytest.raises(NotImplementedError):
        mod.SemanticSegmentorWithTTA(cfg, object(), tta_mapper=object())
