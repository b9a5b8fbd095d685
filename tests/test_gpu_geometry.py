"""Every network kernel against the oracle's taps on odd-sized maps (-m gpu, all through the C ABI).

Network inputs 201x137 (maps 69x101, 35x51, 18x26, 9x13, 5x7, 3x4, 2x2) and 200x136 (68x100, 34x50, 17x25, 9x13, ...):
with the even 192x128 of the other tests every stride-2 operator - stem, stride-2 depthwise inside the fused MBConv kernels
and stand-alone, P6 / P7 pools, BiFPN pools - sees an odd input (symmetric (1, 1) TF-SAME padding, out = ceil(in / 2)) and
an even one, every nearest-up a 2H and a 2H - 1 target, and no large map is a multiple of a 16 x 16, 32- or 64-pixel tile.

Per case: EVERY named activation the lowering stores, every image and every MC sample, against the CPU oracle
(geometry_ref.compare_taps) at 1e-4 * max|ref| + 1e-6 per tap for the float32-class schemes (f16x2, bf16x3, f32) and at
1e-2 * max|ref| + 1e-6 for the one-piece fp16 scheme - a wrong padding / pool / nearest-up rule moves the first tap it
reaches by 0.11 of its maximum or more (test_geometry_host.py), and fades below 1e-6 in the heads.  Then the heads.

Measured on MI355X, worst tap error relative to the tap's maximum (bar 1.0e-4; f16: 1.0e-2), at 201x137 / 200x136:
default f16x2 2.2e-6 / 2.0e-6, bf16x3 1.8e-6, f32 1.1e-6, unfused 1.8e-6 / 1.5e-6, no fused input 1.6e-6, D2 2.8e-6;
f16 1.35e-3 / 1.42e-3 (blocks_3/out: the first projection that reads an fp16-stored expanded tensor through a one-piece
product) - seven times below its bar, so the bar separates the scheme's rounding from a wrong geometry (>= 0.11) on both sides.
No kernel needed a fix.
"""
import numpy as np
import pytest

from common import FULL_MC, HEAD_MC, LOSS_ATT, check_heads, make_images, make_params, make_weights
import geometry_ref as G

pytestmark = pytest.mark.gpu

SEED = 91
ODD, EVEN = "201x137", "200x136"
DROPOUT = {"full_mc": FULL_MC, "head_mc": HEAD_MC, "loss_att": LOSS_ATT}


def _hw(size):
    from uda_amd.hparams_config import parse_image_size
    return parse_image_size(size)


_REF = {}


def _reference(model, size, dropout, raw=(100, 180)):
    """(params, weights, raw uint8 images, oracle input, image scales, oracle taps, oracle class heads, oracle box heads) of two
    images - computed once per (model, size, dropout, raw size), shared by the cases that need it and never modified.  The raw
    images are smaller than the network input unless a test asks otherwise."""
    key = (model, size, dropout, raw)
    if key not in _REF:
        from oracle import preprocess_ref as PP
        p = make_params(image_size=size, model=model, **DROPOUT[dropout])
        w = make_weights(p, seed=5, cls_spread=20.0)
        imgs = make_images(2, raw[0], raw[1], seed=13)
        x, scales = PP.preprocess(imgs, _hw(size), p["mean_rgb"], p["stddev_rgb"])
        taps, rcls, rbox = G.oracle_run(p, w, x, SEED)
        for a in list(taps.values()) + list(rcls) + list(rbox) + [x, imgs, scales]:
            a.setflags(write=False)
        _REF[key] = (p, w, imgs, x, scales, taps, rcls, rbox)
    return _REF[key]


def _driver(p, w, **kw):
    from uda_amd.infer_lib import KerasDriver
    return KerasDriver("_", False, p["name"], batch_size=2, only_network=kw.pop("only_network", False), model_params=p, weights=w, **kw)


def _ops(d, kind):
    return [o for o in d.plan.ops if o["kind"] == kind]


def _check_default(d):
    from uda_amd import capi
    assert d.pw_scheme == "f16x2"
    mbx = _ops(d, capi.OP_MBX)
    assert {(o["k"], o["stride"]) for o in mbx} == {(3, 1), (3, 2), (5, 1), (5, 2)}          # fused MBConv front halves, both strides
    assert any(d.plan.bufs[o["ins"][0]].C > 48 for o in mbx) and any(o["se_scale"] >= 0 for o in mbx)      # deep variant; absorbed projection
    assert sum(bool(o["fuse_in"]) for o in _ops(d, capi.OP_SEP)) == 24 and not _ops(d, capi.OP_FUSE)     # fusion inside the node's conv


def _check_f16(d):
    from uda_amd import capi
    assert d.pw_scheme == "f16" and _ops(d, capi.OP_MBX)
    assert any(b.storage == "f16" for b in d.plan.bufs), "no expanded tensor is stored as fp16"


def _check_bf16x3(d):
    from uda_amd import capi
    assert d.pw_scheme == "bf16x3" and _ops(d, capi.OP_MBX)
    assert any(o["drop_site2"] >= 0 for o in _ops(d, capi.OP_SEP)), "no head layer takes a deferred dropout site"


def _check_f32(d):
    from uda_amd import capi
    assert d.pw_scheme == "f32" and not _ops(d, capi.OP_SEP)
    assert len(_ops(d, capi.OP_FUSE)) == 24                                                                # fuse_kernel
    mbx = _ops(d, capi.OP_MBX)
    assert mbx and all(d.plan.bufs[o["ins"][0]].C <= 48 for o in mbx)                                      # mbx_kernel (exact f32)
    assert {(3, 1), (5, 1), (5, 2)} <= {(o["k"], o["stride"]) for o in _ops(d, capi.OP_DW)}                # dw_kernel
    assert len(_ops(d, capi.OP_PW)) > 40                                                                   # pw_kernel


def _check_unfused(d):
    from uda_amd import capi
    assert d.pw_scheme == "f16x2" and not _ops(d, capi.OP_MBX) and not _ops(d, capi.OP_SEP)
    assert {(o["k"], o["stride"]) for o in _ops(d, capi.OP_DW)} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    assert len(_ops(d, capi.OP_FUSE)) == 24 and not G.deferred_taps(d.plan)
    assert all(o["drop_site"] < 0 for o in _ops(d, capi.OP_SE))


def _check_no_fused_input(d):
    from uda_amd import capi
    assert d.pw_scheme == "f16x2" and len(_ops(d, capi.OP_FUSE)) == 24
    sep = _ops(d, capi.OP_SEP)
    assert sep and not any(o["fuse_in"] for o in sep)


def _check_d2(d):
    from uda_amd import capi
    assert d.pw_scheme == "f16x2" and d.params["fpn_num_filters"] == 112
    sep = [o for o in _ops(d, capi.OP_SEP) if o["fuse_in"]]
    assert len(sep) == 8 * d.params["fpn_cell_repeats"] and all(d.plan.bufs[o["out"]].C == 112 for o in sep)
    assert _ops(d, capi.OP_MBX)


# case: (model, dropout, scheme, planner switches, oracle taps the plan names of all oracle taps, path check)
CASES = {
    "default": ("efficientdet-d0", "full_mc", None, {}, (74, 114), _check_default),
    "f16": ("efficientdet-d0", "full_mc", "f16", {}, (74, 114), _check_f16),
    "bf16x3": ("efficientdet-d0", "head_mc", "bf16x3", {}, (74, 114), _check_bf16x3),
    "f32": ("efficientdet-d0", "loss_att", "f32", {}, (109, 114), _check_f32),
    "unfused": ("efficientdet-d0", "full_mc", None, dict(UDA_FUSE_MBX=0, UDA_FUSE_SEP=0, UDA_DEFER_DROPOUT=0), (114, 114), _check_unfused),
    "no_fused_input": ("efficientdet-d0", "head_mc", None, dict(UDA_FUSE_IN=0), (98, 114), _check_no_fused_input),
    "d2": ("efficientdet-d2", "full_mc", None, {}, (113, 173), _check_d2),
}
RUNS = [("default", ODD), ("default", EVEN), ("f16", ODD), ("f16", EVEN), ("bf16x3", ODD), ("f32", EVEN),
        ("unfused", ODD), ("unfused", EVEN), ("no_fused_input", ODD), ("d2", ODD)]


@pytest.mark.parametrize("case,size", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_every_stored_activation_matches_the_oracle_on_odd_sized_maps(case, size, capsys):
    """Every case prints its compared-tap count and its worst tap error (measured values: module docstring and DESIGN 2 / 9; the
    one-piece fp16 scheme: 1.42e-3 of the tap's maximum against its bar of 1e-2, which is not raised whatever it measures)."""
    model, dropout, scheme, switches, (n_named, n_oracle), check_path = CASES[case]
    p, w, _, x, _, taps, rcls, rbox = _reference(model, size, dropout)
    q = dict(p, uda_keep_buffers=True)
    if scheme:
        q["uda_pw_scheme"] = scheme
    with G.plan_switches(**switches):             # the planner reads its switches per Plan: set for this construction only
        d = _driver(q, w, only_network=True)
    try:
        check_path(d)
        assert d.image_size == _hw(size) and [tuple(v.shape[2:4]) for v in (taps["stem"], taps["p7_in"])] == [G.SIZES[size][0], G.SIZES[size][-1]]
        d.set_dropout_seed(SEED)
        cls, box = d.predict(x)
        tol = G.TAP_TOL[d.pw_scheme]
        rep = G.compare_taps(d, taps, tol)
        with capsys.disabled():
            print("\n[geometry %s %s %s] %d of %d oracle taps compared (plan names %d), worst tap error %.3g of the bar = %.3g of "
                  "max|ref| (%s)" % (case, size, d.pw_scheme, rep.count, len(taps), n_named, rep.worst, rep.worst * tol, rep.worst_tap))
        # no silent skipping: every oracle tap the plan names, minus block 0's two where its dropout site is deferred into the gate
        skipped = G.deferred_taps(d.plan)
        assert skipped == ({"blocks_0/dw", "blocks_0/se"} if (p["mc_dropout"] and p["mc_dropoutrate"] and case != "unfused") else set())
        assert len(taps) == n_oracle and len([k for k in taps if k in d.plan.buffer_names]) == n_named
        assert rep.count == n_named - len(skipped)
        assert set(G.required_taps(taps, d.plan)) <= set(rep.names)
        assert d.range_demotions() == 0
        if d.pw_scheme == "f16":
            from test_gpu_f16_scheme import HEAD_RMS, _rel_rms
            errs = [_rel_rms(g, r) for g, r in zip(cls + box, rcls + rbox)]
            with capsys.disabled():
                print("[geometry %s %s] relative rms of the heads: %s" % (case, size, " ".join("%.2e" % e for e in errs)))
            assert all(np.isfinite(g).all() for g in cls + box) and max(errs) <= HEAD_RMS["full_mc"], errs
        else:
            check_heads(cls, rcls)
            check_heads(box, rbox)
    finally:
        d.close()


def test_postprocess_on_the_oracles_heads_is_bit_exact_at_an_odd_size():
    """The chain smoke() runs, at 201x137: pyramid levels 18x26, 9x13, 5x7, 3x4, 2x2 = 9 x 636 = 5 724 anchors (2^2 x 3^3 x 53: a
    multiple of no 16-, 32- or 64-wide tile of the post-process kernels) - anchor table, then global and per-class mode on
    the oracle's head outputs, bit for bit.  (P3 is the 18x26 map: 35x51 is the stride-4 map below the pyramid.)"""
    from oracle import post_ref as P
    p, w, _, _, scales, _, rcls, rbox = _reference("efficientdet-d0", ODD, "full_mc")
    d = _driver(p, w)
    try:
        assert d.plan.level_hw == G.SIZES[ODD][2:] == [tuple(c.shape[-3:-1]) for c in rcls]
        assert d.plan.anchors().shape == (5724, 4)
        np.testing.assert_array_equal(d.plan.anchors(), P.anchor_boxes(p))
        for mode, ref in (("global", P.postprocess_global), ("per_class", P.postprocess_per_class)):
            want = ref(p, rcls, rbox, scales)
            got = d.postprocess(rcls, rbox, scales, post_mode=mode)
            assert len(got) == len(want), (mode, len(got), len(want))
            for k, (g, r) in enumerate(zip(got, want)):
                assert g.shape == r.shape, (mode, k, g.shape, r.shape)
                np.testing.assert_array_equal(g, r, err_msg="%s output %d" % (mode, k))
            assert want[3].min() > 0
    finally:
        d.close()


@pytest.mark.parametrize("raw", [(137, 201), (90, 150)], ids=["137x201_scale_1", "90x150_padded"])
def test_serve_from_uint8_at_an_odd_size(raw):
    """serve() from raw uint8: images of exactly 137x201 take the uint8 stem (scale 1; a 603-byte row puts its unaligned 12-byte
    window loads at odd byte offsets), 90x150 ones are resampled to 120x201 and zero-padded below.  Preprocessing bit for bit,
    heads within the float32 bar, detections equal to the post-process of the device's own heads."""
    p, w, imgs, x, scales, _, rcls, rbox = _reference("efficientdet-d0", ODD, "full_mc", raw)
    if raw == (137, 201):
        np.testing.assert_array_equal(scales, np.ones(2, np.float32))
    else:
        assert not x[:, 120:].any() and x[:, 119].any()
    d = _driver(p, w)
    try:
        d.set_dropout_seed(SEED)
        got = d.serve(imgs)
        cls, box = d.head_outputs(2)
        pre, pscales = d.preprocessed()
        np.testing.assert_array_equal(pscales, scales)
        np.testing.assert_array_equal(pre, x)
        check_heads(cls, rcls)
        check_heads(box, rbox)
        again = d.postprocess(cls, box, scales)
        assert len(again) == len(got) == 5
        for k, (g, r) in enumerate(zip(got, again)):
            np.testing.assert_array_equal(g, r, err_msg="output %d" % k)
    finally:
        d.close()


def test_resampled_batch_preprocess_is_bit_exact_at_an_odd_size():
    """raw images of 150x260, larger than the 137x201 input: the separate preprocess pass (bilinear down-scaling to 115x201,
    zero rows below) against the oracle bit for bit, as test_gpu_parity.test_preprocess_bit_exact does at 192x128."""
    from oracle import preprocess_ref as PP
    p = make_params(image_size=ODD)
    w = make_weights(p)
    imgs = make_images(2, 150, 260, seed=150)
    d = _driver(p, w)
    try:
        d.serve(imgs)
        got, scales = d.preprocessed()
        want, wscales = PP.preprocess(imgs, d.image_size, p["mean_rgb"], p["stddev_rgb"])
        assert want[:, 114].any() and not want[:, 115:].any()
        np.testing.assert_array_equal(scales, wscales)
        np.testing.assert_array_equal(got, want)
    finally:
        d.close()
