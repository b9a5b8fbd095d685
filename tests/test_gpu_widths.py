"""The BiFPN and head kernels at every width and class count they accept (-m gpu, all through the C ABI).

The planner and `uda_create` take any `fpn_num_filters` that is a multiple of 4 and any `num_classes`; the rest of the suite
runs 64 (D0) and 112 (D2) with 3 / 7 / 10 classes - both widths multiples of 16, class heads of 27 / 63 / 90 channels.  Here the
backbone stays D0's at 192x128 (pinned elsewhere), two BiFPN cells, two head layers, THREE images (T = 3: nine sample rows, so
both branches of the XCD block mapping of sep_kernel / sepf_kernel run), and only the width F, the class count, the dropout
configuration and the split scheme vary (width_cases.py; the path literals are checked on the host by test_widths_host.py):

  w16          F 16, 4 classes     one k-step, one column tile; class head of 36 channels (float4 epilogue)
  w24          F 24, 7             C % 16 == 8: the zeroed tail of sep_kernel's A image inside a 2-step K; one sepf pass of 24 channels
  w88          F 88, 13, head MC   D1's width: tail; deferred-input mode with 352 of 512 units; 3 and 4 column tiles (88, 117 packed)
  w88_f16      F 88, one piece     tail zeroing with one piece image
  w88_bf16x3   F 88, three pieces  the float32 A image's tail branch
  w120         F 120, 15, head MC  tail; no deferred-input mode; class head of 135 channels: blocks of three tiles, one dead
  w128         F 128, 90, head MC  upper bound (132 KB of LDS); 810 channels: nine column blocks, packed rows per block
  w128_bf16x3  F 128, 12           A image + fragments above 120 KB: two tiles a block, gridDim.y = 2
  w128_f16     F 128, 13, head MC  deferred-input mode with all 512 units
  w136         F 136, 7            first width past the fused kernels: fuse_kernel, dw_kernel, pwb_kernel at C = F
  w160         F 160, 90, head MC  D3's width; pwb's 160-wide column tile; 810 outputs unfused
  w384         F 384, 7            D6 / D7's width, the widest of the model table (pws_kernel on the small maps)
  w20          F 20, 7             a multiple of 4, not of 8: unfused, cin % 8 == 4

Per case EVERY named activation the lowering stores, every image and MC sample, against the CPU oracle at
geometry_ref.TAP_TOL (1e-4 of the tap's maximum; one fp16 piece: 1e-2), then the heads (check_heads; one fp16 piece:
HEAD_RMS["full_mc"] of test_gpu_f16_scheme.py), and no range demotion.  What a dropped channel tail does to a node's tap is
measured on the oracle in test_widths_host.py (0.15 of the tap's maximum at F = 88, 0.39 at F = 24: far above either bar).
`bf16` (one bf16 piece) is out of scope: TAP_TOL has no bar for it.

Measured on MI355X: MEASURED below.  Every case passed as the kernels were; no kernel needed a fix.  The worst tap of most cases
lies in the backbone, which does not vary - hence the second figure, over the BiFPN taps alone (P6 / P7 and every node; the
fused lowering stores 18 of them, the unfused one 34).
"""
import numpy as np
import pytest

from common import check_heads, make_images, make_weights
import geometry_ref as G
import width_cases as WC

pytestmark = pytest.mark.gpu

# Measured on MI355X, per case: (taps compared, worst tap error as a fraction of the tap's max|ref| (bar 1e-4; f16: 1e-2), its tap,
# the same over the BiFPN taps alone, its tap).  A record, not a bar: the bars are G.TAP_TOL.
MEASURED = {
    "w16":         (64, 2.00e-6, "blocks_15/out", 1.61e-6, "p6_in"),
    "w24":         (64, 2.00e-6, "blocks_15/out", 1.85e-6, "p6_in"),
    "w88":         (66, 1.68e-6, "blocks_9/out",  8.95e-7, "p6_in"),
    "w88_f16":     (64, 1.61e-3, "blocks_5/dw",   6.44e-4, "p6_in"),      # heads: relative rms 3.6e-4 at most (bar 1.4e-3)
    "w88_bf16x3":  (64, 1.67e-6, "blocks_15/out", 9.90e-7, "p6_in"),
    "w120":        (66, 1.68e-6, "blocks_9/out",  1.07e-6, "p6_in"),
    "w128":        (66, 1.68e-6, "blocks_9/out",  6.53e-7, "p6_in"),
    "w128_bf16x3": (66, 1.50e-6, "blocks_9/out",  8.51e-7, "p6_in"),
    "w128_f16":    (66, 1.34e-3, "blocks_2/dw",   6.08e-4, "p6_in"),      # heads: relative rms 3.5e-4 at most (bar 1.4e-3)
    "w136":        (80, 2.00e-6, "blocks_15/out", 1.50e-6, "cell0/fnode2/fused"),
    "w160":        (82, 1.83e-6, "cell0/fnode1/fused", 1.83e-6, "cell0/fnode1/fused"),
    "w384":        (82, 1.68e-6, "blocks_9/out",  1.47e-6, "cell0/fnode4/fused"),
    "w20":         (80, 2.51e-6, "cell0/fnode7/fused", 2.51e-6, "cell0/fnode7/fused"),
}

_REF = {}


def _reference(case):
    """(params, weights, oracle input, oracle taps, class heads, box heads) of one case: computed once, never modified"""
    if case not in _REF:
        from oracle import preprocess_ref as PP
        from uda_amd.hparams_config import parse_image_size
        p = WC.params_of(case)
        w = make_weights(p, seed=5, cls_spread=20.0)
        imgs = make_images(WC.N_IMAGES, WC.RAW[0], WC.RAW[1], seed=13)
        x, _ = PP.preprocess(imgs, parse_image_size(WC.SIZE), p["mean_rgb"], p["stddev_rgb"])
        taps, rcls, rbox = G.oracle_run(p, w, x, WC.SEED)
        for a in list(taps.values()) + list(rcls) + list(rbox) + [x]:
            a.setflags(write=False)
        _REF[case] = (p, w, x, taps, rcls, rbox)
    return _REF[case]


def _driver(p, w):
    from uda_amd.infer_lib import KerasDriver
    return KerasDriver("_", False, p["name"], batch_size=WC.N_IMAGES, only_network=True, model_params=p, weights=w)


def _check_path(d, c):
    """the lowering the case is about, from the plan (literals: width_cases.py)"""
    from uda_amd import capi
    assert d.pw_scheme == (c.scheme or "f16x2") and d.params["fpn_num_filters"] == c.F
    assert WC.path_counts(d.plan) == (c.sepf, c.sep, c.tin, c.fuse, c.dw)
    kinds = {o["kind"] for o in d.plan.ops}
    if c.sepf:
        assert capi.OP_FUSE not in kinds
        sep = [o for o in d.plan.ops if o["kind"] == capi.OP_SEP]
        assert all(d.plan.bufs[o["ins"][0]].C == c.F for o in sep)
        assert sorted({d.plan.bufs[o["out"]].C for o in sep}) == sorted({c.F, 9 * c.classes, 72})
    else:
        assert capi.OP_SEP not in kinds and capi.OP_FUSE in kinds and capi.OP_DW in kinds


@pytest.mark.parametrize("case", list(WC.CASES))
def test_every_stored_activation_matches_the_oracle_at_this_width(case, capsys):
    """Every case prints its compared-tap count and its worst tap error (measured values: MEASURED above and DESIGN 2 / 9; the bars are
    not raised whatever it measures)."""
    c = WC.CASES[case]
    p, w, x, taps, rcls, rbox = _reference(case)
    d = _driver(dict(p, uda_keep_buffers=True), w)
    try:
        _check_path(d, c)
        d.set_dropout_seed(WC.SEED)
        cls, box = d.predict(x)
        tol = G.TAP_TOL[d.pw_scheme]
        rep = G.compare_taps(d, taps, tol)
        fpn = G.compare_taps(d, {k: v for k, v in taps.items() if k.startswith(("cell", "p6_in", "p7_in"))}, tol)     # (the part that varies)
        with capsys.disabled():
            print("\n[widths %s F=%d classes=%d %s %s] %d of %d oracle taps compared (plan names %d), worst tap error %.3g of the bar = "
                  "%.3g of max|ref| (%s); of the %d BiFPN taps %.3g of max|ref| (%s)" % (
                      case, c.F, c.classes, c.dropout, d.pw_scheme, rep.count, len(taps), c.named, rep.worst, rep.worst * tol,
                      rep.worst_tap, fpn.count, fpn.worst * tol, fpn.worst_tap))
        # no silent skipping: every oracle tap the plan names, minus block 0's two where its dropout site is deferred into the gate
        skipped = G.deferred_taps(d.plan)
        assert skipped == ({"blocks_0/dw", "blocks_0/se"} if c.dropout == "full_mc" else set())
        assert len(taps) == c.taps and len([k for k in taps if k in d.plan.buffer_names]) == c.named
        assert rep.count == c.named - len(skipped) and fpn.count == (34 if c.fuse else 18)
        assert set(G.required_taps(taps, d.plan)) <= set(rep.names)
        assert [g.shape for g in cls + box] == [r.shape for r in rcls + rbox] and cls[0].shape[-1] == 9 * c.classes
        assert d.range_demotions() == 0
        if d.pw_scheme == "f16":
            from test_gpu_f16_scheme import HEAD_RMS, _rel_rms
            errs = [_rel_rms(g, r) for g, r in zip(cls + box, rcls + rbox)]
            with capsys.disabled():
                print("[widths %s] relative rms of the heads: %s" % (case, " ".join("%.2e" % e for e in errs)))
            assert all(np.isfinite(g).all() for g in cls + box) and max(errs) <= HEAD_RMS["full_mc"], errs
        else:
            check_heads(cls, rcls)
            check_heads(box, rbox)
    finally:
        d.close()


def test_a_width_that_is_no_multiple_of_four_is_refused_at_construction():
    """fpn_num_filters = 18: every kernel moves channel quads.  `uda_create` names the channel count; nothing is launched."""
    from uda_amd import capi
    from common import make_params
    p = make_params(num_classes=7, fpn_num_filters=18, **dict(WC.COMMON, **WC.DROPOUT["loss_att"]))
    w = make_weights(p, seed=5, cls_spread=20.0)
    with pytest.raises(capi.UdaError, match=r"channel count 18 not a multiple of 4"):
        _driver(p, w)
