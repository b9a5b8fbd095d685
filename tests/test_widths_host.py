"""BiFPN / head widths, host side (no GPU): the lowering each case of width_cases.py is meant to reach, agreement of the planner's
kernel predicates with the plans it builds at every width and scheme, and proof on the oracle alone that the per-tap bar of
test_gpu_widths.py sees a channel tail that a kernel drops."""
import numpy as np
import pytest

from common import HEAD_MC, make_images, make_params, make_weights
import geometry_ref as G
import width_cases as WC


_W = {}


def _weights(F, classes=7):
    """weights of one (width, class count): computed once, shared, never modified (they do not depend on dropout or scheme)"""
    if (F, classes) not in _W:
        p = make_params(num_classes=classes, fpn_num_filters=F, **WC.COMMON)
        _W[F, classes] = make_weights(p, seed=5, cls_spread=20.0)
    return _W[F, classes]


@pytest.mark.parametrize("case", list(WC.CASES))
def test_every_case_takes_the_lowering_it_names(case):
    from uda_amd import capi, plan as plan_mod
    c = WC.CASES[case]
    p = WC.params_of(case)
    pl = plan_mod.Plan(dict(p, uda_keep_buffers=True), _weights(c.F, c.classes), WC.N_IMAGES, WC.N_IMAGES)
    assert pl.pw_scheme == (c.scheme or "f16x2")
    assert WC.path_counts(pl) == (c.sepf, c.sep, c.tin, c.fuse, c.dw)
    assert pl.T == (1 if c.dropout == "loss_att" else 3)
    # 8 nodes x 2 cells either way; 2 heads x 3 layers x 5 levels; a deferred site has one taker per level and head
    assert c.sepf + c.fuse == 16 and (c.sep == 30) == bool(c.sepf) and c.tin in (0, 10)
    # the oracle records 98 activations at two cells; the fused lowering stores neither the fused tensor nor a depthwise result
    names = ["stem", "p6_in", "p7_in"] + ["cell%d/fnode%d/out" % (r, n) for r in range(2) for n in range(8)]
    assert all(n in pl.buffer_names for n in names)
    assert ("cell0/fnode0/fused" in pl.buffer_names) == bool(c.fuse)
    heads = [pl.bufs[i] for i in pl.head_out["class"] + pl.head_out["box"]]
    assert [b.C for b in heads] == [9 * c.classes] * 5 + [72] * 5
    assert all(b.per_sample == (c.dropout != "loss_att") for b in heads)
    # the shapes the case is about
    sep = [o for o in pl.ops if o["kind"] == capi.OP_SEP and not o["fuse_in"]]
    assert all(pl.bufs[o["ins"][0]].C == c.F for o in sep)
    if c.tin:
        takers = [o for o in sep if o["drop_site2"] >= 0]
        assert all(pl.bufs[o["out"]].C == c.F and not pl.bufs[o["ins"][0]].per_sample and pl.bufs[o["out"]].per_sample for o in takers)


def test_the_literals_the_cases_are_about():
    """what the table claims per width, from the arithmetic of csrc/kernels_sep.hip restated here"""
    tiles = lambda cout: -(-cout // 32)
    assert [WC.CASES[k].F % 16 for k in ("w24", "w88", "w120")] == [8, 8, 8] and WC.CASES["w16"].F == 16        # tail | one k-step
    assert 16 * (88 // 4) == 352 and 16 * (128 // 4) == 512                                                   # deferred-input units of 2 x 256
    assert [tiles(9 * WC.CASES[k].classes) for k in ("w16", "w88", "w120", "w128")] == [2, 4, 5, 26]
    assert (5 + 2) // 3 == 2 and (26 + 2) // 3 == 9 and 26 - 8 * 3 == 2                                       # blocks of three, dead tiles
    assert all((9 * WC.CASES[k].classes) % 4 for k in ("w88", "w120", "w128")) and (9 * 4) % 4 == 0 == (9 * 12) % 4
    # three bf16 pieces at 128: float32 A image + three tiles of fragments above 120 KB -> two tiles a block
    assert 128 * (8 * 64 + 16) + 8 * 3 * 3 * 1024 > 120 * 1024 >= 128 * (8 * 64 + 16) + 8 * 2 * 3 * 1024
    # two fp16 pieces at 128, four tiles: the largest launch of the table, below a CU's 160 KB
    assert 2 * 128 * (8 * 32 + 16) + 8 * 4 * 2 * 1024 == 135168 <= 160 * 1024


@pytest.mark.parametrize("F", WC.WIDTHS)
def test_the_planners_predicates_agree_with_its_plans(F):
    """every width of the table under every split scheme, head-only MC dropout (the configuration in which a head layer may
    defer its site): the node convs are fused exactly where `sepf_supported` says so, the first head layer defers exactly
    where `sep_tin_supported` says so, and nothing above 128 or off a multiple of 8 reaches a fused separable conv"""
    from uda_amd import plan as plan_mod
    w = _weights(F)
    for sch in plan_mod.PW_SCHEMES_ALL:
        p = make_params(num_classes=7, fpn_num_filters=F, uda_pw_scheme=sch, **dict(WC.COMMON, **HEAD_MC))
        pl = plan_mod.Plan(p, w, WC.N_IMAGES, WC.N_IMAGES)
        sepf, sep, tin, fuse, dw = WC.path_counts(pl)
        fusable = sch != "f32" and F % 8 == 0 and 16 <= F <= 128
        assert plan_mod.sepf_supported(F, F, sch) == fusable, (F, sch)
        assert (sepf, fuse) == ((16, 0) if fusable else (0, 16)), (F, sch, sepf, fuse)
        assert (sep, dw) == ((30, 0) if fusable else (0, 46)), (F, sch, sep, dw)
        assert tin == (10 if plan_mod.sep_tin_supported(F, F, sch) else 0), (F, sch, tin)
        if not fusable:
            assert not plan_mod.sep_tin_supported(F, F, sch) or sch != "f32" and F % 8 == 0 and 64 <= F <= 128
    # the decisions as literals (deferred head ops under f16x2 / bf16x3 / bf16x2 / f16 / bf16): one piece leaves room at 120 and 128
    want = {88: (10, 10, 10, 10, 10), 120: (0, 0, 0, 10, 10), 128: (0, 0, 0, 10, 10)}.get(F, (0, 0, 0, 0, 0))
    got = tuple(10 * int(plan_mod.sep_tin_supported(F, F, s)) for s in ("f16x2", "bf16x3", "bf16x2", "f16", "bf16"))
    print("F = %d: deferred head ops under f16x2 / bf16x3 / bf16x2 / f16 / bf16: %s" % (F, got))
    assert got == want, (F, got)


# ------------------------------------------------------------------ a dropped channel tail against the per-tap bar
TAIL_SEED = 11
NODE, NODE_TAP = "fpn_cells/cell_0/fnode0/op_after_combine5/conv", "cell0/fnode0/out"


def _without_tail(F):
    """the oracle with the channels [16 (F // 16), F) missing from ONE node's 1x1: what a kernel computes that stops at the last
    whole k-step of its matrix stage"""
    from oracle import effdet_ref as E
    orig = E._sepconv

    def _sepconv(x, w, prefix, dwk="depthwise_kernel", pwk="pointwise_kernel", use_bias=True):
        if prefix != NODE:
            return orig(x, w, prefix, dwk, pwk, use_bias)
        x = E.depthwise(x, w[prefix + "/" + dwk], 1).clone()
        x[:, 16 * (F // 16):] = 0.0
        return E.conv2d(x, w[prefix + "/" + pwk], 1, w[prefix + "/bias"] if use_bias else None)
    return G._patched("_sepconv", _sepconv)


@pytest.mark.parametrize("F", [88, 24])
def test_the_bar_sees_a_dropped_channel_tail(F):
    """the node's own tap moves by at least ten times the loosest per-tap bar (1e-2 of its maximum, the one-piece fp16 scheme's;
    the float32-class schemes' bar is a hundred times tighter).  Measured with the weights of seed 11: 0.152 of the tap's maximum
    at F = 88 (8 of 88 channels), 0.391 at F = 24 (8 of 24).  The weights of seed 5, which the GPU test uses, give 0.073 at 88:
    730 x the bar of the float32-class cases, 7.3 x the one-piece bar - hence another seed here, never another bar."""
    from oracle import preprocess_ref as PP
    p = make_params(num_classes=7, fpn_num_filters=F, **dict(WC.COMMON, loss_attenuation=True))
    w = make_weights(p, seed=TAIL_SEED, cls_spread=20.0)
    x, _ = PP.preprocess(make_images(1, WC.RAW[0], WC.RAW[1], seed=13), (128, 192), p["mean_rgb"], p["stddev_rgb"])
    base = G.oracle_taps(p, w, x, WC.SEED)
    with _without_tail(F):
        taps = G.oracle_taps(p, w, x, WC.SEED)
    again = G.oracle_taps(p, w, x, WC.SEED)
    assert all(np.array_equal(again[k], base[k]) for k in base), "the patch was not restored"
    tap, dev = G.first_changed_tap(base, taps)
    print("F = %d: channels %d .. %d dropped from %s: first changed tap %s moves by %.3f of its maximum = %.1f x the loosest bar "
          "(%.0f x the float32-class bar)" % (F, 16 * (F // 16), F - 1, NODE, tap, dev, dev / G.LOOSEST_TAP_TOL, dev / G.TAP_TOL["f16x2"]))
    assert tap == NODE_TAP and base[tap].shape[-1] == F
    assert dev >= 10 * G.LOOSEST_TAP_TOL, (tap, dev)
