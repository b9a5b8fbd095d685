"""Odd-sized maps, host side (no GPU): the planner's size bookkeeping against the oracle's, and proof that the per-tap bar
of test_gpu_geometry.py separates a wrong geometry from rounding - for every wrong-geometry variant of geometry_ref.py the
first tap it changes moves by at least ten times the loosest bar, and `compare_taps` itself, given the oracle with swapped
padding halves as the "device", fails at exactly that tap."""
import numpy as np
import pytest

from common import FULL_MC, HEAD_MC, LOSS_ATT, make_images, make_params, make_weights
import geometry_ref as G

SEED = 91


def _inputs(size, model="efficientdet-d0", n=1, **over):
    from oracle import preprocess_ref as PP
    from uda_amd.hparams_config import parse_image_size
    p = make_params(image_size=size, model=model, **over)
    w = make_weights(p, seed=11)
    x, _ = PP.preprocess(make_images(n, 60, 110, seed=13), parse_image_size(size), p["mean_rgb"], p["stddev_rgb"])
    return p, w, x


_CACHE = {}


def _base(size, model="efficientdet-d0"):
    """(params, weights, input, oracle taps) of one image at `size` without dropout: computed once, never modified"""
    if (size, model) not in _CACHE:
        p, w, x = _inputs(size, model=model, **LOSS_ATT)
        _CACHE[size, model] = (p, w, x, G.oracle_taps(p, w, x, SEED))
    return _CACHE[size, model]


def test_the_two_sizes_give_the_expected_maps():
    for size, maps in G.SIZES.items():
        taps = _base(size)[3]
        got = sorted({v.shape[2:4] for k, v in taps.items() if not k.endswith("/se")}, reverse=True)
        assert got == maps, (size, got)
        # between them (and the even 192x128 of the other tests) every stride-2 operator sees an odd and an even input
    odd = lambda size: [(h % 2, w % 2) for h, w in G.SIZES[size][:-1]]
    assert all(a != b for a, b in zip(odd("201x137")[:3], odd("200x136")[:3]))


@pytest.mark.parametrize("model", ["efficientdet-d0", "efficientdet-d2"])
@pytest.mark.parametrize("size", ["200x136", "201x137", "203x141", "131x71"])
def test_planner_shapes_equal_the_oracles(model, size):
    """every tap the plan names - fused default lowering and the unfused one, which names all of them - has the oracle tap's
    H x W x C: `same_out` = ceil(n / 2) everywhere, P6 / P7 and the BiFPN targets included"""
    from uda_amd import plan as plan_mod
    p, w, x, taps = _base(size, model)
    plans = [plan_mod.Plan(p, w, 1, 1)]
    with G.plan_switches(UDA_FUSE_MBX=0, UDA_FUSE_SEP=0, UDA_DEFER_DROPOUT=0):
        plans.append(plan_mod.Plan(p, w, 1, 1))
    assert all(k in plans[1].buffer_names for k in taps), "the unfused lowering names every oracle tap"
    for pl in plans:
        named = [k for k in taps if k in pl.buffer_names]
        assert len(named) >= 70
        for k in named:
            b = pl.bufs[pl.buffer_names[k]]
            assert (b.H, b.W, b.C) == taps[k].shape[2:], (model, size, k, (b.H, b.W, b.C), taps[k].shape)
        # the head levels and the anchors follow the same sizes
        # (nodes 3 .. 7 of the last cell are the outputs of levels 3 .. 7)
        assert pl.level_hw == [taps["cell%d/fnode%d/out" % (p["fpn_cell_repeats"] - 1, n)].shape[2:4] for n in (3, 4, 5, 6, 7)]
        A = len(p["aspect_ratios"]) * p["num_scales"]
        assert pl.anchors().shape == (A * sum(h * w_ for h, w_ in pl.level_hw), 4)


def test_tap_counts_per_lowering():
    """how many of the oracle's taps each lowering of test_gpu_geometry.py names (D0: 114 taps, D2: 173) and how many of those
    are compared: all but the two by-design exceptions of a dropout site deferred into block 0's gate"""
    from uda_amd import capi, plan as plan_mod
    p, w, x, taps = _base("201x137")
    assert len(taps) == 114

    def count(over, **sw):
        q = dict(p, **over)
        with G.plan_switches(**sw):
            pl = plan_mod.Plan(q, w, 2, 2)
        return len([k for k in taps if k in pl.buffer_names]), len(G.comparable_taps(pl, taps)), pl

    assert count(FULL_MC)[:2] == (74, 72)
    assert count(dict(FULL_MC, uda_pw_scheme="f16"))[:2] == (74, 72)
    assert count(dict(HEAD_MC, uda_pw_scheme="bf16x3"))[:2] == (74, 74)
    assert count(dict(LOSS_ATT, uda_pw_scheme="f32"))[:2] == (109, 109)
    named, compared, pl = count(FULL_MC, UDA_FUSE_MBX=0, UDA_FUSE_SEP=0, UDA_DEFER_DROPOUT=0)
    assert (named, compared) == (114, 114) and not {capi.OP_MBX, capi.OP_SEP} & {o["kind"] for o in pl.ops}
    named, compared, pl = count(HEAD_MC, UDA_FUSE_IN=0)
    assert (named, compared) == (98, 98) and sum(o["kind"] == capi.OP_FUSE for o in pl.ops) == 24
    assert G.absorbed_outputs(pl) == {"blocks_0/out"} == G.absorbed_outputs(count(FULL_MC)[2])
    full = count(FULL_MC, UDA_FUSE_MBX=0, UDA_FUSE_SEP=0, UDA_DEFER_DROPOUT=0)[2]
    assert not G.absorbed_outputs(full) and len(G.required_taps(taps, full)) == 1 + 16 + 2 + 24
    for pl in (count(FULL_MC)[2], pl, full):
        assert set(G.required_taps(taps, pl)) <= set(G.comparable_taps(pl, taps))
    p2, w2, _, taps2 = _base("201x137", "efficientdet-d2")
    pl2 = plan_mod.Plan(dict(p2, **FULL_MC), w2, 2, 2)
    assert len(taps2) == 173 and len([k for k in taps2 if k in pl2.buffer_names]) == 113
    assert len(G.comparable_taps(pl2, taps2)) == 111 and set(G.required_taps(taps2, pl2)) <= set(G.comparable_taps(pl2, taps2))


@pytest.mark.parametrize("size", sorted(G.SIZES))
@pytest.mark.parametrize("variant", sorted(G.VARIANTS))
def test_the_bar_separates_a_wrong_geometry_from_rounding(variant, size):
    """the first tap a wrong geometry changes moves by at least 10 x the loosest per-tap bar of the GPU tests (1e-2, the
    one-piece fp16 scheme's) relative to the tap's maximum - measured: 0.115 ... 1.07; further down the network the same
    mistake fades to 1e-6 and less, which is why the GPU tests compare taps, not heads"""
    p, w, x, base = _base(size)
    with G.VARIANTS[variant]():
        taps = G.oracle_taps(p, w, x, SEED)
    again = G.oracle_taps(p, w, x, SEED)
    assert all(np.array_equal(again[k], base[k]) for k in base), "the patch was not restored"
    tap, dev = G.first_changed_tap(base, taps)
    print("%s at %s: first changed tap %s, deviation %.3f of its max" % (variant, size, tap, dev))
    assert tap is not None, "the variant changes nothing at this size"
    assert dev >= 10 * G.LOOSEST_TAP_TOL, (tap, dev)
    if variant == "swapped_same_pad":       # an odd input pads (1, 1) either way: the two sizes catch different operators
        assert tap == {"200x136": "stem", "201x137": "blocks_5/dw"}[size]
    if variant == "zero_padded_max_pool":
        assert tap == "p6_in"


class _OracleAsDevice:
    """What compare_taps needs of a driver - the plan and read_buffer - served from oracle taps in the device's row layout."""

    def __init__(self, p, w, taps, n):
        from uda_amd import plan as plan_mod
        with G.plan_switches(UDA_FUSE_MBX=0, UDA_FUSE_SEP=0, UDA_DEFER_DROPOUT=0):       # names every tap
            self.plan = plan_mod.Plan(p, w, n, n)
        self.taps = taps

    def read_buffer(self, name, n):
        a = self.taps[name]
        if not self.plan.bufs[self.plan.buffer_names[name]].per_sample:
            a = a[:, :1]
        return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))


@pytest.mark.parametrize("size,first", [("200x136", "stem"), ("201x137", "blocks_5/dw")])
def test_compare_taps_fails_at_the_first_wrong_operator(size, first):
    """mutation check: the oracle itself passes as the device (every tap, every MC sample, shared buffers against all samples);
    with the padding halves swapped compare_taps fails, names the first tap the mistake reaches and where in it"""
    p, w, x = _inputs(size, n=2, **FULL_MC)
    taps = G.oracle_taps(p, w, x, SEED)
    assert taps["stem"].shape[:2] == (2, 3)
    assert not np.array_equal(taps["blocks_3/out"][:, 0], taps["blocks_3/out"][:, 1]), "the samples differ behind a dropout site"
    good = _OracleAsDevice(p, w, taps, 2)
    rep = G.compare_taps(good, taps, 1e-4)
    assert rep.count == len(taps) == 114 and rep.worst == 0.0 and rep.names == list(taps)
    with G.swapped_same_pad():
        wrong = G.oracle_taps(p, w, x, SEED)
    with pytest.raises(AssertionError) as e:
        G.compare_taps(_OracleAsDevice(p, w, wrong, 2), taps, G.LOOSEST_TAP_TOL)
    msg = str(e.value)
    assert msg.startswith(first + ":") and "(row " in msg and " y " in msg and " c " in msg, msg
    # a per-sample buffer that serves sample 0's rows to every sample is caught as well
    lazy = dict(taps, **{"blocks_3/out": np.repeat(taps["blocks_3/out"][:, :1], 3, 1)})
    with pytest.raises(AssertionError, match="blocks_3/out"):
        G.compare_taps(_OracleAsDevice(p, w, lazy, 2), taps, G.LOOSEST_TAP_TOL)
