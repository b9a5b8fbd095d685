"""GPU tests of the fp16 range paths that ordinary serves do not reach: an operand above 65504 at an op whose operands are
split into fp16 pieces (`uda_range_demotions`) where the op cannot be demoted (a deferred-input separable conv), where
the run was a member of an ensemble, and where the run was a network-only run post-processed afterwards.

The overflow is made without changing the function the network computes: a depthwise (or BN) scale is multiplied by a
power of two and the 1x1 kernel that follows is divided by the same factor, so that only the operand that is split
grows past fp16's range."""
import numpy as np
import pytest

from common import FULL_MC, HEAD_MC, LOSS_ATT, check_heads, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu

UDA_OP_SEP = 8
UDA_SPLIT_F16X2, UDA_SPLIT_F16X1 = 4, 5


def _driver(p, w, batch, scheme, **kw):
    from uda_amd.infer_lib import KerasDriver
    d = KerasDriver("_", False, p["name"], batch, False, dict(p, uda_pw_scheme=scheme), weights=w, **kw)
    assert d.pw_scheme == scheme
    return d


def _overflow_block3(w):
    """Block 3's projection operand near 1e6 (its depthwise BN scale x 3e5, its projection kernel / 3e5): the same
    function, an A operand of a 1x1 contraction far above 65504 (test_gpu_f16_scheme.test_overflow_is_demoted_and_served)."""
    w = dict(w)
    k = [n for n in w if n.endswith("blocks_3/tpu_batch_normalization_1/gamma")]
    q = [n for n in w if n.endswith("blocks_3/conv2d_1/kernel")]
    assert len(k) == 1 and len(q) == 1
    w[k[0]] = w[k[0]] * np.float32(3.0e5)
    w[q[0]] = w[q[0]] / np.float32(3.0e5)
    return w


@pytest.mark.parametrize("scheme", ["f16x2", "f16"])
def test_deferred_input_sep_overflow_is_refused_before_anything_changes(scheme):
    """D2 under head-only MC dropout: class-net layer 1 (112 -> 112) takes the deferred dropout site of layer 0 (sep_kernel's
    TIN mode), which exists for fp16 pieces (one or two) but not for three bf16 pieces (its LDS image does not fit).  Its
    depthwise taps x 2^30 and its 1x1 kernel x 2^-30 put the pre-scaled depthwise result above 65504 wherever |d| > 2^-20
    (the head's separable convs are initialised with stddev 0.01: its depthwise results are ~1e-4, and 2^12 overflows none).
    The op cannot be demoted: the serve fails with that reason, BEFORE any op is re-packed - every op keeps its scheme, no
    demotion is counted, the next serve fails the same way (not with a broken handle's error) and a batch that stays in
    range (layer 0's dropout keep-scales zero at that site) is served and matches a three-piece handle."""
    from uda_amd.capi import UdaError
    p = make_params(model="efficientdet-d2", image_size="256x256", **HEAD_MC)
    w = dict(make_weights(p, seed=3))
    dk, pk = "class_net/class-1/depthwise_kernel", "class_net/class-1/pointwise_kernel"
    w[dk] = w[dk] * np.float32(2.0 ** 30)
    w[pk] = w[pk] * np.float32(2.0 ** -30)
    imgs = make_images(2, 100, 180, seed=4)
    d = _driver(p, w, 2, scheme)
    ops = d.plan.ops
    tin = [i for i, o in enumerate(ops) if o["kind"] == UDA_OP_SEP and o["drop_site2"] >= 0 and not o["fuse_in"]]
    assert len(tin) == 10, tin            # class and box layer 1, five levels each
    before = [d.op_scheme(i) for i in range(len(ops))]
    want = UDA_SPLIT_F16X2 if scheme == "f16x2" else UDA_SPLIT_F16X1
    assert all(before[i][0] == want for i in tin)
    for _ in range(2):
        d.set_dropout_seed(7)
        with pytest.raises(UdaError, match=r"deferred-input separable conv 112 -> 112 has no three-piece kernel"):
            d.serve(imgs)
        assert d.range_demotions() == 0
        assert [d.op_scheme(i) for i in range(len(ops))] == before
    # in range: the class-net layer 1 input sites dropped entirely
    ref = _driver(p, w, 2, "bf16x3")
    ref.set_dropout_seed(7)
    ref.serve(imgs)
    masks = ref.dropout_masks(2)
    class1 = {ops[i]["drop_site2"] for i in tin[:5]}
    for s in class1:
        masks[d.plan.sites[s][0]][...] = 0.0
    heads = {}
    for name, drv in (("dev", d), ("ref", ref)):
        drv.set_dropout_masks(masks)
        det = drv.serve(imgs)
        assert all(np.isfinite(x).all() for x in det[:3]), name
        heads[name] = drv.head_outputs(2)
    assert d.range_demotions() == 0
    d.close()
    ref.close()
    check_heads(heads["dev"][0] + heads["dev"][1], heads["ref"][0] + heads["ref"][1],
                tol=(2e-4 if scheme == "f16x2" else 4e-3), tol_rms=(1e-4 if scheme == "f16x2" else 1.4e-3))


def test_ensemble_member_that_overflows_is_served_again_before_aggregation():
    """A 3-member deep ensemble whose member 1 overflows (default scheme, two fp16 pieces): the member's heads are checked
    before they are copied into the aggregating handle, so the detections are finite, the member counts its demotion, and
    the aggregation equals the oracle's on the members' (checked) head outputs bit for bit."""
    from oracle import effdet_ref as E, post_ref as P, preprocess_ref as PP
    from uda_amd.infer_lib import EnsembleDriver
    p = make_params(**LOSS_ATT)
    ws = [make_weights(p, seed=40 + m, cls_spread=20.0) for m in range(3)]
    ws[1] = _overflow_block3(ws[1])
    imgs = make_images(2, 100, 180, seed=44)
    ens = EnsembleDriver(ws, p["name"], batch_size=2, model_params=p)
    got = ens.serve(imgs)
    demoted = [m.range_demotions() for m in ens.members]
    assert demoted[1] >= 1 and demoted[0] == demoted[2] == 0, demoted
    assert all(np.isfinite(x).all() for x in got[:3])
    heads = [m.head_outputs(2) for m in ens.members]
    assert [m.range_demotions() for m in ens.members] == demoted
    x, scales = PP.preprocess(imgs, (128, 192), p["mean_rgb"], p["stddev_rgb"])
    pm = dict(p, mc_dropout=True, mc_dropoutrate=1e-9, mc_dropoutsamp=3)
    cls_g = [np.stack([heads[m][0][l] for m in range(3)]) for l in range(5)]
    box_g = [np.stack([heads[m][1][l] for m in range(3)]) for l in range(5)]
    want = P.postprocess_global(pm, cls_g, box_g, scales)
    for g, r in zip(got, want):
        np.testing.assert_array_equal(g, r)
    # the member that overflowed computes its function: its heads against the oracle network
    rc, rb = E.forward_once(ws[1], p, x)
    check_heads(heads[1][0] + heads[1][1], rc + rb)
    ens.close()


def test_network_only_run_then_postprocess_equals_serve():
    """A network-only run (`run_network`: uda_run without post-process) that overflows, post-processed afterwards on the
    same handle from its resident heads: the heads are checked (and the run served again) before the post-process reads
    them, so the detections equal those of `serve` on the same batch bit for bit."""
    p = make_params(**FULL_MC)
    w = _overflow_block3(make_weights(p, seed=81))
    imgs = make_images(2, 100, 180, seed=82)
    a = _driver(p, w, 2, "f16x2")
    a.set_dropout_seed(5)
    want = a.serve(imgs)
    demoted = a.range_demotions()
    assert demoted >= 1
    a.close()
    b = _driver(p, w, 2, "f16x2")
    b.set_dropout_seed(5)
    n = b.run_network(imgs)
    _, scales = b.preprocessed_scales(n)
    cls, box = b.device_heads(n)
    got = b.postprocess(cls, box, scales)
    assert b.range_demotions() == demoted
    b.close()
    assert all(np.isfinite(x).all() for x in got[:3])
    assert len(got) == len(want)
    for g, r in zip(got, want):
        np.testing.assert_array_equal(g, r)
