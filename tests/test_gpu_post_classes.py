"""The post-process at many classes (run with -m gpu on an MI355X): the rest of the suite stops at 10.  The reference's default
is 90 classes; here 90, 128 and 15 - `aggregate_reg_kernel`'s runtime class loop at class counts its two specialisations do not
cover, `aggregate_kernel` one class at a time at a large count, `class_mean` / `topk*` over A_tot x 90 entries,
`merge_per_class` and the per-class NMS with 90 and 128 segments, `probs_kernel` at 90 and 128.

`KerasDriver.postprocess` on the ORACLE network's head outputs (common.oracle_heads: D0 at 192x128, two images, weights of
seed 11 with a class spread of 20, oracle seed 21) against `oracle.post_ref` bit for bit - both post modes, the pre-NMS
candidates, and the bits of the scores - as test_gpu_post_edges.py does on crafted heads.

Vacuity, asserted on the reference alone: both modes return detections in every image, at least 10 distinct classes appear
(over the two modes; per mode, global / per-class, measured: 19-27 / 29-36 at 90 and 128 classes, 9 / 12 with top-k, 12 / 15 at
15 classes) and at least one class id is above 64 (largest id measured: 85-88 at 90 classes, 127 at 128; the 15-class
configuration has no such id to show)."""
import functools

import numpy as np
import pytest

from common import FULL_MC, LOSS_ATT, PLAIN, make_images, make_params, make_weights, oracle_heads
from test_gpu_post_edges import MODES, TOPK

pytestmark = pytest.mark.gpu

# name: (num_classes, configuration)
CONFIGS = {
    "c90_plain": (90, PLAIN),
    "c90_lossatt": (90, LOSS_ATT),
    "c90_full_mc_t3": (90, dict(FULL_MC, mc_dropoutsamp=3)),
    "c90_full_mc_t10": (90, dict(FULL_MC, mc_dropoutsamp=10)),
    "c90_full_mc_t20": (90, dict(FULL_MC, mc_dropoutsamp=20)),
    "c90_full_mc_t30": (90, dict(FULL_MC, mc_dropoutsamp=30)),
    "c90_topk": (90, dict(PLAIN, **TOPK)),
    "c128_lossatt": (128, LOSS_ATT),
    "c15_full_mc_t20": (15, dict(FULL_MC, mc_dropoutsamp=20)),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(params, weights, heads, scales, {mode: output tuple, "pre": candidates}) of the oracle for one configuration"""
    from oracle import post_ref as P, preprocess_ref as PP
    classes, cfg = CONFIGS[name]
    p = make_params(num_classes=classes, **cfg)
    w = make_weights(p, seed=11, cls_spread=20.0)
    x, scales = PP.preprocess(make_images(2, 100, 180, seed=12), (128, 192), p["mean_rgb"], p["stddev_rgb"])
    cls, box = oracle_heads(p, w, x, 21)
    for a in list(cls) + list(box) + [scales]:
        a.setflags(write=False)
    with np.errstate(all="ignore"):
        want = {"global": P.postprocess_global(p, cls, box, scales), "per_class": P.postprocess_per_class(p, cls, box, scales),
                "pre": P.pre_nms(p, cls, box)}
    return p, w, cls, box, scales, want


def check_vacuity(name, want):
    """on the reference alone: detections in both modes and every image; over the two modes at least 10 distinct classes and
    (where there are that many classes) a class id above 64.  Returns ({mode: distinct classes}, largest class id)."""
    classes = CONFIGS[name][0]
    per_mode, ids_all = {}, []
    for mode in MODES:
        out = want[mode]
        valid = out[3]
        assert (valid > 0).all(), (name, mode, valid)
        assert not np.isnan(out[1]).any(), (name, mode, "NaN scores in the reference")
        cl = out[2][..., 0] if out[2].ndim == 3 else out[2]          # ([N, M, 1 + C] with MC dropout: the id comes first)
        ids = np.concatenate([cl[i, :int(valid[i])] for i in range(len(valid))]).astype(np.int64)
        per_mode[mode] = len(np.unique(ids))
        ids_all.append(ids)
    ids = np.concatenate(ids_all)
    assert len(np.unique(ids)) >= 10, (name, per_mode)
    if classes > 65:
        assert ids.max() > 64, (name, int(ids.max()))
    return per_mode, int(ids.max())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_postprocess_on_the_oracles_heads_at_many_classes(name, capsys):
    from uda_amd.infer_lib import KerasDriver
    p, w, cls, box, scales, want = reference(name)
    distinct, top = check_vacuity(name, want)
    with capsys.disabled():
        print("\n[post classes %s] valid %s / %s, distinct classes %s, largest class id %d" % (
            name, want["global"][3].tolist(), want["per_class"][3].tolist(), distinct, top))
    d = KerasDriver("_", False, p["name"], batch_size=2, model_params=p, weights=w)
    try:
        for mode in MODES:
            got = d.postprocess(cls, box, scales, post_mode=mode)
            ref = want[mode]
            assert len(got) == len(ref), (mode, len(got), len(ref))
            for k, (g, r) in enumerate(zip(got, ref)):
                assert g.shape == r.shape and g.dtype == r.dtype, (mode, k, g.shape, r.shape, g.dtype, r.dtype)
                np.testing.assert_array_equal(g, r, err_msg="%s %s output %d" % (name, mode, k))
                if k == 1:      # scores: signed zeros and every other bit pattern
                    np.testing.assert_array_equal(g.view(np.uint32), r.view(np.uint32), err_msg="%s %s score bits" % (name, mode))
        cand = d.candidates(2)
        pre = want["pre"]
        for key in ("classes", "scores", "boxes", "u_cls", "u_al", "u_ep"):
            if pre[key] is not None:
                assert cand[key].shape == pre[key].shape, (key, cand[key].shape, pre[key].shape)
                np.testing.assert_array_equal(cand[key], pre[key], err_msg="%s candidates %s" % (name, key))
    finally:
        d.close()
