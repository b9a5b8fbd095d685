"""The whole post-process (`aggregate*`, `class_mean`, `topk*`, NMS, `merge_per_class`, `gather`) on crafted head outputs
(run with -m gpu on an MI355X): the values a trained checkpoint produces and random-init weights never do - saturated
sigmoids, exp under- and overflow in the decode, a class that wins everywhere, identical MC samples, exact ties, signed
zeros, boxes far outside the frame.  `KerasDriver.postprocess` on the heads against `oracle.post_ref` bit for bit
(`assert_array_equal`: NaN equals NaN, inf equals inf - the only tolerance), in both post modes, plus the pre-NMS candidates.

The heads start from the oracle network's outputs (shape, dtype, background values: one run, shared by every
configuration) and are overwritten with numpy.  Image 0 carries the case on every anchor; in image 1 all but a few dozen
anchors are pushed below the score threshold, so `valid < max_output_size` occurs too.

Cases and where `valid < max_output_size` (image 1, asserted in `_check_vacuity` on the reference alone):
  flat              every class logit -2.0                          every configuration without top-k, both modes
  flat_zeros        logits -0.0 / +0.0 alternating by anchor        every configuration without top-k, both modes
  one_class         class C-1 at +6, the others at -6               every configuration without top-k, both modes
  saturated         logits from {-90, -30, -17, 17, 30, 90}         every configuration without top-k, both modes
  collapsed_boxes   th / tw = -104 (a third), +12 (a third),        every configuration without top-k, both modes
                    ty / tx = +-50 (a tenth)
  wide_sigma        sigma channels from {-40, 0, 5, 30}             loss attenuation, l-norm and falsedec, both modes
  identical_samples / identical_outlier   (MC configurations)       both MC configurations without top-k, both modes
(`valid > 0` holds in image 0 of every case, configuration and mode.)

Not in scope, and kept out of the NMS on purpose: non-finite BOX coordinates as live candidates.  `wide_sigma` overflows the
float64 decode to inf at |sigma| >= 30 - those anchors are compared as candidates (`d.candidates` against `pre_nms`) but
carry a class logit of -30, below the score threshold, so no infinite box enters the heap (inf - inf gives a NaN IoU
whose handling the reference does not define)."""
import functools

import numpy as np
import pytest

from common import FULL_MC, LOSS_ATT, PLAIN, make_images, make_params, make_weights, oracle_heads

pytestmark = pytest.mark.gpu

TOPK = dict(nms_configs=dict(method="gaussian", iou_thresh=None, score_thresh=0.0, sigma=None, pyfunc=False,
                             max_nms_inputs=500, max_output_size=100))
CONFIGS = {
    "plain": PLAIN,
    "lossatt": LOSS_ATT,
    "lossatt_falsedec": dict(LOSS_ATT, uncert_adjust_method="falsedec"),
    "full_mc_t10": dict(FULL_MC, mc_dropoutsamp=10),          # register-resident aggregate
    "full_mc_t30": dict(FULL_MC, mc_dropoutsamp=30),          # one class at a time
    "topk_mc": dict(FULL_MC, **TOPK),
    "topk_plain": dict(PLAIN, **TOPK),
}
MODES = ("global", "per_class")
KEEP = 12          # live anchors per level left in image 1


@functools.lru_cache(maxsize=None)
def _base():
    """One pass of the oracle network (loss attenuation, no MC): [N, h, w, A*C] class and [N, h, w, 8A] box outputs."""
    from oracle import preprocess_ref as PP
    p = make_params(**LOSS_ATT)
    w = make_weights(p, seed=11, cls_spread=20.0)
    x, scales = PP.preprocess(make_images(2, 100, 180, seed=12), (128, 192), p["mean_rgb"], p["stddev_rgb"])
    rcls, rbox = oracle_heads(p, w, x, 21)
    for a in rcls + rbox:
        a.setflags(write=False)
    return rcls, rbox, scales


def _parts(p):
    """The base heads in the layout of configuration `p`, per level [class [.., N, A_l, C], box [.., N, A_l, 4], sigma or None]
    (`..` = T for an MC-stacked head, nothing otherwise): sample t is the base pass times (1 + 0.03 g_t) plus noise of 0.05."""
    from oracle import post_ref as P
    rcls, rbox, _ = _base()
    C = p["num_classes"]
    T = int(p["mc_dropoutsamp"]) if p["mc_dropout"] else 1
    stacked_c, stacked_b = P.mc_layout(p)
    rng = np.random.default_rng([T, 9])
    out = []
    for c, b in zip(rcls, rbox):
        def lay(a, stacked):
            if not stacked:
                return a.copy()
            return np.stack([(a * np.float32(1.0 + 0.03 * rng.standard_normal()) +
                              rng.normal(0.0, 0.05, a.shape).astype(np.float32)).astype(np.float32) for t in range(T)])
        c2, b2 = lay(c, stacked_c), lay(b, stacked_b)
        half = b2.shape[-1] // 2
        cv = c2.reshape(c2.shape[:-3] + (-1, C))
        bv = b2[..., :half].reshape(b2.shape[:-3] + (-1, 4)).copy()
        sv = b2[..., half:].reshape(b2.shape[:-3] + (-1, 4)).copy() if p["loss_attenuation"] else None
        out.append([cv, bv, sv, c.shape[-4:-1]])            # (N, h, w) of the level
    return out


def _heads(parts):
    cls, box = [], []
    for cv, bv, sv, (n, h, w) in parts:
        lead = cv.shape[:-3]
        cls.append(np.ascontiguousarray(cv.reshape(lead + (n, h, w, -1)), np.float32))
        b = bv.reshape(lead + (n, h, w, -1))
        if sv is not None:
            b = np.concatenate([b, sv.reshape(lead + (n, h, w, -1))], -1)
        box.append(np.ascontiguousarray(b, np.float32))
    return cls, box


def _thin_image1(parts, rng):
    """Image 1: all but KEEP anchors per level fall below the score threshold (logit -30: a score of 1e-13)."""
    for cv, _, _, _ in parts:
        a = cv.shape[-2]
        dead = np.ones(a, bool)
        dead[rng.choice(a, min(KEEP, a), replace=False)] = False
        cv[..., 1, dead, :] = -30.0


def _case_flat(parts, rng, p):
    for cv, _, _, _ in parts:
        cv[...] = -2.0


def _case_flat_zeros(parts, rng, p):
    for cv, _, _, _ in parts:
        cv[..., 0::2, :] = -0.0
        cv[..., 1::2, :] = 0.0


def _case_one_class(parts, rng, p):
    for cv, _, _, _ in parts:
        cv[...] = -6.0
        cv[..., -1] = 6.0


def _case_saturated(parts, rng, p):
    for cv, _, _, _ in parts:
        cv[...] = rng.choice(np.float32([-90, -30, -17, 17, 30, 90]), cv.shape)


def _case_collapsed_boxes(parts, rng, p):
    for _, bv, _, _ in parts:
        u = rng.random(bv.shape[-3:-1])                    # per (image, anchor), the same in every MC sample
        bv[..., 2:][..., u < 1 / 3, :] = -104.0            # float32 exp underflows to 0: zero-area boxes
        sel = (u >= 1 / 3) & (u < 2 / 3)
        bv[..., 2:][..., sel, :] = 12.0                    # far outside the frame: the clip of the gather
        v = rng.random(bv.shape[-3:-1])
        bv[..., :2][..., v < 0.05, :] = 50.0
        bv[..., :2][..., (v >= 0.05) & (v < 0.1), :] = -50.0


def _case_wide_sigma(parts, rng, p):
    for cv, _, sv, _ in parts:
        sv[...] = rng.choice(np.float32([-40, 0, 5, 30]), sv.shape[-3:])
        overflow = (np.abs(sv) >= 30).any(-1)
        while overflow.ndim > 2:
            overflow = overflow.any(0)
        cv[..., overflow, :] = -30.0                       # (infinite boxes stay out of the heap: see the module docstring)


def _case_identical_samples(parts, rng, p):
    for cv, bv, sv, _ in parts:
        for a in (cv, bv, sv):
            if a is not None and a.ndim == 4:
                a[1:] = a[0]


def _case_identical_outlier(parts, rng, p):
    _case_identical_samples(parts, rng, p)
    for cv, bv, _, _ in parts:
        if cv.ndim == 4:
            cv[-1] += np.float32(1e4)
        if bv.ndim == 4:
            bv[-1, ..., :2] += np.float32(1e4)            # (ty / tx only: th / tw + 1e4 would be an infinite box)


CASES = {
    "flat": _case_flat, "flat_zeros": _case_flat_zeros, "one_class": _case_one_class, "saturated": _case_saturated,
    "collapsed_boxes": _case_collapsed_boxes, "wide_sigma": _case_wide_sigma,
    "identical_samples": _case_identical_samples, "identical_outlier": _case_identical_outlier,
}


def _cases_of(p):
    names = ["flat", "flat_zeros", "one_class", "saturated", "collapsed_boxes"]
    if p["loss_attenuation"] and not p["mc_dropout"]:
        names.append("wide_sigma")
    if p["mc_dropout"]:
        names += ["identical_samples", "identical_outlier"]
    return names


def crafted_heads(p, case):
    rng = np.random.default_rng([sorted(CASES).index(case), 5])
    parts = _parts(p)
    CASES[case](parts, rng, p)
    _thin_image1(parts, rng)
    return _heads(parts)


def reference(p, case):
    """(heads, pre_nms, {mode: output tuple}) of the oracle for one configuration and case."""
    from oracle import post_ref as P
    cls, box = crafted_heads(p, case)
    scales = _base()[2]
    with np.errstate(all="ignore"):
        want = {"global": P.postprocess_global(p, cls, box, scales), "per_class": P.postprocess_per_class(p, cls, box, scales),
                "pre": P.pre_nms(p, cls, box)}
    return cls, box, scales, want


def _check_vacuity(name, case, want):
    M = 100
    for mode in MODES:
        valid = want[mode][3]
        assert valid[0] > 0, (name, case, mode, valid)
        assert not np.isnan(want[mode][1]).any(), (name, case, mode, "NaN scores in the reference")
    if not name.startswith("topk"):
        assert all(want[mode][3][1] < M for mode in MODES), (name, case, [want[m][3] for m in MODES])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_postprocess_on_crafted_heads(name):
    from uda_amd.infer_lib import KerasDriver, ServingDriver
    p = make_params(**CONFIGS[name])
    d = KerasDriver("_", False, p["name"], batch_size=2, model_params=p, weights=make_weights(p, seed=11))
    try:
        for case in _cases_of(p):
            cls, box, scales, want = reference(p, case)
            _check_vacuity(name, case, want)
            for mode in MODES:
                got = d.postprocess(cls, box, scales, post_mode=mode)
                ref = want[mode]
                assert len(got) == len(ref), (case, mode, len(got), len(ref))
                for k, (g, r) in enumerate(zip(got, ref)):
                    assert g.shape == r.shape and g.dtype == r.dtype, (case, mode, k, g.shape, r.shape, g.dtype, r.dtype)
                    np.testing.assert_array_equal(g, r, err_msg="%s %s %s output %d" % (name, case, mode, k))
                    if k == 1:      # scores: signed zeros and every other bit pattern
                        np.testing.assert_array_equal(g.view(np.uint32), r.view(np.uint32), err_msg="%s %s %s score bits" % (name, case, mode))
            cand = d.candidates(2)
            pre = want["pre"]
            for key in ("classes", "scores", "boxes", "u_cls", "u_al", "u_ep"):
                if pre[key] is not None:
                    assert cand[key].shape == pre[key].shape, (case, key, cand[key].shape, pre[key].shape)
                    np.testing.assert_array_equal(cand[key], pre[key], err_msg="%s %s candidates %s" % (name, case, key))
    finally:
        d.close()
