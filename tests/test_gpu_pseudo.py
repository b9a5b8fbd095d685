"""Pseudo-labelling on the device (`ServingDriver.pseudo_rows` / `serve_pseudo_labels`, `pseudo_labels.select_detections`;
reference SSL_stac.py:302-642): the kernels against what the reference's own `STAC.score_image` returned
(tests/golden/pseudo_golden.npz), the two host-array instantiations against each other bit for bit, the scan across the
256-thread stride and the 99-row cap against the restatement (tests/pseudo_ref.py), the served flow bit for bit against the
host-array entry point on the detections the device produced, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import pseudo_ref as R
from common import HEAD_MC, LOSS_ATT, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu

RAW = (130, 190)                 # model input 128 x 192 (make_params' default)
SEED = 29
# The seeded weights give every image 100 detections with scores between 0.009 and 0.02: this NMS threshold ends the list early,
# so that the images carry padded slots (0 < valid_len < M); min_score and tau are then chosen inside the list
NMS = dict(nms_configs=dict(method="gaussian", iou_thresh=None, score_thresh=0.0125, sigma=None, pyfunc=False,
                            max_nms_inputs=0, max_output_size=100))
G = R.Golden()
RESIDENT = ("alluncert", "pseudoscore_combo", "epuncert", "ental", "pseudoscore_score", "entropy", "box_norm_albox", "class_mcclass")


def check_against_golden_rows(got, g, kept_want):
    rec, minmax, kept, cand = got
    np.testing.assert_array_equal(rec["image"], g["cand_image"])
    np.testing.assert_array_equal(rec["row"], g["cand_row"])
    np.testing.assert_array_equal(rec["cls"], g["cand_classes"])
    np.testing.assert_array_equal(kept, kept_want)
    np.testing.assert_array_equal(cand, g["cand"])
    np.testing.assert_array_equal(np.isnan(rec["v"]), np.isnan(g["cand_v"]))
    np.testing.assert_array_equal(np.isinf(rec["v"]), np.isinf(g["cand_v"]))
    np.testing.assert_allclose(rec["v"], g["cand_v"], rtol=1e-12, atol=0)
    if "minmax" in g:
        np.testing.assert_allclose(minmax, g["minmax"], rtol=1e-12, atol=0)


def check_against_restatement(got, cols, sel, min_score, tau, max_rows=99):
    """got = (records, minmax, kept, cand) of the device for the float64 columns `cols`: rows exact, values to 1e-12."""
    res, minmax, kept, cand, _ = R.rows(cols, sel.components, sel.invert, sel.gate, min_score, tau, max_rows)
    rec = got[0]
    np.testing.assert_array_equal(rec["image"], res["image"])
    np.testing.assert_array_equal(rec["row"], res["row"])
    np.testing.assert_array_equal(rec["cls"], res["cls"])
    np.testing.assert_array_equal(got[2], kept)
    np.testing.assert_array_equal(got[3], cand)
    np.testing.assert_allclose(rec["v"], res["v"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[1], minmax, rtol=1e-12, atol=0)
    for k, (i, r) in enumerate(zip(rec["image"], rec["row"])):
        assert (rec["box"][k] == np.asarray(cols["boxes"][i][r][:4], np.float32)).all() and rec["det_score"][k] == np.float32(cols["scores"][i][r])
    return kept, cand


def same_bits(a, b):
    assert a[0].tobytes() == b[0].tobytes()
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])


# ------------------------------------------------------------------ the kernels against the reference's own results
@pytest.mark.parametrize("ci", range(len(G.cases)), ids=G.ids)
def test_golden_through_device(ci):
    from uda_amd import active_learning as AL, pseudo_labels as PL
    ds, strategy, tau = G.cases[ci]
    cols, C_, names, g = G.case(ci)
    got = PL.select_detections(cols, strategy, tau, G.min_score, opt_params=G.opt, num_classes=C_)
    check_against_golden_rows(got, g, G.z["%s_kept" % ds][:len(names)])
    sel = PL.resolve_selection("pseudoscore_" + strategy, dict.fromkeys(AL.SOURCES), G.opt)
    acc = PL.PseudoLabelSet(sel, tau, G.opt_thrs)
    half = len(names) // 2
    for lo, hi in ((0, half), (half, len(names))):             # two batches, as a dataset is served
        sub = {k: v[lo:hi] for k, v in cols.items()}
        acc.add(names[lo:hi], PL.select_detections(sub, sel, tau, G.min_score, num_classes=C_), boxes=sub["boxes"])
    R.same_selection(acc.finalize(), G.returned(ci))


@pytest.mark.parametrize("ds,strategy,tau", [("b", "alluncert", 0.4), ("b", "pseudoscore_combo", 0.9), ("b", "class_mcclass", 0.4),
                                             ("a", "box_norm_albox", 0.4), ("z", "ental", 0.4), ("z", "box_norm_albox", 0.4),
                                             ("z", "combo", 0.4)])
def test_float_and_double_instantiations_agree_bit_for_bit(ds, strategy, tau):
    from uda_amd import pseudo_labels as PL
    cols, C_ = G.columns(ds)
    cols32 = {k: v.astype(np.float32) for k, v in cols.items()}
    if ds == "z":                                              # (rounding to float32 must not open the zero sides)
        assert (cols32["boxes"][0, 0, 2] == cols32["boxes"][0, 0, 0]) and (cols32["boxes"][1, 0, 3] == cols32["boxes"][1, 0, 1])
    back = {k: v.astype(np.float64) for k, v in cols32.items()}
    min_score = float(np.float32(G.min_score))
    a = PL.select_detections(back, strategy, tau, min_score, opt_params=G.opt, num_classes=C_)
    b = PL.select_detections(cols32, strategy, tau, min_score, opt_params=G.opt, num_classes=C_, as_float32=True)
    assert len(a[0]) > 0
    same_bits(a, b)
    if ds == "z" and strategy != "combo":
        assert not np.isfinite(a[0]["v"]).all() or not np.isfinite(a[1]).all()


def test_scan_across_the_thread_stride_and_the_cap():
    """M = 300 in one image: ranks and candidate slots carry over from the first chunk of 256 rows into the second; with
    max_rows = 250 rows of the second chunk take part, with 99 none of them does.  And the fixture's image with 100 kept rows
    under the multi-column branches, which the reference cannot serve: capped at 99 like every other branch."""
    from uda_amd import active_learning as AL, pseudo_labels as PL
    rng = np.random.default_rng(11)
    n, M, C_ = 1, 300, 4
    scores = np.where(rng.uniform(size=(n, M)) < 0.9, rng.uniform(0.11, 0.99, (n, M)), rng.uniform(0.0, 0.09, (n, M)))
    y1, x1 = rng.uniform(0, 300, (n, M)), rng.uniform(0, 900, (n, M))
    cols = dict(boxes=np.stack([y1, x1, y1 + rng.uniform(2, 60, (n, M)), x1 + rng.uniform(2, 60, (n, M))], -1), scores=scores,
                classes=rng.integers(1, C_ + 1, (n, M)).astype(np.float64), entropy=rng.uniform(0.01, 2.0, (n, M)),
                albox=rng.gamma(2.0, 0.5, (n, M, 4)), mcbox=rng.gamma(2.0, 0.5, (n, M, 4)), mcclass=rng.gamma(2.0, 0.2, (n, M, C_)))
    assert (scores[0, :256] > 0.1).sum() > 200 and (scores[0, 256:] > 0.1).sum() > 30
    for strategy, tau in (("alluncert", 0.5), ("entropy", 1.0), ("score", 0.5)):
        sel = PL.resolve_selection(strategy, dict.fromkeys(AL.SOURCES))
        for max_rows in (99, 250, 4096):
            got = PL.select_detections(cols, sel, tau, 0.1, num_classes=C_, max_rows=max_rows)
            kept, cand = check_against_restatement(got, cols, sel, 0.1, tau, max_rows)
            assert kept[0] > 250 and 0 < cand[0] < min(max_rows, kept[0])
            assert (got[0]["row"].max() >= 256) == (max_rows > 99)
    cols, C_ = G.columns("a")
    assert (cols["scores"][-1] > G.min_score).sum() == 100
    for strategy in ("alluncert", "ental", "epuncert", "combo"):
        sel = PL.resolve_selection(strategy, dict.fromkeys(AL.SOURCES), G.opt)
        got = PL.select_detections(cols, sel, 0.4, G.min_score, num_classes=C_)
        kept, cand = check_against_restatement(got, cols, sel, G.min_score, 0.4)
        assert kept[-1] == 100 and not (got[0]["row"][got[0]["image"] == len(kept) - 1] == 99).any()
        uncapped = PL.select_detections(cols, sel, 0.0, G.min_score, num_classes=C_, max_rows=100)
        assert uncapped[3][-1] == 100 and PL.select_detections(cols, sel, 0.0, G.min_score, num_classes=C_)[3][-1] == 99


# ------------------------------------------------------------------ the served flow
def _driver(cfg, batch, **over):
    from uda_amd.infer_lib import KerasDriver
    p = make_params(**dict(cfg, **dict(NMS, **over)))
    d = KerasDriver("_", False, p["name"], batch, False, p, weights=make_weights(p, seed=12, cls_spread=20.0))
    d.set_dropout_seed(SEED)
    return d


@pytest.fixture(scope="module")
def driver():
    d = _driver(HEAD_MC, 13)
    yield d
    d.close()


def cuts_inside(scores, valid):
    """(min_score, tau) as float32 values at the 30 % and 70 % quantiles of the valid served scores."""
    s = np.sort(np.concatenate([scores[i, :int(valid[i])] for i in range(len(valid))]))
    assert len(s) > 8
    pick = lambda q: float(np.float32((float(s[int(q * len(s))]) + float(s[int(q * len(s)) + 1])) / 2))      # noqa: E731
    return pick(0.3), pick(0.7)


def columns64(un):
    return {k: (None if un.get(k) is None else np.asarray(un[k], np.float64)) for k in R.COLUMN_KEYS}


def check_served(d, un, got, strategy, min_score, tau, opt):
    """got: the device's result for the resident detections whose unpacked columns are `un`."""
    from uda_amd import pseudo_labels as PL
    sel = PL.resolve_selection(strategy, d.params, opt)
    cols32 = {k: un[k] for k in R.COLUMN_KEYS if un.get(k) is not None}
    host = PL.select_detections(cols32, sel, tau, min_score, num_classes=d.num_classes, as_float32=True)
    same_bits(got, host)
    return check_against_restatement(got, columns64(un), sel, np.float32(min_score), tau)


@pytest.mark.parametrize("n", [2, 13])
def test_serve_pseudo_labels(driver, n, monkeypatch):
    d = driver
    imgs = make_images(n, *RAW, seed=3 + n)
    un = d.serve_unpacked(imgs)
    valid = un["valid_len"]
    assert (valid > 0).all()
    min_score, tau = cuts_inside(un["scores"], valid)
    inside = False
    with monkeypatch.context() as mp:
        # the 100-row tuple is never downloaded: the resident serve, then the records alone
        mp.setattr(d, "_collect", lambda *a, **k: pytest.fail("serve_pseudo_labels downloaded the detection columns"))
        served = {s: d.serve_pseudo_labels(imgs, s, tau, G.opt, min_score) for s in RESIDENT}
        assert d.serve_resident(imgs) == n
        again = d.pseudo_rows("alluncert", tau, min_score=min_score)
    same_bits(again, served["alluncert"])
    for strategy, got in served.items():
        kept, cand = check_served(d, un, got, strategy, min_score, tau, G.opt)
        if strategy in ("alluncert", "pseudoscore_score"):
            inside |= bool(((kept > 0) & (kept < valid) & (cand > 0) & (cand < kept)).any())
    assert inside, "no image with 0 < cand < kept < valid_len: the cuts never fell inside a list"
    # the default min_score is the writer's 0.1 under SSL: above every seeded score, nothing is kept
    none = d.pseudo_rows("entropy", tau)
    assert len(none[0]) == 0 and (none[2] == 0).all() and (none[1] == [np.inf, -np.inf]).all()


def test_as_while_resident_callback_and_accumulated(driver):
    from uda_amd import postprocess as pp, pseudo_labels as PL
    d = driver
    batches = [make_images(3, *RAW, seed=21), make_images(1, *RAW, seed=22)]
    first = d.serve(batches[0])
    min_score, tau = cuts_inside(first[1], first[3])
    sel = PL.resolve_selection("pseudoscore_ental", d.params)
    acc = PL.PseudoLabelSet(sel, tau)

    def per_batch(det):
        probab, entropy = (a[:det[0].shape[0]] for a in d.class_probs(det[0].shape[0]))
        return pp.unpack_detections(d.params, det, probab, entropy), d.pseudo_rows(sel, tau, min_score=min_score)

    seen = 0
    for b, (un, got) in enumerate(d.serve_stream(batches, while_resident=per_batch)):
        check_served(d, un, got, sel.name, min_score, tau, None)
        acc.add(["%d_%d.png" % (b, i) for i in range(len(got[3]))], got)
        seen += int(got[3].sum())
    names, classes, boxes, pseudo = acc.finalize()
    assert acc.n_images == 4 and seen > 0 and sum(len(c) for c in classes) == seen       # epuncert / ental: the det_score filter alone
    assert len(names) == len(pseudo) > 0


def test_ensemble_selects_in_its_aggregating_handle():
    from uda_amd import postprocess as pp
    from uda_amd.infer_lib import EnsembleDriver
    p = make_params(**dict(LOSS_ATT, **NMS))
    ens = EnsembleDriver([make_weights(p, seed=40 + m, cls_spread=20.0) for m in range(2)], p["name"], batch_size=2, model_params=p)
    try:
        imgs = make_images(2, *RAW, seed=14)
        det = ens.serve(imgs)
        min_score, tau = cuts_inside(det[1], det[3])
        got = ens.serve_pseudo_labels(imgs, "ental", tau, min_score=min_score)
        probab, entropy = ens.post.class_probs(2)
        un = pp.unpack_detections(ens.post.params, det, probab, entropy)
        kept, cand = check_served(ens.post, un, got, "ental", min_score, tau, None)
        assert cand.sum() > 0
    finally:
        ens.close()


def test_refusals_leave_the_handle_usable(driver):
    from uda_amd import capi, pseudo_labels as PL
    from uda_amd.infer_lib import KerasDriver
    d = driver
    imgs = make_images(2, *RAW, seed=8)
    det = d.serve(imgs)
    min_score, tau = cuts_inside(det[1], det[3])
    want = d.pseudo_rows("alluncert", tau, min_score=min_score)
    usable = lambda: same_bits(d.pseudo_rows("alluncert", tau, min_score=min_score), want)      # noqa: E731
    with pytest.raises(ValueError, match="tau"):
        d.pseudo_rows("alluncert", -0.5, min_score=min_score)
    with pytest.raises(ValueError, match="select_detections"):
        d.pseudo_rows("calib_entropy", tau, min_score=min_score)
    # the library refuses by itself what the Python layer would not ask for
    one, three = PL.resolve_selection("entropy", d.params).desc(), PL.resolve_selection("alluncert", d.params).desc()
    for desc, invert, gate, t, max_rows, msg in ((one, 0, 1, -0.5, 99, "tau"), (one, 0, 1, float("nan"), 99, "tau"), (one, 0, 1, tau, 0, "max_rows"),
                                                 (one, 1, 0, tau, 99, "invert needs"), (three, 0, 0, tau, 99, "need invert"),
                                                 (three, 1, 1, tau, 99, "gate 1")):
        assert d._lib.uda_pseudo_rows(d._h, C.byref(desc), invert, gate, C.c_float(min_score), C.c_double(t), max_rows) == 1
        assert msg in d._lib.uda_last_error(d._h).decode()
    usable()
    d.serve(imgs, post_mode="per_class")
    with pytest.raises(capi.UdaError, match="per class"):
        d.pseudo_rows("entropy", tau, min_score=min_score)
    d.stage_images(imgs)
    t = d.run_async()
    with pytest.raises(capi.UdaError, match="in flight"):
        d.pseudo_rows("entropy", tau, min_score=min_score)
    d.collect(t)
    d.serve(imgs)
    usable()
    p = dict(d.params, enable_softmax=False)
    fresh = KerasDriver("_", False, p["name"], 2, False, p, weights=d.weights)
    try:
        fresh.set_dropout_seed(SEED)
        with pytest.raises(capi.UdaError, match="no global post-process"):
            fresh.pseudo_rows("score", tau, min_score=min_score)
        fresh.serve(imgs)
        ent = PL.Selection("x", [[("entropy", "scalar", 1.0)]], {}, False, 0, 1, "tau", False)
        with pytest.raises(capi.UdaError, match="no entropy"):
            fresh.pseudo_rows(ent, tau, min_score=min_score)
        assert fresh.pseudo_rows("entropy", tau, min_score=min_score)[3].sum() > 0          # the reference's fallback: det_score
    finally:
        fresh.close()
