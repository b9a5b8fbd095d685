"""The evaluation services at their wave, block and cap boundaries on the device: every case of tests/service_cases.py through
its handle-free entry point against the numpy mirror, compared exactly as the service's own device test compares it; the two
calibration kernels on tables built from the served values themselves (one point, two points, thresholds that ARE observed
values with a plateau, a range that excludes both tails, classes without a table); the consistency scores at max_output_size
128 and 1.  tests/test_service_cases_host.py asserts on the CPU that every case reaches the boundary it is named after."""
import numpy as np
import pytest

import service_cases as SC
from common import FULL_MC, HEAD_MC, LOSS_ATT, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ assign
@pytest.mark.parametrize("name", SC.ASSIGN_CASES)
def test_assign(name):
    """Indices and counts equal, IoU within 1e-12.  At M = 4095 the block asks for 65524 bytes of LDS, at 4096 for 65540 (4 static
    bytes beside 64 KiB): the runtime grants both launches as they are, and the last staged box (rank 4095) wins its row."""
    from uda_amd import utils_extra as U
    c = SC.assign_case(name)
    worst = 0.0
    for method in SC.ASSIGN_METHODS:
        for keep in SC.ASSIGN_KEEPS:
            want = SC.expected_assign(name, method, keep)
            if want is None:                             # a kept row without a detection: refused, never answered
                with pytest.raises(ValueError):
                    U.assign_gt_boxes(method, c["gt_boxes"], c["gt_classes"], c["dets"], keep=keep)
                continue
            idx, iou, count = U.assign_gt_boxes(method, c["gt_boxes"], c["gt_classes"], c["dets"], keep=keep)
            np.testing.assert_array_equal(idx, want[0], err_msg="%s %s" % (method, keep))
            np.testing.assert_array_equal(count, want[2])
            assert iou.dtype == np.float64
            np.testing.assert_allclose(iou, want[1], rtol=0, atol=1e-12)
            worst = max(worst, float(np.abs(iou - want[1]).max()) if iou.size else 0.0)
    print("assign %s: worst IoU error %.3g (bound 1e-12)" % (name, worst))


def test_assign_without_detections_is_an_error_of_the_library_too():
    """M = 0 with a kept row, past the wrapper's own check: an error return with a message, not index 0 of nothing."""
    from uda_amd import capi
    lib = capi.load()
    gb, gc = np.array([[[1, 2, 3, 4]]], np.float32), np.array([[2]], np.float32)
    idx, iou, count = np.full((1, 1), 7, np.int32), np.zeros((1, 1)), np.zeros((1,), np.int32)
    for method in (capi.ASSIGN_IOU, capi.ASSIGN_MSE, capi.ASSIGN_RANK):
        rc = lib.uda_assign_gt_np(0, None, gb.ctypes.data, gc.ctypes.data, 1, 0, 1, method, capi.ASSIGN_KEEP_VALIDATE, idx.ctypes.data,
                                  iou.ctypes.data, count.ctypes.data)
        assert rc != 0 and "0 detections" in lib.uda_last_error(None).decode() and idx[0, 0] == 7
    rc = lib.uda_assign_gt_np(0, None, gb.ctypes.data, gc.ctypes.data, 1, 0, 1, capi.ASSIGN_IOU, capi.ASSIGN_KEEP_CALIBRATE, idx.ctypes.data,
                              iou.ctypes.data, count.ctypes.data)
    assert rc == 0 and idx[0, 0] == -1 and count[0] == 0


# ------------------------------------------------------------------ score
def _strategy(c, name):
    from uda_amd import active_learning as AL
    srcs = {t[0] for comp in c["components"] for t in comp}
    return AL.Strategy(name, c["components"], c["reduce_mean"], {s: s for s in srcs}, False, None)


@pytest.mark.parametrize("name", SC.SCORE_CASES)
def test_score(name):
    """Counts equal, components within rtol 1e-12 of the mirror, the float32 and float64 instantiations bit-identical."""
    from uda_amd import active_learning as AL
    c = SC.score_case(name)
    st = _strategy(c, name)
    want, wcount, wcls = SC.expected_score(name)
    got64 = AL.score_detections(SC.as64(c["cols"]), st, c["min_score"], num_classes=c["num_classes"])
    got32 = AL.score_detections(c["cols"], st, c["min_score"], num_classes=c["num_classes"], as_float32=True)
    for comp, count, cls in (got64, got32):
        np.testing.assert_array_equal(count, wcount)
        np.testing.assert_array_equal(cls, wcls)
        np.testing.assert_allclose(comp, want, rtol=1e-12, atol=0)
    assert np.array_equal(got64[0].view(np.uint64), got32[0].view(np.uint64))
    print("score %s: worst relative error %.3g (bound 1e-12)" % (name, float(np.max(np.abs(got64[0] - want) / np.abs(want)))))


# ------------------------------------------------------------------ pseudo
@pytest.mark.parametrize("name", SC.PSEUDO_CASES)
def test_pseudo(name):
    """Rows, classes and counts exact, values within 1e-12, the selection `pseudo_ref.same_selection` to the mirror's, the two
    instantiations bit-identical."""
    import pseudo_ref as R
    from uda_amd import active_learning as AL, pseudo_labels as PL
    c = SC.pseudo_case(name)
    cols = SC.as64(c["cols"])
    (res, minmax, kept, cand, _), selection = SC.expected_pseudo(name)
    sel = PL.resolve_selection(SC.PSEUDO_STRATEGY, dict.fromkeys(AL.SOURCES))
    got = PL.select_detections(cols, sel, SC.PSEUDO_TAU, SC.PSEUDO_MIN, num_classes=c["num_classes"], max_rows=c["max_rows"])
    rec = got[0]
    for f in ("image", "row", "cls"):
        np.testing.assert_array_equal(rec[f], res[f], err_msg=f)
    np.testing.assert_array_equal(got[2], kept)
    np.testing.assert_array_equal(got[3], cand)
    np.testing.assert_allclose(rec["v"], res["v"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[1], minmax, rtol=1e-12, atol=0)
    assert (rec["box"] == c["cols"]["boxes"][rec["image"], rec["row"]]).all() and (rec["det_score"] == c["cols"]["scores"][rec["image"], rec["row"]]).all()
    acc = PL.PseudoLabelSet(sel, SC.PSEUDO_TAU)
    acc.add(c["names"], got, boxes=cols["boxes"])
    R.same_selection(acc.finalize(), selection)
    f32 = PL.select_detections(c["cols"], sel, SC.PSEUDO_TAU, SC.PSEUDO_MIN, num_classes=c["num_classes"], max_rows=c["max_rows"], as_float32=True)
    assert got[0].tobytes() == f32[0].tobytes() and np.array_equal(got[1].view(np.uint64), f32[1].view(np.uint64))
    np.testing.assert_array_equal(got[2], f32[2])
    np.testing.assert_array_equal(got[3], f32[3])
    print("pseudo %s: worst relative error %.3g (bound 1e-12)" % (name, float(np.max(np.abs(rec["v"] - res["v"]) / np.abs(res["v"])))))


# ------------------------------------------------------------------ coco
@pytest.mark.parametrize("name", SC.COCO_CASES)
def test_coco(name):
    """Records (every row, not the evaluated ones only: the mirror defines them all), npig and used equal."""
    from uda_amd import coco_metric as CM
    c = SC.coco_case(name)
    want = SC.expected_coco(name)
    rec, npig, used = CM.match_np(c["det"], c["gt"], c["num_classes"], c["thrs"])
    for f in ("score", "cls", "rank", "matched", "ignored"):
        np.testing.assert_array_equal(rec[f], want[0][f], err_msg=f)
    np.testing.assert_array_equal(npig, want[1])
    np.testing.assert_array_equal(used, want[2])


# ------------------------------------------------------------------ thr
@pytest.mark.parametrize("name", SC.THR_CASES)
def test_thr(name):
    from test_gpu_thr import assert_matches
    from uda_amd import thresholding as TH
    c = SC.thr_case(name)
    for fix_cd in (1, 0):
        got = TH.roc_objective(c["uncerts"], c["ious"], c["tp_class"], c["iou_thrs"], c["params"], fix_cd, c["budget"], c["group"])
        assert_matches(got, SC.expected_thr(name, fix_cd), c["uncerts"].shape[1])


# ------------------------------------------------------------------ calibration on tables built from the served values
def _serve(cfg):
    from uda_amd.infer_lib import KerasDriver
    p = make_params(**cfg)
    d = KerasDriver("_", False, p["name"], batch_size=2, only_network=False, model_params=p, weights=make_weights(p, cls_spread=20.0))
    d.set_dropout_seed(5)
    return d, d.serve(make_images(2, 128, 192))


@pytest.fixture(scope="module")
def served_full():
    d, det = _serve(FULL_MC)
    yield d, det
    d.close()


@pytest.fixture(scope="module")
def served_la():
    d, det = _serve(LOSS_ATT)
    yield d, det
    d.close()


def edge_tables(values, rng, top=60.0, flat=False):
    """The four tables of the issue from observed values: one point; two points; thresholds that are observed values, with a
    plateau in ys; a range without the lowest and the highest tenth.  flat: ys follows a curve of slope <= 0.9 with a plateau
    (for inputs the device computes itself: an input one ulp off a threshold moves the output by as little)."""
    v = np.unique(np.asarray(values, np.float64))
    assert len(v) >= 12
    pick = v[np.unique(np.linspace(0, len(v) - 1, 24).astype(int))][2:-2]          # (the tails stay outside: clipped on both sides)
    inner = np.linspace(*np.quantile(v, [0.1, 0.9]), 9)
    mid, quart = v[[len(v) // 2]], v[[len(v) // 4, 3 * len(v) // 4]]
    if flat:
        a, b = pick[5], pick[7]
        curve = lambda x: 0.05 + 0.9 * np.minimum(x, a) + 0.9 * np.maximum(0.0, x - b)      # noqa: E731
        out = {"one": (mid, curve(mid)), "two": (quart, curve(quart)), "hits": (pick, curve(pick)), "inner": (inner, curve(inner))}
    else:
        ys = np.sort(rng.uniform(0, top, len(pick)))
        ys[5:8] = ys[5]
        out = {"one": (mid, np.array([0.35 * top])), "two": (quart, np.array([0.1, 0.2]) * top), "hits": (pick, ys),
               "inner": (inner, np.sort(rng.uniform(0, top, 9)))}
    assert (out["hits"][1][5:8] == out["hits"][1][5]).all() and np.all(np.diff(pick) > 0) and np.all(np.diff(inner) > 0)
    return out


def _iso(tables):
    from uda_amd.calibration import IsoTable
    return [IsoTable(*t) for t in tables]


def _box_raw(d, n, col0, relative, tables):
    """uda_calibrate_box in its per-(class, coordinate) mode with a table list that may hold None: a class without a table is an
    empty table (the wrapper's IsoTable cannot state one)."""
    from uda_amd import capi
    out = np.empty((n, d.M, 4), np.float32)
    off = np.zeros(len(tables) + 1, np.int32)
    off[1:] = np.cumsum([0 if t is None else len(t[0]) for t in tables])
    xs = np.ascontiguousarray(np.concatenate([np.asarray(t[0], np.float64) for t in tables if t is not None]))
    ys = np.ascontiguousarray(np.concatenate([np.asarray(t[1], np.float64) for t in tables if t is not None]))
    d._ck(d._lib.uda_calibrate_box(d._h, col0, capi.CALIB_ISO_PERCLSCOO, int(relative), len(tables), off.ctypes.data, xs.ctypes.data,
                                   ys.ctypes.data, None, out.ctypes.data), "uda_calibrate_box")
    return out


def _check_box(got, want, x, table, seen, exact_value=True):
    """got / want / x: the outputs and the inputs one table served.  Existing tolerance everywhere; exact where the input IS a
    threshold (both sides reduce to ys[j] + slope * 0)."""
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-6)
    xs, ys = table
    j = np.searchsorted(xs, x.astype(np.float64))
    hit = (j < len(xs)) & (xs[np.minimum(j, len(xs) - 1)] == x)
    np.testing.assert_array_equal(got[hit], want[hit])
    if exact_value:
        np.testing.assert_array_equal(want[hit], ys[j[hit]].astype(np.float32))
    seen["hits"] += int(hit.sum())
    seen["below"] += int((x < xs[0]).sum())
    seen["above"] += int((x > xs[-1]).sum())
    return float(np.abs(got - want).max()) if got.size else 0.0


def test_box_calibration_on_tables_of_served_values(served_full):
    from oracle import calib_ref as CR
    from uda_amd.calibration import BoxCalibrator
    d, det = served_full
    C = d.params["num_classes"]
    rng = np.random.default_rng(31)
    cls_all = det[2][..., 0]
    present = np.unique(cls_all[cls_all >= 1]).astype(int)
    K = int(present[len(present) // 2]) if len(present) > 1 else 0       # classes 1 .. K get tables, the classes above none
    assert 1 <= K < present.max(), "fewer than two classes among the served rows"
    worst = 0.0
    for which, col0 in (("albox", 4), ("mcbox", 8)):
        unc = np.nan_to_num(det[0][..., col0:col0 + 4])
        seen = dict(hits=0, below=0, above=0, tableless=0)
        # one table for everything, each of the four kinds
        for kind, table in edge_tables(unc.ravel(), rng).items():
            got = BoxCalibrator(d, {"iso_all": _iso([table])[0]}).calibrate_boxuncert(2, which, "iso_all")
            for n in range(2):
                want = CR.calibrate_boxuncert("iso_all", {"iso_all": table}, C, unc[n], cls_all[n], det[0][n][:, :4])
                worst = max(worst, _check_box(got[n], want, unc[n], table, seen))
        # one table per coordinate, a kind each
        tabs = [edge_tables(unc[..., j].ravel(), rng)[kind] for j, kind in enumerate(("one", "two", "hits", "inner"))]
        got = BoxCalibrator(d, {"iso_percoo": _iso(tabs)}).calibrate_boxuncert(2, which, "iso_percoo")
        for n in range(2):
            want = CR.calibrate_boxuncert("iso_percoo", {"iso_percoo": tabs}, C, unc[n], cls_all[n], det[0][n][:, :4])
            for j in range(4):
                worst = max(worst, _check_box(got[n][:, j], want[:, j], unc[n][:, j], tabs[j], seen))
        # one table per (class, coordinate) for classes 1 .. K only; plain and relative to the box side
        boxes = det[0][..., :4]
        norm = np.stack([boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]] * 2, -1)
        rel = np.divide(unc, norm, out=np.zeros_like(unc), where=norm != 0, dtype=np.float16)
        for relative, src, method in ((0, unc, "iso_perclscoo"), (1, rel, "rel_iso_perclscoo")):
            tabs = []
            for ci in range(1, K + 1):
                for j in range(4):
                    vals = src[..., j][cls_all == ci]
                    kinds = edge_tables(vals, rng, top=3.0 if relative else 60.0) if len(np.unique(vals)) >= 12 else None
                    tabs.append(kinds[("hits", "inner", "two", "one")[(ci + j) % 4]] if kinds else (np.unique(vals)[:1].astype(np.float64), np.array([1.5])))
            got = _box_raw(d, 2, col0, relative, tabs + [None] * (4 * (C - K)))
            for n in range(2):
                want = CR.calibrate_boxuncert(method, {method: tabs}, K, unc[n], cls_all[n], boxes[n])
                np.testing.assert_allclose(got[n], want, rtol=2e-6, atol=1e-6, err_msg=method)
                none = cls_all[n].astype(int) > K
                assert (want[none] == 0).all() and (got[n][none] == 0).all()
                seen["tableless"] += int(none.sum())
                for ci in range(1, K + 1):
                    rows = cls_all[n].astype(int) == ci
                    for j in range(4 if rows.any() else 0):
                        # (relative: the output is table value * box side - compared exactly, not restated)
                        worst = max(worst, _check_box(got[n][rows, j], want[rows, j], src[n][rows, j], tabs[(ci - 1) * 4 + j], seen,
                                                      exact_value=not relative))
        assert min(seen.values()) > 0, (which, seen)
        print("box calibration %s: %s" % (which, seen))
    print("box calibration: worst absolute error %.3g (bound 2e-6 relative + 1e-6)" % worst)


@pytest.mark.parametrize("with_unc", [False, True], ids=["loss_att", "full_mc"])
def test_class_calibration_on_tables_of_served_values(with_unc, served_full, served_la):
    from oracle import calib_ref as CR
    from uda_amd.calibration import ClassCalibrator
    d, det = served_full if with_unc else served_la
    C = d.params["num_classes"]
    rng = np.random.default_rng(37)
    logits = det[4].reshape(-1, C)
    unc = det[2][..., 1:].reshape(-1, C) if with_unc else None
    p = CR._stable_softmax(logits)
    seen = dict(hits=0, below=0, above=0)

    def check(method, model, dev_model):
        cal = ClassCalibrator(d, {method: dev_model}, calib_method=method, draws=10, seed=77)
        got = cal.perform_class_calib(2, method)
        want = CR.perform_class_calib(method, {method: model}, logits, unc, draws=10, seed=77)
        assert len(got) == len(want) == (3 if with_unc else 2)
        np.testing.assert_allclose(got[1].reshape(-1, C), want[1], rtol=5e-5, atol=2e-6, err_msg=method)
        np.testing.assert_allclose(got[0].reshape(-1), want[0], rtol=1e-4, atol=1e-5, err_msg=method)
        if with_unc:
            np.testing.assert_allclose(got[2].reshape(-1, C), want[2], rtol=1e-3, atol=2e-6, err_msg=method)
        return float(np.abs(got[1].reshape(-1, C) - want[1]).max())

    def count(x, table):
        xs = table[0]
        seen["hits"] += int(np.isin(x.astype(np.float64), xs).sum())
        seen["below"] += int((x < xs[0]).sum())
        seen["above"] += int((x > xs[-1]).sum())

    worst = 0.0
    for kind, table in edge_tables(p.ravel(), rng, flat=True).items():
        worst = max(worst, check("iso_all", table, _iso([table])[0]))
        count(p.ravel(), table)
    tabs = [edge_tables(p[:, c], rng, flat=True)[("hits", "inner", "two", "one")[c % 4]] for c in range(C)]
    worst = max(worst, check("iso_percls", tabs, _iso(tabs)))
    for c in range(C):
        count(p[:, c], tabs[c])
    assert min(seen.values()) > 0, seen
    # a class without a table cannot be stated here: the library wants a threshold in every table, and says so
    off = np.zeros(C + 1, np.int32)
    off[2:] = np.cumsum([len(t[0]) for t in tabs[1:]])
    xs, ys = np.concatenate([t[0] for t in tabs[1:]]), np.concatenate([t[1] for t in tabs[1:]])
    probs, ent = np.empty((2, d.M, C), np.float32), np.empty((2, d.M), np.float32)
    from uda_amd import capi
    rc = d._lib.uda_calibrate_class(d._h, capi.CLS_ISO_PERCLS, C, off.ctypes.data, xs.ctypes.data, ys.ctypes.data, None, 0,
                                    capi.C.c_uint64(0), probs.ctypes.data, ent.ctypes.data, None)
    assert rc != 0 and "at least one threshold" in d._lib.uda_last_error(d._h).decode()
    print("class calibration (MC std %s): %s, worst absolute error of the probabilities %.3g" % (with_unc, seen, worst))


# ------------------------------------------------------------------ consistency at the largest and the smallest max_output_size
@pytest.mark.parametrize("M", [128, 1])
def test_consistency_at_max_output_size(M):
    from test_gpu_consistency import _check_scores
    from uda_amd.infer_lib import KerasDriver
    nms = dict(method="gaussian", iou_thresh=None, score_thresh=0.0125, sigma=None, pyfunc=False, max_nms_inputs=0, max_output_size=M)
    p = make_params(image_size="256x128", consistency_ssl=True, nms_configs=nms, **HEAD_MC)
    d = KerasDriver("_", False, p["name"], 2, False, p, weights=make_weights(p, seed=12, cls_spread=20.0))
    try:
        d.set_dropout_seed(23)
        assert d.M == M
        imgs = make_images(2, 140, 260, seed=3)
        det, iou, agree = d.serve_consistency(imgs)
        assert iou.shape == agree.shape == (2, M) and iou.dtype == np.float64
        _check_scores(d, imgs, det, iou, agree)
        assert det[3].max() > 0 and (iou > 0).any()
        if M == 128:
            assert det[3].min() < M, "no padded row: the kernel's last staged rows were all real"
        print("consistency M = %d: valid_len %s" % (M, det[3].tolist()))
    finally:
        d.close()
