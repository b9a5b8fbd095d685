"""Thresholding, host side (`uda_amd.thresholding`; reference uncertainty_analysis.py:44-327): the numpy mirror (tests/thr_ref.py)
against what the reference's own `roc_metrics` / `_f_x` returned (tests/golden/thr_golden.npz), the seeded search with the mirror
as its evaluator, the result files, the columns from validation records, the verdict, and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import thr_ref as R
from uda_amd import capi, hparams_config, plan as plan_mod, writers
from uda_amd import thresholding as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "thr_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
NEW_SYMBOLS = ("uda_thr_objective_np",)


def gold_case(c):
    g = {k: GOLD["%s_%s" % (c, k)] for k in ("uncerts", "ious", "tp_class", "iou_thrs", "params", "thr", "rate", "auc", "loss")}
    g["fix_cd"], g["budget"], g["G"] = int(GOLD[c + "_fix_cd"]), float(GOLD[c + "_budget"]), int(GOLD[c + "_G"])
    g["group"] = GOLD[c + "_group"] if c + "_group" in GOLD.files else None
    return g


def assert_matches(got, g):
    """thr and rate identical (NaN = NaN, +inf = +inf), auc within N * 2^-52: the worst case of summing N terms that add up to at
    most 1 in another order."""
    thr, rate, auc = got
    N = g["uncerts"].shape[1]
    assert np.array_equal(thr, g["thr"], equal_nan=True)
    assert np.array_equal(rate, g["rate"], equal_nan=True)
    assert np.array_equal(np.isnan(auc), np.isnan(g["auc"]))
    ok = ~np.isnan(auc)
    assert (np.abs(auc[ok] - g["auc"][ok]) <= N * 2.0 ** -52).all()


def test_fixture_covers_what_it_should():
    assert str(GOLD["sklearn_version"]) and str(GOLD["numpy_version"])
    gs = [gold_case(c) for c in CASES]
    assert {g["uncerts"].shape[1] for g in gs} >= {2, 3, 5, 17, 64, 65, 257, 1025, 4099}
    assert {g["uncerts"].shape[0] for g in gs} == {1, 2, 3} and {g["iou_thrs"].size for g in gs} == {1, 6, 32}
    assert {g["params"].shape[0] for g in gs} == {1, 3, 64} and {g["G"] for g in gs} == {0, 3, 10}
    assert {(g["fix_cd"], g["budget"]) for g in gs} == {(0, 0.8), (0, 0.95), (1, 0.8), (1, 0.95)}
    for c, g in zip(CASES, gs):
        assert np.isnan(g["rate"]).all() == (c in ("allcorrect", "allwrong")) == bool(np.isnan(g["rate"]).any())
        if g["group"] is not None:
            assert g["G"] // 2 not in g["group"] and g["group"].max() == g["G"] - 1


@pytest.mark.parametrize("c", CASES)
def test_mirror_reproduces_the_reference(c):
    g = gold_case(c)
    got = R.roc_objective(g["uncerts"], g["ious"], g["tp_class"], g["iou_thrs"], g["params"], g["fix_cd"], g["budget"], g["group"])
    assert_matches(got, g)
    assert np.array_equal(TH.losses(got[1]), g["loss"])           # `_f_x` of the reference, through its stand-in study


# ------------------------------------------------------------------ the search, with the mirror as evaluator
def search_problem(seed=3, N=400):
    """Uncertainty 0 separates failures from correct detections (with overlap), uncertainty 1 is noise."""
    rng = np.random.default_rng(seed)
    tp = rng.random(N) < 0.9
    ious = np.round(rng.uniform(0.3, 1.0, N), 3)
    wrong = ~(tp & (ious >= 0.5))
    good = np.round(np.where(wrong, rng.normal(0.7, 0.2, N), rng.normal(0.3, 0.2, N)).clip(0, 2), 3)
    noise = np.round(rng.uniform(0, 1, N), 3)
    return dict(gt_classes=rng.integers(1, 4, N).astype(np.float64), tps_class=tp, ious=ious, uncert=[good, noise])


def optimal(tmp_path, **kw):
    args = dict(search_problem(), source_path=str(tmp_path), objective=R.roc_objective, population=24, rounds=4)
    args.update(kw)
    return TH.UncertOptimal(**args)


def test_search_is_deterministic_and_returns_the_minimum(tmp_path):
    a = optimal(tmp_path / "a")
    os.makedirs(a.source_path)
    pa = a.get_optimal_uncertainty()
    b = optimal(tmp_path / "b")
    os.makedirs(b.source_path)
    assert b.get_optimal_uncertainty() == pa and len(pa) == 2
    tried, loss = a.evaluated
    assert a.loss == loss.min() and np.array_equal(tried[int(np.argmin(loss))], pa)       # ties to the earliest
    assert np.array_equal(tried[:3], [[1, 0], [0, 1], [1, 1]]) and (tried >= 0).all() and (tried <= 1).all()
    corner = TH.losses(a.evaluate(np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]))[1])
    assert (a.loss <= corner).all()
    assert a.loss <= corner[0] < corner[1]           # the informative uncertainty alone beats the noise alone
    c = optimal(tmp_path / "c", seed=99)
    os.makedirs(c.source_path)
    assert c.get_optimal_uncertainty() != pa


def test_search_per_class(tmp_path):
    o = optimal(tmp_path, per_cls=True, added_name="_clsopt", population=12, rounds=2)
    p = o.get_optimal_uncertainty()
    assert len(p) == 2 * 3 and o.num_classes == 3
    tried, loss = o.evaluated
    assert np.array_equal(tried[:3], [[1, 0] * 3, [0, 1] * 3, [1] * 6]) and o.loss == loss.min()
    assert os.path.exists(os.path.join(str(tmp_path), "optimal_params_cd_0.95_iou_0.5_0.75_clsopt.txt"))


def test_default_budget_is_at_least_the_references():
    assert TH.DEFAULT_POPULATION * TH.DEFAULT_ROUNDS >= 1500


def test_files_round_trip_and_carry_the_references_names(tmp_path):
    o = optimal(tmp_path)
    p = o.get_optimal_uncertainty()
    names = sorted(os.listdir(str(tmp_path)))
    assert names == ["optimal_params_cd_0.95_iou_0.5_0.75.txt", "optimal_thrs_cd_0.95_iou_0.5_0.75.txt"]
    for name, want in zip(names, (p, o.opt_thrs)):
        text = open(os.path.join(str(tmp_path), name)).read()
        assert text == str(np.asarray(want, dtype="object"))
        assert [float(x.strip("[]")) for x in text.split()] == want           # the reference's parser
    assert len(o.opt_thrs) == 6
    again = TH.UncertOptimal(source_path=str(tmp_path), objective=None)      # nothing to search with: it must read
    assert again.get_optimal_uncertainty() == p and again.opt_thrs == o.opt_thrs
    fd = TH.result_paths("/x", dict(thr_cd=False, thr_fpr_tpr=0.9, thr_iou_thrs=[0.5]), "_a")
    assert fd == ("/x/optimal_params_fd_0.9_iou_0.5_0.5_a.txt", "/x/optimal_thrs_fd_0.9_iou_0.5_0.5_a.txt")


def test_hyper_parameters_and_their_table():
    h = hparams_config.default_detection_configs()
    assert h.thr_fpr_tpr == 0.95 and h.thr_cd is True and h.thr_sel_uncert == "ENTALBOX"
    assert h.thr_iou_thrs == list(np.round(np.arange(0.50, 0.76, 0.05), 2))
    for k in ("thr_fpr_tpr", "thr_cd", "thr_iou_thrs", "thr_sel_uncert"):
        assert "thresholding" in plan_mod.MODEL_PARAM_HANDLING[k]


def test_unavailable_methods_raise():
    for m in ("optuna", "hebo"):
        with pytest.raises(ValueError, match="population"):
            TH.UncertOptimal(method=m)


# ------------------------------------------------------------------ columns from validation records
def test_from_validate_records(tmp_path):
    f32 = np.float32
    filtered = {
        "names": ["a.png", "a.png", "b.png", "b.png"], "scores": f32([0.9, 0.8, 0.7, 0.6]),
        "boxes": f32([[10, 10, 50, 90], [0, 0, 20, 20], [30, 30, 60, 70], [5, 5, 15, 25]]),
        "gt_boxes": f32([[12, 8, 52, 88], [100, 100, 120, 120], [30, 30, 60, 70], [5, 10, 15, 30]]),
        "occlusions": [0, 1, 0, 2], "truncations": [0.0, 0.5, 0.0, 0.0], "classes": f32([1, 2, 3, 1]), "gt_classes": f32([1, 2, 2, 1]),
        "logits": np.zeros((4, 3), f32), "probab": np.full((4, 3), 1 / 3, f32), "entropy": f32([0.125, 0.5, 0.875, 0.25]),
        "albox": f32([[4, 8, 4, 8], [1, 1, 1, 1], [3, 4, 3, 4], [1, 2, 1, 2]])}
    params = dict(enable_softmax=True, loss_attenuation=True, calibrate_classification=True, calibrate_regression=True,
                  calib_method_class="iso_percls", calib_method_box="iso_perclscoo", thr_sel_uncert="ENTALBOX")
    cal = {"iso_percls_entropy": f32([0.25, 0.625, 1.0, 0.375]), "iso_perclscoo_albox": filtered["albox"] * f32(2)}
    recs = writers.validate_records(filtered, params, calibrated=cal)
    cols = TH.from_validate_records(recs, params)
    keep = [0, 2, 3]                                            # row 1 does not touch its ground truth
    assert cols["image_names"] == ["a.png", "b.png", "b.png"]
    np.testing.assert_array_equal(cols["tps_class"], [True, False, True])
    np.testing.assert_array_equal(cols["gt_classes"], [1, 2, 1])
    inter = 38.0 * 78.0
    np.testing.assert_array_equal(cols["ious"], [inter / (2 * 40 * 80 - inter), 1.0, 10.0 * 15 / (2 * 200 - 150)])
    np.testing.assert_array_equal(cols["uncert"][0], np.float64(filtered["entropy"])[keep])
    np.testing.assert_array_equal(cols["uncert"][1], [np.mean([4 / 40, 8 / 80, 4 / 40, 8 / 80]), np.mean([3 / 30, 4 / 40] * 2),
                                                      np.mean([1 / 10, 2 / 20] * 2)])
    calib = TH.from_validate_records(recs, params, calib=True)
    np.testing.assert_array_equal(calib["uncert"][0], np.float64(cal["iso_percls_entropy"])[keep])
    np.testing.assert_array_equal(calib["uncert"][1], 2 * cols["uncert"][1])
    only = TH.from_validate_records(recs, dict(params, thr_sel_uncert="ENT"))
    assert len(only["uncert"]) == 1
    path = str(tmp_path / "validate_results.txt")
    writers.write_validate_results(path, recs)
    from_file = TH.from_validate_records(path, params)
    for a, b in zip(from_file["uncert"] + [from_file["ious"]], cols["uncert"] + [cols["ious"]]):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="uncalib_albox"):
        TH.from_validate_records([{k: v for k, v in r.items() if k != "uncalib_albox"} for r in recs], params)


def test_autolabel_verdict():
    thrs = [0.4, 0.6]                                          # mean 0.5
    comp = np.array([[0.49], [0.5], [0.0], [0.7], [np.nextafter(0.5, 0)]])
    count = np.array([3, 2, 0, 1, 1], np.int32)
    np.testing.assert_array_equal(TH.autolabel_verdict((comp, count, None), thrs), [True, False, True, False, True])
    np.testing.assert_array_equal(TH.autolabel_verdict((np.array([[9.0]]), np.array([0])), thrs), [True])


# ------------------------------------------------------------------ refusals, in Python
def test_refusals():
    rng = np.random.default_rng(0)
    N = 8
    unc, iou, tp, thr, par = rng.random((2, N)), rng.random(N), np.ones(N), [0.5], [[1.0, 1.0]]

    def refuse(match, **kw):
        a = dict(uncerts=unc, ious=iou, tp_class=tp, iou_thrs=thr, params=par, budget=0.95)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            TH.check_problem(**a)

    for bad in (np.nan, np.inf, -np.inf):
        for key, val in (("uncerts", unc), ("ious", iou), ("params", np.asarray(par))):
            v = np.array(val, np.float64)
            v.flat[0] = bad
            refuse("NaN or inf", **{key: v})
    refuse("rows", uncerts=unc[:, :1], ious=iou[:1], tp_class=tp[:1])
    refuse("rows", uncerts=np.zeros((1, TH.MAX_N + 1)), ious=np.zeros(TH.MAX_N + 1), tp_class=np.zeros(TH.MAX_N + 1), params=[[1.0]])
    refuse("uncertainties", uncerts=rng.random((5, N)), params=[[1.0] * 5])
    refuse("IoU thresholds", iou_thrs=np.linspace(0, 1, 33))
    refuse("IoU thresholds", iou_thrs=[])
    refuse("candidates", params=np.zeros((TH.MAX_P + 1, 2)))
    refuse("candidates", params=np.zeros((0, 2)))
    refuse("groups", group=np.r_[np.zeros(N - 1), TH.MAX_G], params=np.zeros((1, 2 * (TH.MAX_G + 1))))
    refuse("group ids", group=np.r_[np.zeros(N - 1), -1], params=np.zeros((1, 2)))
    refuse("group ids", group=np.r_[np.zeros(N - 1), 0.5], params=np.zeros((1, 2)))
    refuse(r"params must be \[P, 2\]", params=[[1.0, 1.0, 1.0]])
    refuse("for uncerts of", ious=iou[:-1])
    for b in (0.0, 1.0, -0.1, np.nan):
        refuse("budget", budget=b)
    u, i, t, th, p, b, g, G = TH.check_problem(unc[:, ::2], iou[::2], tp[::2], thr, [1.0] * 6, 0.5, group=[0, 2, 2, 0])
    assert u.flags.c_contiguous and i.flags.c_contiguous and u.dtype == np.float64 and t.dtype == np.uint8
    assert g.dtype == np.int32 and G == 3 and p.shape == (1, 6) and th.dtype == np.float64 and b == 0.5
    with pytest.raises(ValueError, match=r"\[P, 6\]"):
        TH.check_problem(unc, iou, tp, thr, par, 0.5, group=np.r_[np.zeros(N - 1), 2])


def test_header_binding_and_library_have_the_new_symbol():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uda_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uda_[a-z0-9_]+)\s*\(", src))
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    for macro, val in (("UDA_THR_MAX_N", capi.THR_MAX_N), ("UDA_THR_MAX_U", capi.THR_MAX_U), ("UDA_THR_MAX_THRS", capi.THR_MAX_THRS),
                       ("UDA_THR_MAX_P", capi.THR_MAX_P), ("UDA_THR_MAX_G", capi.THR_MAX_G)):
        assert "#define %s %d" % (macro, val) in src
    assert (TH.MAX_N, TH.MAX_U, TH.MAX_K, TH.MAX_P, TH.MAX_G) == (262144, 4, 32, 65536, 8192)
    import uda_amd
    assert "thresholding" in open(os.path.join(uda_amd.PACKAGE_DIR, "__init__.py")).read()       # the package's module list
