"""Active-learning image scores, host side (`uda_amd.active_learning`; reference active_learning_loop.py:528-840): the numpy
restatement (tests/score_ref.py) against what the reference's own `score_image` / `select_images` returned
(tests/golden/score_golden.npz), the strategy grammar under four configurations, the accumulator and the selection against the
fixture through a stand-in driver, and the bound of the one numerical deviation from the file route (no 4-decimal rounding)."""
import ast
import os

import numpy as np
import pytest

import score_ref as S
from common import FULL_MC, HEAD_MC, LOSS_ATT, PLAIN, make_params
from uda_amd import active_learning as AL
from uda_amd import writers

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_golden.npz"))
MIN_SCORE = float(GOLD["min_score"][0])
OPT = tuple(float(v) for v in GOLD["opt_params"])
NAMES = [str(v) for v in GOLD["names"]]
IM_NAMES = [str(v) for v in GOLD["im_names"]]
CASES = [(str(d), str(s), int(k)) for d, s, k in zip(GOLD["case_dataset"], GOLD["case_strategy"], GOLD["case_num_per_iter"])]
COLUMN_KEYS = ("boxes", "scores", "classes", "entropy", "albox", "mcbox", "mcclass")


def gold_columns(ds):
    return {k: GOLD["%s_%s" % (ds, k)] for k in COLUMN_KEYS}, int(GOLD["%s_num_classes" % ds][0])


# ------------------------------------------------------------------ the restatement against the reference's own results
@pytest.mark.parametrize("ci", range(len(CASES)), ids=["%s-%s" % (c[0], c[1]) for c in CASES])
def test_restatement_equals_the_reference(ci):
    ds, strategy, npi = CASES[ci]
    cols, C = gold_columns(ds)
    comps, reduce_mean = S.components_of(strategy, OPT)
    comp, count, cls = S.score_columns(cols, comps, reduce_mean, MIN_SCORE, C)
    np.testing.assert_array_equal(count, GOLD["kept"])
    kept = count > 0
    assert (comp[~kept] == 0).all() and (cls[~kept] == 0).all() and (cls.sum(1) == count).all()
    # terms are non-negative and at most ~110 float64 additions are reordered: 110 * 2^-53 = 1.2e-14, two orders of margin
    np.testing.assert_allclose(comp[kept], GOLD["k%d_components" % ci], rtol=1e-12, atol=0)
    final = S.combine(comp[kept], S.combine_of(strategy, comp.shape[1]))
    np.testing.assert_allclose(final, GOLD["k%d_scores" % ci], rtol=0, atol=1e-10)
    names = [n for n, k in zip(NAMES, kept) if k]
    assert S.select(final, names, cls[kept], strategy, npi, IM_NAMES) == GOLD["k%d_selected" % ci].tolist()


def test_fixture_covers_what_it_should():
    strategies = " ".join(c[1] for c in CASES)
    for word in ("entropy", "mean_entropy", "alluncert", "highep_lowal", "sota", "epuncert", "ental", "combo", "box_norm_albox",
                 "box_albox", "class_mcclass", "foo", "perc_", "nee_", "bottomk_"):
        assert word in strategies
    assert {0, 1, 2, 7, 8, 9, 100} <= set(GOLD["kept"].tolist())
    assert {int(GOLD["%s_num_classes" % d][0]) for d in GOLD["datasets"]} == {3, 10}
    cols, _ = gold_columns("c")                                   # the `perc` dataset: nobody predicts the middle class
    assert sorted(set(cols["classes"][cols["scores"] > MIN_SCORE].astype(int))) == [1, 3]
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_golden.npz")) < 1 << 20


# ------------------------------------------------------------------ the strategy grammar
PARAMS = {"full_mc": FULL_MC, "head_mc": HEAD_MC, "loss_att": LOSS_ATT, "plain": PLAIN}
DET = [[("det_score", "scalar", 1.0)]]
# what a configuration without MC dropout (loss_att) / without any uncertainty head (plain) makes of the fixture strategies:
# a branch that reads a missing column raises, a key the file would not contain falls back to det_score
REDUCED = {
    "loss_att": {"alluncert": None, "mean_alluncert_highep_lowal": None, "sota": None, "epuncert": None, "class_mcclass": DET,
                 "box_norm_mcbox": DET, "perc_mean_alluncert": None, "nee_mean_epuncert": None, "bottomk_sota": None},
    "plain": {"alluncert": None, "mean_alluncert_highep_lowal": None, "sota": None, "epuncert": None, "ental": None,
              "mean_ental": None, "combo": None, "box_norm_albox": DET, "box_albox": DET, "class_mcclass": DET,
              "box_norm_mcbox": DET, "perc_mean_alluncert": None, "nee_mean_epuncert": None, "bottomk_sota": None},
}


@pytest.mark.parametrize("cfg", list(PARAMS))
def test_resolve_strategy(cfg):
    p = make_params(**PARAMS[cfg])
    for strategy in sorted({c[1] for c in CASES}):
        want, reduce_mean = S.components_of(strategy, OPT)
        want = REDUCED.get(cfg, {}).get(strategy, want)
        if want is None:
            with pytest.raises(ValueError, match="does not emit"):
                AL.resolve_strategy(strategy, p, OPT)
            continue
        st = AL.resolve_strategy(strategy, p, OPT)
        assert [[tuple(t) for t in comp] for comp in st.components] == want, strategy
        assert st.reduce_mean == reduce_mean and not st.calibrated
        assert st.combine == S.combine_of(strategy, len(want))
        d = st.desc()
        assert d.n_comp == len(want) and d.reduce_mean == int(reduce_mean)
        for k, comp in enumerate(want):
            assert d.n_terms[k] == len(comp)
            for t, (src, tr, w) in enumerate(comp):
                assert (d.term[k][t].source, d.term[k][t].transform, d.term[k][t].weight) == (AL.SOURCES[src], AL.TRANSFORMS[tr], w)


def test_resolve_strategy_errors_and_calibrated_names():
    p = make_params(**FULL_MC)
    for bad in ("logits", "probab", "mean_logits", "calib_probab"):
        with pytest.raises(ValueError, match="does not score"):
            AL.resolve_strategy(bad, p)
    with pytest.raises(ValueError, match="opt_params"):
        AL.resolve_strategy("combo", p)
    with pytest.raises(ValueError, match="combo"):
        AL.resolve_strategy("combo_alluncert", p, OPT)
    with pytest.raises(ValueError, match="highep_lowal"):
        AL.resolve_strategy("epuncert_highep_lowal", p)
    assert AL.resolve_strategy("probab", make_params(enable_softmax=False)).components == DET     # not in such a file: fallback
    assert AL.resolve_strategy("bbox", p).components == DET       # contains "box": the key becomes uncalib_bbox, which no line has
    assert AL.resolve_strategy("entropy", make_params(enable_softmax=False)).components == DET
    st = AL.resolve_strategy("calib_alluncert", p)
    assert st.calibrated and st.columns == {"mcbox": "iso_perclscoo_mcbox", "albox": "iso_perclscoo_albox", "mcclass": "iso_percls_mcclass"}
    st = AL.resolve_strategy("calib_ental", p)
    assert st.columns == {"albox": "iso_perclscoo_albox", "entropy": "iso_percls_entropy"}
    st = AL.resolve_strategy("calib_combo", p, OPT)
    assert st.columns == {"albox": "iso_perclscoo_albox", "entropy": "iso_percls_entropy"} and st.components[0][0][2] == OPT[0]
    st = AL.resolve_strategy("calib_box_norm_albox", p)
    assert st.columns == {"albox": "iso_perclscoo_albox"} and st.components == [[("albox", "rel_mean", 1.0)]]
    st = AL.resolve_strategy("calib_class_mcclass", p)
    assert st.columns == {"mcclass": "iso_percls_mcclass"} and st.components == [[("mcclass", "mean", 1.0)]]
    st = AL.resolve_strategy("calib_entropy", p)
    assert st.columns == {"entropy": "iso_percls_entropy"} and st.calibrated
    assert not AL.resolve_strategy("box_albox", p).calibrated


def test_default_min_score():
    p = make_params()
    nms = dict(p["nms_configs"])
    assert AL.default_min_score(dict(p, nms_configs=dict(nms, score_thresh=0.25))) == 0.25
    assert AL.default_min_score(dict(p, nms_configs=dict(nms, score_thresh=0.0)), average_score=0.6) == 0.6
    assert AL.default_min_score(dict(p, nms_configs=dict(nms, score_thresh=None))) == 0.4
    assert AL.default_min_score(dict(p, nms_configs=dict(nms, score_thresh=0.25)), ssl=True) == 0.1


# ------------------------------------------------------------------ accumulator + selection through a stand-in driver
class RefDriver:
    """`score_images` of a ServingDriver whose resident batch is a slice of the fixture's columns, scored by the restatement."""

    def __init__(self, cols, num_classes):
        self.cols, self.num_classes, self.batch = cols, num_classes, None

    def serve_resident(self, rows):
        self.batch = {k: v[rows] for k, v in self.cols.items()}
        return len(rows)

    def score_images(self, strategy, min_score, opt_params=None):
        st = AL.resolve_strategy(strategy, dict.fromkeys(AL.SOURCES), opt_params)
        return S.score_columns(self.batch, st.components, st.reduce_mean, min_score, self.num_classes)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=["%s-%s" % (c[0], c[1]) for c in CASES])
def test_image_scores_and_select_images(ci):
    ds, strategy, npi = CASES[ci]
    cols, C = gold_columns(ds)
    drv = RefDriver(cols, C)
    acc = AL.ImageScores(AL.resolve_strategy(strategy, dict.fromkeys(AL.SOURCES), OPT))
    for rows in (range(0, 4), range(4, 5), range(5, 13)):       # the second batch holds only the image with nothing kept
        drv.serve_resident(list(rows))
        acc.add([NAMES[i] for i in rows], drv.score_images(strategy, MIN_SCORE, OPT))
    assert len(acc) == 12 and acc.names == [n for n, k in zip(NAMES, GOLD["kept"]) if k]
    np.testing.assert_array_equal(acc.count, GOLD["kept"][GOLD["kept"] > 0])
    np.testing.assert_allclose(acc.components, GOLD["k%d_components" % ci], rtol=1e-12, atol=0)
    np.testing.assert_allclose(acc.scores(), GOLD["k%d_scores" % ci], rtol=0, atol=1e-10)
    assert acc.select(npi, IM_NAMES) == GOLD["k%d_selected" % ci].tolist()
    assert AL.select_images(GOLD["k%d_scores" % ci], acc.names, acc.class_counts, strategy, npi, IM_NAMES) == \
        GOLD["k%d_selected" % ci].tolist()


def test_image_scores_refuses_mismatched_names_and_empty():
    acc = AL.ImageScores(AL.resolve_strategy("entropy", dict.fromkeys(AL.SOURCES)))
    with pytest.raises(ValueError, match="nothing scored"):
        acc.scores()
    with pytest.raises(ValueError, match="names"):
        acc.add(["a.jpg"], (np.zeros((2, 1)), np.ones(2, np.int32), np.ones((2, 3), np.int32)))


# ------------------------------------------------------------------ deviation 1: the file's 4-decimal rounding
def synthetic_unpacked(seed, n=6, M=40, C=7):
    """float32 columns as `serve_unpacked` returns them: KITTI-sized boxes with sides of 8 to 200 px, box stds of a few
    pixels, class stds below 1, entropies below log2(C), descending scores that cross the threshold inside the list."""
    rng = np.random.default_rng(seed)
    y1, x1 = rng.uniform(0, 300, (n, M)), rng.uniform(0, 1000, (n, M))
    h, w = rng.uniform(8.5, 200, (n, M)), rng.uniform(8.5, 200, (n, M))
    boxes = np.stack([y1, x1, y1 + h, x1 + w], -1).astype(np.float32)
    scores = np.sort(rng.uniform(0.05, 0.95, (n, M)), 1)[:, ::-1].astype(np.float32)
    scores[0] = 0.1                                               # an image with nothing above the threshold
    classes = rng.integers(1, C + 1, (n, M)).astype(np.float32)
    logits = rng.normal(0, 2, (n, M, C)).astype(np.float32)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    probab = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    entropy = (-np.sum(probab * np.log2(np.maximum(probab, 1e-7)), -1)).astype(np.float32)
    return dict(boxes=boxes, scores=scores, classes=classes, logits=logits, probab=probab, entropy=entropy,
                albox=rng.gamma(2.0, 1.0, (n, M, 4)).astype(np.float32), mcbox=rng.gamma(2.0, 0.5, (n, M, 4)).astype(np.float32),
                mcclass=rng.gamma(2.0, 0.15, (n, M, C)).astype(np.float32)), C


def parse_file_columns(un, lines, min_score):
    """The columns as the file holds them: float64 [n, M, ...], rows the writer skipped stay 0."""
    n, M = un["scores"].shape
    out = {k: np.zeros(un[k].shape, np.float64) for k in COLUMN_KEYS}
    it = iter(lines)
    for i in range(n):
        for r in np.where(un["scores"][i] > min_score)[0]:
            d = ast.literal_eval(next(it).replace("inf", "2e308"))
            assert d["image_name"] == "im%d.jpg" % i
            out["scores"][i, r], out["boxes"][i, r], out["classes"][i, r] = d["det_score"], d["bbox"], d["class"]
            out["entropy"][i, r], out["albox"][i, r] = d["entropy"], d["uncalib_albox"]
            out["mcbox"][i, r], out["mcclass"][i, r] = d["uncalib_mcbox"], d["uncalib_mcclass"]
    assert next(it, None) is None
    return out


@pytest.mark.parametrize("strategy", ["entropy", "mean_entropy", "alluncert", "mean_alluncert", "epuncert", "mean_ental", "combo",
                                      "box_norm_albox", "mean_box_albox", "class_mcclass", "foo"])
def test_rounding_of_the_file_route_stays_within_the_stated_bound(strategy, tmp_path):
    """DESIGN 12, deviation 1: per component at most 5e-5 / (min kept side) for a relativized term and 5e-5 for any other,
    times the weights."""
    min_score = 0.4
    un, C = synthetic_unpacked(5)
    recs = writers.prediction_records(un, ["im%d" % i for i in range(un["scores"].shape[0])], min_score)
    path = str(tmp_path / "prediction_data.txt")
    writers.write_prediction_data(path, recs)
    filed = parse_file_columns(un, open(path).readlines(), min_score)
    exact = {k: un[k].astype(np.float64) for k in COLUMN_KEYS}
    comps, reduce_mean = S.components_of(strategy, OPT)
    a, ca, _ = S.score_columns(filed, comps, reduce_mean, min_score, C)
    b, cb, _ = S.score_columns(exact, comps, reduce_mean, np.float32(min_score), C)
    np.testing.assert_array_equal(ca, cb)
    assert ca[0] == 0 and (ca[1:] > 0).all() and (ca < un["scores"].shape[1]).any()
    side = np.minimum(un["boxes"][..., 2] - un["boxes"][..., 0], un["boxes"][..., 3] - un["boxes"][..., 1]).astype(np.float64)
    worst = 0.0
    for i in np.nonzero(ca)[0]:
        min_side = side[i][un["scores"][i] > min_score].min()
        for k, comp in enumerate(comps):
            bound = sum(abs(w) * (5e-5 / min_side if tr == "rel_mean" else 5e-5) for _, tr, w in comp)
            worst = max(worst, abs(a[i, k] - b[i, k]) / bound)
            assert abs(a[i, k] - b[i, k]) <= bound * 1.01, (i, k, a[i, k], b[i, k], bound)
    print("%s: largest difference / bound = %.3f" % (strategy, worst))
    assert worst > 0 or strategy == "foo"            # the route does round: the comparison is not vacuous


def test_sample_sharded_driver_points_to_the_host_array_path():
    from uda_amd import dist
    for call in (lambda: dist.SampleShardedDriver.score_images(None, "entropy", 0.4),
                 lambda: dist.SampleShardedDriver.serve_score(dist.SampleShardedDriver.__new__(dist.SampleShardedDriver), [], "entropy", 0.4)):
        with pytest.raises(ValueError, match="score_detections"):
            call()
