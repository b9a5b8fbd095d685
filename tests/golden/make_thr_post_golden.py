"""Generates tests/golden/thr_post_golden.npz by running the REAL reference methods `MainUncertViz._plot_validheat`,
`_plot_metricsspider`, `_collect_postthresholding` and `_collect_thresh_results` (src/uncertainty_analysis.py:734-749, :838-880,
:920-1101) on `object.__new__(MainUncertViz)` with the members set by hand.  The module's imports are stubbed the way
make_thr_report_golden.py stubs them (sklearn is real); the stand-ins record what the methods would have drawn: the array given to
`imshow`, keyed by the name given to the `savefig` that follows; the `det` rows given to the polar axis' `plot`; the
`(img_name, label)` pairs given to `_draw_postthresholding`.  `get_dataset_data(...)[-2]` is the case's mask size, `random.seed` is
set per case, every directory lies under a temporary one.  Run once where a checkout of the reference and sklearn exist; the .npz
(data only) is committed and is what the tests read.

    python tests/golden/make_thr_post_golden.py <src directory of the reference's checkout>

Every input is a float32-representable value on a coarse grid (quarter pixels, 1/1024 for sigma and entropy) and is stored as
float32, which keeps the file small; the tests read it back as float64, the values the reference saw.  Per case the fixture holds
the inputs, the recorded maps (`map_<stem>`), the spider rows [3, 5], the four image lists, and the threshold and mask sums of
`_collect_thresh_results` at the largest IoU threshold.

Asserted below: every ranking case has at least 12 images on which nothing is removed (the reference samples 10 of them; else:
another seed) and equal per-image counts inside a top list, so that the tie rule is exercised."""
import os
import random
import sys
import tempfile
import warnings
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_thr_post_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]

for name in ("optuna", "dataset_data", "hebo", "hebo.design_space", "hebo.design_space.design_space", "hebo.optimizers",
             "hebo.optimizers.hebo", "hparams_config", "matplotlib", "matplotlib.pyplot", "matplotlib.patches", "mpl_toolkits",
             "mpl_toolkits.axes_grid1", "PIL", "utils_box", "utils_infer", "utils_extra", "tensorflow", "uncertainty_toolbox",
             "uncertainty_toolbox.viz", "absl"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
import numpy as np                       # noqa: E402
import sklearn                           # noqa: E402
import uncertainty_analysis as UA        # noqa: E402  (the reference module)


class _Rec:
    pending, maps, spider, drawn = None, {}, [], []

    @classmethod
    def reset(cls):
        cls.pending, cls.maps, cls.spider, cls.drawn = None, {}, [], []


class _HeatAx:
    def imshow(self, mask, **kw):
        _Rec.pending = np.array(mask, np.float64)
        return mock.MagicMock()


class _PolarAx:
    def set_rlabel_position(self, *a):
        pass

    def plot(self, angles, det, **kw):
        _Rec.spider.append(np.array(det, np.float64))

    def fill(self, *a, **kw):
        pass


def _savefig(path, **kw):
    if _Rec.pending is not None:
        stem = os.path.basename(path)
        assert stem.startswith("heat_") and stem.endswith(".png"), stem
        _Rec.maps[stem[5:-4]] = _Rec.pending
        _Rec.pending = None


UA.plt.gca = lambda: _HeatAx()
UA.plt.subplot = lambda *a, **kw: _PolarAx()
UA.plt.savefig = _savefig

H, W = 37, 53
DEFAULT6 = [float(v) for v in np.round(np.arange(0.50, 0.76, 0.05), 2)]
THRS = {2: [0.5, 0.75], 6: DEFAULT6}
# name, N, calibrated columns, K, budget, fix_cd, ranking
CASES = [
    ("n2", 2, True, 6, 0.95, True, False),
    ("n65_nocalib", 65, False, 2, 0.8, False, True),
    ("n1025", 1025, True, 6, 0.95, True, True),
    ("n3000", 3000, True, 6, 0.8, False, True),
]
CLEAN = 14                               # images whose rows are confident and correct: nothing of theirs should be removed


def f32(a):
    """The values the fixture stores: float32-representable, handed to the reference as float64."""
    return np.asarray(a, np.float32).astype(np.float64)


def grid(a, step):
    return np.round(np.asarray(a) / step) * step


def make_case(rng, N, calib):
    tp = rng.random(N) < 0.85
    ious = grid(rng.uniform(0.05, 0.999, N), 1 / 1024)
    ious[0], tp[0] = 0.984375, True          # correct at every threshold
    ious[1], tp[1] = 0.3125, False           # wrong at every threshold
    wrong = ~(tp & (ious >= 0.5))
    entropy = grid(rng.uniform(0, 1.2, N) * np.where(wrong, 1.0, 0.6), 1 / 1024)
    albox = grid(rng.uniform(0.01, 0.3, (N, 4)) * np.where(wrong, 1.5, 1.0)[:, None], 1 / 1024)
    y1, x1 = rng.uniform(-3, H - 2, N), rng.uniform(-3, W - 2, N)
    gt = grid(np.stack([y1, x1, y1 + rng.uniform(0.5, H / 2, N), x1 + rng.uniform(0.5, W / 2, N)], 1), 0.25)
    pred = gt + grid(rng.normal(0, 1.0, (N, 4)), 0.25)
    # negative (from the end), beyond the map, zero-area, inverted, fractional on both sides of an integer, -0.5 (int -> 0)
    special = [((-2.5, -0.5, 30.25, 40.75), (-40.0, -60.0, -1.0, -1.25)),
               ((3.0, 4.0, H + 5.5, W + 20.0), (35.75, 50.5, 1e6, 1e6)),
               ((10.0, 10.0, 10.0, 30.0), (12.0, 7.0, 20.0, 7.0)),
               ((20.0, 30.0, 10.0, 40.0), (5.0, 40.0, 25.0, 12.0)),
               ((9.999999, 10.000001, 19.999999, 20.000001), (10.0, 9.75, 20.25, 20.0)),
               ((0.0, 0.0, float(H), float(W)), (-0.5, -0.75, H - 0.25, W + 0.25))]
    for j, (g, p) in enumerate(special):
        if 2 * j + 1 < N or j == 0:
            gt[(2 * j) % N], pred[(2 * j + 1) % N] = g, p
    ids = names = None
    if N >= 64:
        n_img = N // 6 + CLEAN
        ids = rng.integers(0, n_img, N)
        ids[2:2 + n_img] = np.arange(n_img)
        ids[:2] = n_img - 1
        clean = ids < CLEAN
        entropy[clean], albox[clean] = grid(entropy[clean] / 64, 1 / 1024), grid(albox[clean] / 64, 1 / 65536)
        tp[clean], ious[clean] = True, 0.90625
        perm = rng.permutation(n_img)            # np.unique's order is not the order of first appearance
        names = np.array(["img_%04d.png" % perm[i] for i in ids])
    entropy, albox, gt, pred, ious = f32(entropy), f32(albox), f32(gt), f32(pred), f32(ious)
    out = dict(gt_boxes=gt, pred_boxes=pred, albox=albox, entropy=entropy, ious=ious, tp_class=tp)
    if calib:
        out["calib_albox"], out["calib_entropy"] = f32(grid(albox * 1.25, 1 / 65536)), f32(grid(entropy * 0.75, 1 / 4096))
    out["opt_uncert"] = f32(0.75 * entropy + 0.25 * np.mean(albox, axis=1))
    return out, names


class _Retry(Exception):
    pass


def run_reference(case, names, thrs, fix_cd, budget, ranking, seed, tmp):
    UA.FIX_CD, UA.FPR_TPR, UA.IOU_THRS = bool(fix_cd), float(budget), list(thrs)
    UA.get_dataset_data = lambda path: (None, None, (H, W), None)
    viz = object.__new__(UA.MainUncertViz)
    viz.source_path = tmp
    viz.gt_boxes, viz.pred_boxes = case["gt_boxes"].copy(), case["pred_boxes"].copy()
    viz.albox, viz.entropy = case["albox"].copy(), case["entropy"].copy()
    viz.calib_albox = case["calib_albox"].copy() if "calib_albox" in case else None
    viz.calib_entropy = case["calib_entropy"].copy() if "calib_entropy" in case else None
    viz.opt_uncert, viz.ious, viz.tps_class = case["opt_uncert"].copy(), case["ious"].copy(), case["tp_class"].copy()
    viz.imgs_list = names
    _Rec.reset()
    viz.pred_filters = viz._collect_thresh_results(eval_iou_thr=np.max(thrs))
    viz._plot_metricsspider()
    viz._plot_validheat()
    got = {"map_" + k: v for k, v in _Rec.maps.items()}
    assert len(_Rec.spider) == 3
    got["spider"] = np.stack(_Rec.spider)
    got["collect_thr"] = np.array(viz.pred_filters[3], np.float64)
    got["collect_counts"] = np.array([f.sum() for f in viz.pred_filters[:3]], np.int64)
    if ranking:
        viz._draw_postthresholding = lambda img_name, title: _Rec.drawn.append((str(img_name), title))
        u, thr = viz.opt_uncert, viz.pred_filters[3]
        untouched = [n for n in np.unique(names) if np.all(u[names == n] < thr)]
        if len(untouched) < 12:
            raise _Retry("%d images with nothing removed" % len(untouched))
        random.seed(seed)
        viz._collect_postthresholding()
        tie = False
        for j, label in enumerate(("top_correctremove", "top_falserremove", "top_falseremain", "random_noremoval")):
            got["list_" + label] = np.array([n for n, t in _Rec.drawn if t == label])
            if j < 3:
                cnt = [int(np.sum(names[viz.pred_filters[j]] == n)) for n in got["list_" + label]]
                assert cnt == sorted(cnt, reverse=True)
                tie = tie or len(set(cnt)) < len(cnt)
        if not tie:
            raise _Retry("no equal counts inside a top list")
        assert len(got["list_random_noremoval"]) == 10
    return got


def main():
    warnings.simplefilter("ignore")
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__),
           "cases": np.array([c[0] for c in CASES]), "mask_size": np.array([H, W])}
    with tempfile.TemporaryDirectory() as tmp:
        for index, (name, N, calib, K, budget, fix_cd, ranking) in enumerate(CASES):
            for attempt in range(64):
                rng = np.random.default_rng([20241021, index, attempt])
                case, names = make_case(rng, N, calib)
                seed = 1000 * index + attempt
                try:
                    got = run_reference(case, names, THRS[K], fix_cd, budget, ranking, seed, tmp)
                    break
                except _Retry as e:
                    print("  seed %d of %s: %s" % (attempt, name, e))
            else:
                raise SystemExit("no seed of %s gives a ranking case" % name)
            for key, val in case.items():
                assert val.dtype == bool or np.array_equal(val.astype(np.float32).astype(np.float64), val), key
                out["%s_%s" % (name, key)] = val.astype(np.uint8) if val.dtype == bool else val.astype(np.float32)
            if names is not None:
                out["%s_image_names" % name] = names
            for key, val in (("iou_thrs", np.asarray(THRS[K])), ("fix_cd", np.array(int(fix_cd))), ("budget", np.array(budget)),
                             ("seed", np.array(seed))):
                out["%s_%s" % (name, key)] = val
            for key, val in got.items():
                out["%s_%s" % (name, key)] = val
            print("%-12s N %5d K %d maps %2d thr %.6g removed %s\n%s" % (name, N, K, sum(k.startswith("map_") for k in got),
                                                                          got["collect_thr"], got["collect_counts"], got["spider"]))
    dst = os.path.join(HERE, "thr_post_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) <= os.path.getsize(os.path.join(HERE, "pseudo_golden.npz"))


if __name__ == "__main__":
    main()
