"""Generates tests/golden/epal_golden.npz by running the REAL reference method `EpistemicVSAleatoric.compare_epal`
(src/uncertainty_ep_vs_al.py:456-545, with `get_plot_grid`, `_get_cell_indices`, `get_metrics_comp`, `save_highlow` under it) on
synthetic validate_results.txt files that this maker writes with `writers.validate_records` / `write_validate_results`.  Run once
where a checkout of the reference and scipy exist; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_epal_golden.py <src directory of the reference's checkout>

Stubbed, in this maker only: tensorflow, tensorflow_probability, seaborn, matplotlib and PIL (MagicMock; `plt.subplots` returns a
pair), the `brisque` package (a BRISQUE whose score is 0.0), `PARENT_DIR` (a temporary directory) and `get_dataset_data` (the
case's class names), and `_save_crops` (nothing).  `scipy.stats.gaussian_kde` is wrapped so that the evaluated values are captured;
`plot_unc_metrics`, `get_plot_grid`, `_get_cell_indices` and `save_highlow` are wrapped so that what they are handed and what they
return is captured - the lists, the cell indices, the grid's steps and the two index lists are the run's own, nothing is restated
here - and are then run as they are.

Cases (`cases`; the runs of a case are `<case>_runs`, each "<uncert>|<ent>|<im_numbs>"):
  main    400 rows, 3 classes, a tenth of them displaced to an IoU of 0.1 or less: uncalib, uncalib with the entropy, iso_all
  deep     90 rows with a cluster in either corner: the search grows past g = 4
  empty    60 rows on the diagonal and one in the high-AL corner: both corners hold fewer than 3 at g = 2, one list has one row
Stored per case: the columns `kde_ref.golden_records` rebuilds the records from (boxes in quarter pixels, everything else on a
1/1024 grid, all float32; the iso_all columns are derived there), `<case>_text_sha` - the sha256 of the validate_results.txt the reference read.  Per run `<case>_r<k>_`:
grid_size, cell_indices, hal_lep_ind, lal_hep_ind, n_metrics, labels, m<j>_<col> (the lists handed to plot_unc_metrics; col 6 is
the stubbed BRISQUE and is not stored), kde (the captured values at every `kde_stride`-th of the 10 000 mesh positions),
hal_lep_txt / lal_hep_txt (the two files), subdir."""
import hashlib
import os
import sys
import tempfile
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_epal_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
for name in ("tensorflow", "tensorflow_probability", "seaborn", "matplotlib", "matplotlib.pyplot", "PIL", "brisque", "dataset_data"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np                       # noqa: E402
import scipy.stats                       # noqa: E402
import uncertainty_ep_vs_al as EP        # noqa: E402  (the reference module)
import kde_ref as R                      # noqa: E402
from uda_amd import writers              # noqa: E402

CLASS_NAMES = ["car", "pedestrian", "cyclist"]
KDE_STRIDE = 29
KDE_IDX = np.arange(0, 10000, KDE_STRIDE)


class _Rec:
    kde, lists, grid, cells, ind = [], [], None, None, None


class CapturingKde(scipy.stats.gaussian_kde):
    def evaluate(self, points):
        out = super().evaluate(points)
        _Rec.kde.append(np.array(out, np.float64))
        return out

    __call__ = evaluate


class ZeroBrisque:
    def __init__(self, url=False):
        pass

    def score(self, img):
        return 0.0


_PLOT = EP.EpistemicVSAleatoric.plot_unc_metrics


def _plot_unc_metrics(self, data_list, labels, colors):
    _Rec.lists.append(([list(d) for d in data_list], list(labels), list(colors)))
    return _PLOT(self, data_list, labels, colors)


_GRID = EP.EpistemicVSAleatoric.get_plot_grid
_SAVE = EP.EpistemicVSAleatoric.save_highlow
_CELLS = EP.EpistemicVSAleatoric._get_cell_indices


def _get_plot_grid(self, av_al, av_mc):
    _Rec.grid = np.array(_GRID(self, av_al, av_mc))
    return _Rec.grid


def _save_highlow(self, detections, gt_bbox, bbox, hal_lep_ind, lal_hep_ind):
    _Rec.ind = (np.array(hal_lep_ind), np.array(lal_hep_ind))
    return _SAVE(self, detections, gt_bbox, bbox, hal_lep_ind, lal_hep_ind)


def _get_cell_indices(grid_size, uncert_data):
    _Rec.cells = _CELLS(grid_size, uncert_data)              # the last call of a run is the one at the grid size it settles on
    return _Rec.cells


EP.EpistemicVSAleatoric.get_plot_grid = _get_plot_grid
EP.EpistemicVSAleatoric.save_highlow = _save_highlow
EP.EpistemicVSAleatoric._get_cell_indices = staticmethod(_get_cell_indices)
EP.plt.subplots = lambda *a, **kw: (mock.MagicMock(), mock.MagicMock())
EP.BRISQUE = ZeroBrisque
EP.get_dataset_data = lambda model_name: (None, "images/", CLASS_NAMES, None)
EP.EpistemicVSAleatoric._save_crops = lambda self, *a: None
EP.EpistemicVSAleatoric.plot_unc_metrics = _plot_unc_metrics


def q(a, step):
    """onto a grid of `step`, as float32 (exact for the ranges used here)."""
    return (np.round(np.asarray(a, np.float64) / step) * step).astype(np.float32)


def make_case(case, n, seed):
    rng = np.random.default_rng(seed)
    y1, x1 = rng.uniform(0, 300, n), rng.uniform(0, 600, n)
    h, w = rng.uniform(24, 200, n), rng.uniform(24, 260, n)
    boxes = q(np.stack([y1, x1, y1 + h, x1 + w], 1), 0.25)
    gt = boxes + q(rng.normal(0, 3, (n, 4)), 0.25)
    if case == "main":
        far = rng.choice(n, n // 10, replace=False)
        gt[far[::2]] += q(np.stack([h, w, h, w], 1)[far[::2]] * 0.8, 0.25)       # a sliver of overlap
        gt[far[1::2]] += 1000.0                                                  # none
        al = rng.lognormal(-3.0, 0.6, n)
        mc = 0.4 * al + rng.lognormal(-3.6, 0.7, n)
    elif case == "deep":
        t = rng.uniform(0, 1, n)
        al = np.where(np.arange(n) % 3 == 0, 0.10 - 0.005 * t, np.where(np.arange(n) % 3 == 1, 0.005 * t + 0.001, 0.02 + 0.06 * t))
        mc = np.where(np.arange(n) % 3 == 0, 0.004 * rng.uniform(0, 1, n) + 0.001, np.where(np.arange(n) % 3 == 1, 0.08 - 0.004 * rng.uniform(0, 1, n),
                                                                                         0.02 + 0.04 * rng.uniform(0, 1, n)))
    else:
        t = np.concatenate([np.linspace(0.01, 0.04, n // 2), np.linspace(0.06, 0.09, n - n // 2)])   # nothing near the cut at g = 2
        al, mc = t.copy(), t * 0.8 + 0.001
        al[17], mc[17] = 0.088, 0.0105
    hw = (boxes[:, [2, 3, 2, 3]] - boxes[:, [0, 1, 0, 1]]).astype(np.float64)
    albox = q(al[:, None] * hw * rng.uniform(0.9, 1.1, (n, 4)), 1 / 1024)
    mcbox = q(mc[:, None] * hw * rng.uniform(0.9, 1.1, (n, 4)), 1 / 1024)
    logits = q(rng.normal(0, 2, (n, 3)), 1 / 1024)
    e = np.exp(logits - logits.max(1, keepdims=True))
    probab = q(e / e.sum(1, keepdims=True), 1 / 1024)
    entropy = q(-(probab * np.log(np.maximum(probab, 1e-6))).sum(1), 1 / 1024)
    classes = logits.argmax(1) + 1
    gt_classes = np.where(rng.uniform(0, 1, n) < 0.85, classes, rng.integers(1, 4, n))
    return dict(names=np.array(["%06d.png" % (i // 3) for i in range(n)]), scores=q(rng.uniform(0.3, 1.0, n), 1 / 1024), boxes=boxes,
                gt_boxes=gt.astype(np.float32), classes=classes.astype(np.int32), gt_classes=gt_classes.astype(np.int32), logits=logits,
                probab=probab, entropy=entropy, mcbox=mcbox, albox=albox)


CASES = [("main", 400, 31, [("uncalib", False, 4), ("uncalib", True, 4), ("iso_all", False, 3)]),
         ("deep", 90, 32, [("uncalib", False, 10)]),
         ("empty", 60, 33, [("uncalib", False, 10)])]


def main():
    out = {"numpy_version": np.array([np.__version__]), "scipy_version": np.array([scipy.__version__]), "class_names": np.array(CLASS_NAMES),
           "cases": np.array([c[0] for c in CASES]), "kde_stride": np.array(KDE_STRIDE)}
    for case, n, seed, runs in CASES:
        cols = make_case(case, n, seed)
        for k, v in cols.items():
            out["%s_%s" % (case, k)] = v
        out[case + "_runs"] = np.array(["%s|%d|%d" % r for r in runs])
        records = R.golden_records(cols)
        for k, (uncert, ent, numb) in enumerate(runs):
            with tempfile.TemporaryDirectory() as tmp, mock.patch.object(scipy.stats, "gaussian_kde", CapturingKde):
                os.makedirs(tmp + "/results/validation/m")
                writers.write_validate_results(tmp + "/results/validation/m/validate_results.txt", records)
                text = open(tmp + "/results/validation/m/validate_results.txt", "rb").read()
                out[case + "_text_sha"] = np.array([hashlib.sha256(text).hexdigest()])
                EP.PARENT_DIR = tmp
                _Rec.kde, _Rec.lists = [], []
                obj = EP.EpistemicVSAleatoric("m", im_numbs=numb, iou_thr=0.1, uncert=uncert, ent=ent)
                with np.errstate(all="ignore"):
                    obj.compare_epal()
                assert len(_Rec.kde) == 1 and len(_Rec.lists) == 1 and _Rec.kde[0].shape == (10000,)
                sub = "compare_epal/entropy" if ent else "compare_epal/mcdropout"
                assert os.path.normpath(obj.source_path) == os.path.normpath(tmp + "/results/validation/m/" + sub)
                pre = "%s_r%d_" % (case, k)
                # captured from the run itself: the last _get_cell_indices call of get_plot_grid, its return value, and the index
                # lists compare_epal hands to save_highlow
                cells, g = _Rec.cells, obj.grid_size
                assert np.array_equal(cells[0], _Rec.grid) and len(_Rec.ind) == 2
                out[pre + "grid_size"] = np.array(g)
                out[pre + "cell_indices"] = np.asarray(_Rec.grid).astype(np.int32)
                out[pre + "cell_steps"] = np.array(cells[1:], np.float64)
                out[pre + "hal_lep_ind"], out[pre + "lal_hep_ind"] = _Rec.ind
                kept = len(_Rec.grid)
                lists, labels, _ = _Rec.lists[0]
                out[pre + "n_metrics"] = np.array(len(lists))
                out[pre + "labels"] = np.array(labels if labels else [""])
                for j, data in enumerate(lists):
                    assert len(data) == 9
                    for col in (0, 1, 2, 3, 4, 5, 7, 8):
                        out["%sm%d_%d" % (pre, j, col)] = np.asarray(data[col])
                out[pre + "kde"] = _Rec.kde[0][KDE_IDX]
                for stem in ("hal_lep", "lal_hep"):
                    out[pre + stem + "_txt"] = np.array([open("%s/%s_%s_iou_0.1.txt" % (obj.source_path, stem, uncert)).read()])
                out[pre + "subdir"] = np.array([sub])
                print(case, uncert, ent, "kept", kept, "grid", g, "corners", len(out[pre + "hal_lep_ind"]), len(out[pre + "lal_hep_ind"]))
        if case == "deep":
            assert int(out["deep_r0_grid_size"]) > 4
        if case == "empty":
            assert int(out["empty_r0_grid_size"]) == 2 and len(out["empty_r0_hal_lep_ind"]) == 1 and len(out["empty_r0_lal_hep_ind"]) == 0
    path = os.path.join(HERE, "epal_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
