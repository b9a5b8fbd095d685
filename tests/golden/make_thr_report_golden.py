"""Generates tests/golden/thr_report_golden.npz by running the REAL reference functions `calc_jsd` (src/utils_extra.py:25-36),
`roc_metrics`, `MainUncertViz._save_thr_performance` and `MainUncertViz._collect_thresh_results`
(src/uncertainty_analysis.py:44-83, :517-749).  Both modules import optuna, hebo, matplotlib, TensorFlow and friends at the top;
all are stubbed (the stubs of make_thr_golden.py, and utils_extra is the real one here); sklearn and scipy are real.  The methods
run on `object.__new__(MainUncertViz)` with the members set by hand, the module's FPR_TPR / FIX_CD / IOU_THRS set per case, and a
stand-in for `plt.subplots` whose axis records the `cellText` of the table.  Run once where a checkout of the reference, sklearn
and scipy exist; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_thr_report_golden.py <src directory of the reference's checkout>

Per case the fixture holds the inputs (uncerts [U, N], opt_uncert, ious, tp_class, gt_classes, iou_thrs, opt_params or nothing,
fix_cd, budget), the bytes of thr_metrics_*.txt, `table_data` as strings, `fprs_opt`, and per (segment, column, threshold) what
`calc_jsd` / `roc_metrics` / `np.mean` / `np.std` returned on the slices the reference takes: segments = all rows, then classes
1..C; columns = the U uncertainties, opt_uncert, and with opt_params the reference's per-class combination (:576-595, its running
index advancing only for classes with rows).  A segment without rows holds NaN (+inf for thr): the reference never evaluates it.
`_collect_thresh_results` at the largest IoU threshold gives opt_thr and the sums of its three masks.

Asserted below: no value the reference prints lies within 1e-9 of a `:.3f` or `round(..., 2)` boundary (else: another seed), so the
texts can be compared byte for byte although sums are ordered differently elsewhere."""
import os
import sys
import tempfile
import warnings
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_thr_report_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]

for name in ("optuna", "dataset_data", "hebo", "hebo.design_space", "hebo.design_space.design_space", "hebo.optimizers",
             "hebo.optimizers.hebo", "hparams_config", "matplotlib", "matplotlib.pyplot", "matplotlib.patches", "mpl_toolkits",
             "mpl_toolkits.axes_grid1", "PIL", "utils_box", "utils_infer", "tensorflow", "uncertainty_toolbox",
             "uncertainty_toolbox.viz", "absl"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
import numpy as np                       # noqa: E402
import scipy                             # noqa: E402
import scipy.spatial.distance            # noqa: E402,F401  (utils_extra reaches both through `import scipy`)
import scipy.stats                       # noqa: E402,F401
import sklearn                           # noqa: E402
import uncertainty_analysis as UA        # noqa: E402  (the reference module)
import utils_extra                       # noqa: E402  (the reference module, the real one)

assert UA.calc_jsd is utils_extra.calc_jsd


class _Ax:
    recorded = None

    def table(self, cellText=None, **kw):
        _Ax.recorded = [list(r) for r in cellText]
        return mock.MagicMock()

    def axis(self, *a):
        pass


UA.plt.subplots = lambda **kw: (mock.MagicMock(), _Ax())

DEFAULT6 = [float(v) for v in np.round(np.arange(0.50, 0.76, 0.05), 2)]
THRS = {1: [0.5], 2: [0.5, 0.75], 6: DEFAULT6}
# name, N, U, K, budget, fix_cd, C, opt ("global" | "percls" | ""), decimals, kind
CASES = [
    ("n2_txt", 2, 1, 6, 0.95, True, 0, "", 1, ""),
    ("n3_k1_txt", 3, 2, 1, 0.8, False, 0, "", 1, ""),
    ("n65_u1_global", 65, 1, 2, 0.8, False, 3, "global", 1, ""),
    ("n257_u3_percls", 257, 3, 2, 0.95, True, 6, "percls", 2, "special"),
    ("n1025_ties", 1025, 2, 6, 0.8, True, 3, "global", 1, ""),
    ("n3000_cd_global", 3000, 2, 6, 0.95, True, 5, "global", 4, "bigclass"),
    ("n3000_fd_percls", 3000, 2, 6, 0.8, False, 5, "percls", 3, "bigclass"),
    ("n3000_u3_txt", 3000, 3, 6, 0.95, False, 0, "", 4, ""),
]


def make_case(rng, N, U, K, C, opt, dec, kind):
    thrs = THRS[K]
    tp = rng.random(N) < 0.85
    ious = np.round(rng.uniform(0.05, 0.999, N), 3)
    ious[0], tp[0] = 0.99, True             # correct at every threshold
    ious[1], tp[1] = 0.3, False             # wrong at every threshold
    wrong = ~(tp & (ious >= 0.5))
    ent = np.round(rng.uniform(0, 1.2, N) * np.where(wrong, 1.0, 0.6), dec)      # failures are somewhat more uncertain
    cols = [ent] + [np.round(rng.gamma(2.0, 0.05, N) * np.where(wrong, 1.5, 1.0), dec) for _ in range(U - 1)]
    uncerts = np.stack(cols[:U])
    gt = None
    if C:
        empty = C // 2 + 1                                       # a class in the middle has no row; the last one has
        present = [c for c in range(1, C + 1) if c != empty]
        p = np.ones(len(present))
        if kind == "bigclass":
            p[0] = 3.0 * len(present)                            # class 1 alone straddles the 2048-row tile
        gt = rng.choice(present, N, p=p / p.sum()).astype(np.float64)
        gt[:len(present)] = present
        if kind == "special":                                    # classes 1..6, class 4 empty
            gt[gt == 2] = 1
            gt[gt == 3] = 1
            gt[gt == 5] = 1
            gt[10] = 2                                           # class 2: one row
            gt[20], gt[21] = 3, 3                                # class 3: two rows with equal scores, one correct and one wrong
            uncerts[:, 21] = uncerts[:, 20]
            ious[20], tp[20], ious[21], tp[21] = 0.99, True, 0.99, False
            five = np.flatnonzero(gt == 1)[30:50]                # class 5: twenty rows, all correct - one label only
            gt[five] = 5
            ious[five], tp[five] = 0.99, True
            assert set(np.unique(gt)) == {1, 2, 3, 5, 6}
        else:
            assert empty not in gt and gt.max() == C
    weights = np.round(rng.uniform(0.1, 1.0, U), 2)
    opt_params = None
    if opt == "global":
        opt_params = [float(w) for w in weights]
    elif opt == "percls":
        opt_params = [float(w) for w in np.round(rng.uniform(0.05, 1.0, U * C), 2)]
    if opt == "percls":                                          # opt_uncert the way __init__ builds it (:435-444)
        collected = [u.copy() for u in uncerts]
        it = 0
        for i in range(C):
            for j in range(U):
                collected[j][gt == i + 1] *= opt_params[it]
                it += 1
        opt_uncert = np.sum(collected, axis=0)
    else:
        opt_uncert = sum(w * u for w, u in zip(weights, uncerts))
    return uncerts, opt_uncert, ious, tp, gt, thrs, opt_params


def class_column(uncerts, gt, opt_params, C):
    """The per-class combination of _save_thr_performance (:576-595), all classes in one column (their rows are disjoint)."""
    col = np.zeros(uncerts.shape[1])
    n_iter = 0
    for i in range(C):
        sel = np.where(gt == i + 1)[0]
        if len(sel) > 0:
            per = [u[sel] for u in uncerts]
            if len(opt_params) == len(per):
                col[sel] = sum(p * u for p, u in zip(opt_params, per))
            else:
                for j in range(len(per)):
                    per[j] *= opt_params[n_iter]
                    n_iter += 1
                col[sel] = np.sum(per, axis=0)
    return col


class _Boundary(Exception):
    """A printed value lies within 1e-9 of a rounding boundary: the case is drawn again with its next seed."""


def need(ok, what):
    if not ok:
        raise _Boundary(what)


def off_boundary(v, decimals):
    x = abs(float(v)) * 10 ** decimals
    return abs(x - np.floor(x) - 0.5) > 1e-9 * 10 ** decimals


def run_reference(name, uncerts, opt_uncert, ious, tp, gt, thrs, opt_params, fix_cd, budget, tmp):
    UA.FIX_CD, UA.FPR_TPR, UA.IOU_THRS = bool(fix_cd), float(budget), list(thrs)
    U, N = uncerts.shape
    K, C = len(thrs), 0 if gt is None else int(max(gt))
    viz = object.__new__(UA.MainUncertViz)
    viz.source_path = tmp
    viz.selected_uncerts = [u.copy() for u in uncerts]
    viz.opt_uncert = opt_uncert.copy()
    viz.tps_class, viz.ious = tp.copy(), ious.copy()
    viz.gt_classes = gt
    viz.label_map = {i + 1: "class%d" % (i + 1) for i in range(C)}
    _Ax.recorded = None
    added = "_" + name
    fprs_opt = viz._save_thr_performance(added_name=added, opt_params=opt_params)
    path = tmp + "/thr_metrics_" + ("cd" if fix_cd else "fd") + "_" + str(float(budget)) + "_iou_" + str(np.min(thrs)) + "_" + \
        str(np.max(thrs)) + added + ".txt"
    with open(path, "rb") as f:
        txt = f.read()
    table = None
    if opt_params is not None:
        table = np.array([[str(x) for x in row] for row in _Ax.recorded])
    else:
        assert _Ax.recorded is None

    cols = [u for u in uncerts] + [opt_uncert]
    if opt_params is not None:
        cols.append(class_column(uncerts, gt, opt_params, C))
    segs = [np.arange(N)] + [np.where(gt == i + 1)[0] for i in range(C)]
    B, S = len(segs), len(cols)
    roc = np.full((B, S, K, 3), np.nan)
    roc[..., 0] = np.inf
    jsd = np.full((B, S, K), np.nan)
    mean, std = np.full((B, S, K, 2), np.nan), np.full((B, S, K, 2), np.nan)
    n_label = np.zeros((B, K, 2), np.int64)
    for b, sel in enumerate(segs):
        for k, t in enumerate(thrs):
            correct = np.asarray((ious[sel] >= t) * tp[sel])
            n_label[b, k] = correct.sum(), (~correct).sum()
            if len(sel) == 0:
                continue
            for s, col in enumerate(cols):
                u = col[sel]
                jsd[b, s, k] = UA.calc_jsd(u[correct], u[~correct])
                roc[b, s, k] = UA.roc_metrics(u, correct)
                for j, sub in enumerate((u[correct], u[~correct])):
                    if len(sub):
                        mean[b, s, k, j], std[b, s, k, j] = np.mean(sub), np.std(sub)
    # what the reference prints, away from every rounding boundary
    j100, a100 = np.nan_to_num(jsd), np.nan_to_num(roc[..., 2]) * 100
    f100 = np.where(np.isnan(roc[..., 1]), 0.0, (1 - roc[..., 1]) * 100)
    for v in (j100, a100, f100):
        for s in range(U + 1):
            need(off_boundary(np.mean(v[0, s]), 3), (name, "txt", s))
            if opt_params is not None:
                need(all(off_boundary(x, 2) for x in v[0, s]) and off_boundary(np.mean(v[0, s]), 2), (name, "table", s))
        if opt_params is not None:
            for b in range(1, B):
                if len(segs[b]):
                    need(all(off_boundary(x, 2) for x in v[b, U + 1]) and off_boundary(np.mean(v[b, U + 1]), 2), (name, b))
    assert fprs_opt == np.mean(f100[0, U]), name

    removed = viz._collect_thresh_results(eval_iou_thr=np.max(thrs))
    assert removed[3] == roc[0, U, K - 1, 0] or (np.isinf(removed[3]) and np.isinf(roc[0, U, K - 1, 0])), name
    collect = np.array([removed[0].sum(), removed[1].sum(), removed[2].sum()], np.int64)
    return dict(txt=np.frombuffer(txt, np.uint8), table=table, fprs_opt=np.array(fprs_opt), roc=roc, jsd=jsd, mean=mean, std=std,
                n_label=n_label, collect_counts=collect, collect_thr=np.array(removed[3]))


def main():
    warnings.simplefilter("ignore")
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__),
           "scipy_version": np.array(scipy.__version__), "cases": np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        for index, (name, N, U, K, budget, fix_cd, C, opt, dec, kind) in enumerate(CASES):
            for attempt in range(64):           # the case's seeds in turn, until nothing printed sits on a rounding boundary
                rng = np.random.default_rng([20241020, index, attempt])
                uncerts, opt_uncert, ious, tp, gt, thrs, opt_params = make_case(rng, N, U, K, C, opt, dec, kind)
                try:
                    got = run_reference(name, uncerts, opt_uncert, ious, tp, gt, thrs, opt_params, fix_cd, budget, tmp)
                    break
                except _Boundary as e:
                    print("  seed %d of %s: on a boundary %s" % (attempt, name, e))
            else:
                raise SystemExit("no seed of %s keeps clear of the rounding boundaries" % name)
            for key, val in (("uncerts", uncerts), ("opt_uncert", opt_uncert), ("ious", ious), ("tp_class", tp.astype(np.uint8)),
                             ("iou_thrs", np.asarray(thrs)), ("fix_cd", np.array(int(fix_cd))), ("budget", np.array(budget))):
                out["%s_%s" % (name, key)] = val
            if gt is not None:
                out["%s_gt_classes" % name] = gt
            if opt_params is not None:
                out["%s_opt_params" % name] = np.asarray(opt_params)
            for key, val in got.items():
                if val is not None:
                    out["%s_%s" % (name, key)] = val
            ties = N - len(np.unique(opt_uncert))
            print("%-16s N %5d U %d K %d C %d %-7s tied rows %4d  fprs_opt %.6f  nan jsd %d" %
                  (name, N, U, K, C, opt, ties, got["fprs_opt"], int(np.isnan(got["jsd"]).sum())))
            print(bytes(got["txt"]).decode(), end="")
    dst = os.path.join(HERE, "thr_report_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 1000000


if __name__ == "__main__":
    main()
