"""Generates tests/golden/thr_golden.npz by running the REAL reference functions `roc_metrics` and the loss closure `_f_x` of
`UncertOptimal._extract_optimal_params` (src/uncertainty_analysis.py:44-152).  The module imports optuna, hebo, matplotlib,
TensorFlow-side helpers and friends at the top; all are stubbed.  `_f_x` is a closure, reached here through a stand-in for optuna
whose trials suggest the fixture's candidates and record the value the reference tells back.  Run once where a checkout of the
reference and sklearn exist; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_thr_golden.py <src directory of the reference's checkout>

Per case the fixture holds the inputs (uncerts [U, N], ious, tp_class, group or nothing, iou_thrs [K], params [P, d], fix_cd,
budget) and what the reference returned: thr / rate / auc [P, K] from `roc_metrics` on the combined score built the way `_f_x`
builds it, and loss [P] from `_f_x` itself.  Asserted below: the loss of `_f_x` equals the mean of rate * 100 (NaN as 1) of those
`roc_metrics` calls, so both paths saw the same scores; every problem outside the deliberately degenerate cases has both labels;
ties are frequent (scores rounded to 1, 2 or 4 decimals, one case with all scores equal, one with zero weights)."""
import os
import sys
import warnings
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_thr_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]


class _Done(Exception):
    pass


class _Trial:
    def __init__(self, row):
        self.row = list(row)

    def suggest_float(self, name, lo, hi):
        return self.row[int(name.split("_")[1]) - 1]


class _Study:
    """ask() hands out the queued candidates in order; tell() records the loss the reference computed for each."""
    queue, values = [], []

    def ask(self):
        if not _Study.queue:
            raise _Done()
        return _Trial(_Study.queue.pop(0))

    def tell(self, trial, value):
        _Study.values.append(float(value))


for name in ("optuna", "dataset_data", "hebo", "hebo.design_space", "hebo.design_space.design_space", "hebo.optimizers",
             "hebo.optimizers.hebo", "hparams_config", "matplotlib", "matplotlib.pyplot", "matplotlib.patches", "mpl_toolkits",
             "mpl_toolkits.axes_grid1", "PIL", "utils_box", "utils_extra", "utils_infer", "tensorflow"):
    sys.modules[name] = mock.MagicMock()
sys.modules["optuna"].create_study = lambda direction=None: _Study()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
import numpy as np                       # noqa: E402
import sklearn                           # noqa: E402
import uncertainty_analysis as UA        # noqa: E402  (the reference module)

DEFAULT6 = [float(v) for v in np.round(np.arange(0.50, 0.76, 0.05), 2)]
THRS = {1: [0.5], 6: DEFAULT6, 32: [float(v) for v in np.linspace(0.05, 0.95, 32)]}
# name, N, U, K, budget, fix_cd, G, P, decimals, kind
CASES = [
    ("n2", 2, 1, 1, 0.95, True, 0, 1, 1, ""),
    ("n3", 3, 2, 6, 0.95, False, 0, 3, 1, ""),
    ("n5", 5, 3, 6, 0.8, True, 0, 3, 2, ""),
    ("n17", 17, 2, 32, 0.8, False, 0, 3, 1, ""),
    ("n64g3", 64, 2, 6, 0.95, True, 3, 3, 2, ""),
    ("n65g10", 65, 3, 6, 0.95, False, 10, 3, 2, ""),
    ("n257p64", 257, 2, 6, 0.95, True, 0, 64, 2, ""),
    ("n257k32", 257, 1, 32, 0.8, False, 0, 3, 1, ""),
    ("n1025", 1025, 2, 6, 0.95, True, 0, 3, 4, ""),
    ("n1025g3", 1025, 3, 6, 0.8, False, 3, 3, 2, ""),
    ("n4099", 4099, 2, 6, 0.95, True, 0, 3, 4, ""),
    ("n4099k32", 4099, 2, 32, 0.95, False, 0, 1, 2, ""),
    ("allequal", 64, 2, 6, 0.95, True, 0, 1, 2, "allequal"),
    ("zeroweight", 257, 2, 6, 0.8, False, 0, 3, 2, "zeroweight"),
    ("allcorrect", 17, 2, 1, 0.95, True, 0, 1, 2, "allcorrect"),
    ("allwrong", 17, 2, 6, 0.95, False, 0, 3, 2, "allwrong"),
]


def make_case(rng, N, U, K, G, P, dec, kind):
    thrs = THRS[K]
    tp = rng.random(N) < 0.85
    ious = np.round(rng.uniform(0.05, 0.999, N), 3)
    ious[0], tp[0] = 0.99, True             # correct at every threshold
    ious[1], tp[1] = 0.7, False             # wrong at every threshold
    wrong = ~(tp & (ious >= 0.5))
    ent = np.round(rng.uniform(0, 1.2, N) * np.where(wrong, 1.0, 0.6), dec)      # failures are somewhat more uncertain
    cols = [ent] + [np.round(rng.gamma(2.0, 0.05, N) * np.where(wrong, 1.5, 1.0), dec) for _ in range(U - 1)]
    uncerts = np.stack(cols[:U])
    group = None
    if G:
        present = [g for g in range(G) if g != G // 2]          # the middle class has no row; the last one has
        group = rng.choice(present, N).astype(np.int32)
        group[:len(present)] = present[:N]
        assert G // 2 not in group and group.max() == G - 1
    d = U * max(G, 1)
    params = rng.uniform(0, 1, (P, d))
    params[0] = np.round(params[0], 1)       # round weights: sums of different rows collide
    if G and P > 1:
        params[1] = np.tile(np.round(params[1, :U], 1), G)      # every class the same round weights
    if kind == "allequal":
        uncerts[:] = uncerts[:, :1]
    if kind == "zeroweight":
        params[0], params[1], params[2] = (0.0, 0.5), (0.5, 0.0), (0.0, 0.0)
    if kind == "allcorrect":
        ious[:], tp[:] = 0.99, True
    if kind == "allwrong":
        tp[:] = False
    return uncerts, ious, tp, group, np.asarray(thrs, np.float64), params


def combined_like_f_x(uncerts, row, group, G):
    """The score the way `_f_x` builds it (uncertainty_analysis.py:134-147)."""
    if group is None:
        return sum(param * uncert for param, uncert in zip(row, list(uncerts)))
    collected = [u.copy() for u in uncerts]
    it = 0
    for i in range(G):
        for j in range(len(collected)):
            collected[j][group + 1 == i + 1] *= row[it]
            it += 1
    return np.sum(collected, axis=0)


def run_reference(uncerts, ious, tp, group, thrs, params, fix_cd, budget):
    UA.FIX_CD, UA.FPR_TPR, UA.IOU_THRS = bool(fix_cd), float(budget), list(thrs)
    G = 0 if group is None else int(group.max()) + 1
    P, K = len(params), len(thrs)
    out = np.zeros((3, P, K))
    for p, row in enumerate(params):
        u = combined_like_f_x(uncerts, row, group, G)
        for k, t in enumerate(thrs):
            out[:, p, k] = UA.roc_metrics(u, np.asarray((ious >= t) * tp, dtype=int))
    opt = UA.UncertOptimal(None if group is None else (group + 1).astype(np.float64), tp, ious, [u.copy() for u in uncerts],
                           per_cls=group is not None, source_path=os.devnull)
    _Study.queue, _Study.values = [list(r) for r in params], []
    try:
        opt._extract_optimal_params()
    except _Done:
        pass
    loss = np.asarray(_Study.values)
    assert loss.shape == (P,)
    rate = np.where(np.isnan(out[1]), 1.0, out[1])
    assert np.array_equal(loss, np.mean(rate * 100, axis=1)), "the recipe's scores differ from _f_x's"
    return out, loss


def main():
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(20241018)
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__),
           "cases": np.array([c[0] for c in CASES])}
    for name, N, U, K, budget, fix_cd, G, P, dec, kind in CASES:
        uncerts, ious, tp, group, thrs, params = make_case(rng, N, U, K, G, P, dec, kind)
        got, loss = run_reference(uncerts, ious, tp, group, thrs, params, fix_cd, budget)
        degenerate = kind in ("allcorrect", "allwrong")
        for t in thrs:
            lab = (ious >= t) & tp
            assert degenerate == (lab.all() or not lab.any()), (name, t)
        assert np.isnan(got[1]).all() == degenerate and np.isnan(got[1]).any() == degenerate, name
        if degenerate:
            assert np.isposinf(got[0]).all() and np.isnan(got[2]).all(), name
        ties = max(N - len(np.unique(combined_like_f_x(uncerts, row, group, G))) for row in params)
        assert kind or N < 17 or ties > 0, name
        for key, val in (("uncerts", uncerts), ("ious", ious), ("tp_class", tp.astype(np.uint8)), ("iou_thrs", thrs),
                         ("params", params), ("fix_cd", np.array(int(fix_cd))), ("budget", np.array(budget)), ("G", np.array(G)),
                         ("thr", got[0]), ("rate", got[1]), ("auc", got[2]), ("loss", loss)):
            out["%s_%s" % (name, key)] = val
        if group is not None:
            out["%s_group" % name] = group
        print("%-11s N %5d U %d K %2d P %2d G %2d  tied rows %4d  loss[0] %.6g" % (name, N, U, K, P, G, ties, loss[0]))
    dst = os.path.join(HERE, "thr_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 1000000


if __name__ == "__main__":
    main()
