"""Generates tests/golden/uncert_report_golden.npz by running the REAL reference functions `calc_ece`, `calc_nll`, `calc_rmse`,
`calc_iou_np` (src/utils_box.py:17-102), `RegressionCalib._relative_calc_ece` and `_conf_all` (src/calibrate_regression.py:46-61,
231-349) and `ValidUncertPlot.__init__` (src/utils_extra.py:378-445) on float64 arrays made here.  Run once where a checkout of
the reference exists; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_uncert_report_golden.py <src directory of the reference's checkout>

How the functions are reached: tensorflow and friends, uncertainty_toolbox, sklearn, matplotlib and absl are stubbed; the three
`tf` calls of calc_rmse (tf.math.sqrt, tf.reduce_mean, tf.math.square) are numpy's.  `ValidUncertPlot.collect_uvi` (plots) is
replaced by a no-op and the class is constructed on a temporary folder, aleatoric first and mcdropout second as
Validate.launch_val does, so that model_performance.txt holds what the reference writes; `_conf_all` runs on an object made with
`__new__` and writes regression_logging.txt there.  All inputs are float64, so numpy's scalar promotion plays no part.

Cases: n1, n5 and n300 rows, two sigma columns each.  n5 is planted: row 0 has sigma = 0 in column 0, row 1 a residual of 0,
row 2 both, row 3 a ground-truth coordinate equal to 0, row 4 a prediction that does not touch its ground truth (IoU 0).  n300
has classes 1 and 3 of three (class 2 is empty), rows with residual 0, with a ground-truth coordinate of 0 and with IoU 0, and
sigmas in [0.5, 8] (pixels).  Recorded per case: the inputs; ious, % missing, misclassification, mIoU, RMSE; per column calc_ece
flattened, of the [N, 4] arrays and per coordinate, the rows inside +-sigma (the loop of _conf_all:258-265, restated here for the
unrounded count and checked against the rounded text), calc_nll over the elements whose sigma is neither 0 nor non-finite (and,
as `nll_raw`, over all elements: what nan_to_num makes of sigma = 0), RMSUE, sharpness, `_relative_calc_ece` of the relativised arrays and of
their first coordinate; for n300 the same per class; the texts of both files (regression_logging.txt not for n5, whose NLL is that
artefact); z = norm.ppf((1 - p_m) / 2) for the 100 levels; numpy's version.  What is planted is asserted in main()."""
import os
import sys
import tempfile
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_uncert_report_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
import numpy as np                       # noqa: E402

for name in ("tensorflow", "tensorflow.python", "tensorflow.python.training", "tensorflow_probability", "uncertainty_toolbox",
             "uncertainty_toolbox.viz", "sklearn", "sklearn.metrics", "sklearn.isotonic", "matplotlib", "absl"):
    sys.modules[name] = mock.MagicMock()
tf = sys.modules["tensorflow"]
tf.math.sqrt, tf.math.square, tf.reduce_mean = np.sqrt, np.square, np.mean
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
from scipy import stats                  # noqa: E402
import utils_box as UB                   # noqa: E402  (the reference modules)
import utils_extra as UE                 # noqa: E402
import calibrate_regression as CR        # noqa: E402

UE.ValidUncertPlot.collect_uvi = lambda self: None
DECODING = "l-norm"
METHOD = "TS All"


def make_case(n, seed, planted):
    rng = np.random.default_rng(seed)
    y1, x1 = rng.uniform(5, 300, n), rng.uniform(5, 300, n)
    h, w = rng.uniform(40, 200, n), rng.uniform(40, 200, n)    # (no noise turns a box inside out)
    gt = np.stack([y1, x1, y1 + h, x1 + w], 1)
    pred = gt + rng.normal(0, 3, (n, 4))
    sig = np.stack([rng.uniform(0.5, 8, (n, 4)), rng.uniform(0.5, 6, (n, 4))])
    gc = rng.choice([1.0, 3.0], n)
    pc = np.where(rng.uniform(size=n) < 0.2, 4.0 - gc, gc)
    if planted == "n5":
        sig[0, 0] = 0.0
        pred[1] = gt[1]
        sig[0, 2] = 0.0
        pred[2] = gt[2]
        gt[3, 0] = 0.0
        pred[4] = gt[4] + 1000.0
    elif planted == "n300":
        pred[7] = gt[7]
        pred[100, 2] = gt[100, 2]
        gt[20, 1] = 0.0
        gt[21, 0] = 0.0
        pred[50] = gt[50] + 1000.0
        pred[260] = gt[260] - 2000.0
    return gt, pred, sig, gc, pc


def relativize(pred, x):
    return UB.relativize_uncert(pred, x)


def covered_rows(gt, pred, s):           # the loop of _conf_all:258-265
    correct_all = 0
    for i in range(len(s)):
        if (pred[i] - s[i] <= gt[i]).all() and (gt[i] <= pred[i] + s[i]).all():
            correct_all += 1
    return correct_all


def column_numbers(gt, pred, s):
    res = np.abs(gt - pred)
    ok = ~((s == 0) | ~np.isfinite(s))
    with np.errstate(all="ignore"):
        out = dict(ece_flat=UB.calc_ece(gt.flatten(), pred.flatten(), s.flatten()), ece_box=UB.calc_ece(gt, pred, s),
                   ece_coord=np.array([UB.calc_ece(gt[:, c], pred[:, c], s[:, c]) for c in range(4)]),
                   covered=covered_rows(gt, pred, s), nll=UB.calc_nll(res[ok], s[ok]), nll_raw=UB.calc_nll(res.flatten(), s.flatten()),
                   rmsue=UB.calc_rmse(res.flatten(), s.flatten()), sharp=np.sqrt(np.mean(np.square(s.astype(np.float32).flatten()))),
                   rel_ece_box=CR.RegressionCalib._relative_calc_ece(relativize(pred, res), relativize(pred, s)),
                   rel_ece_coord0=CR.RegressionCalib._relative_calc_ece(relativize(pred, res)[:, 0], relativize(pred, s)[:, 0]))
    return out


def header_numbers(gt, pred, gc, pc):
    ious = UB.calc_iou_np(gt, pred)
    return dict(ious=ious, md=len(ious[ious == 0]) / len(ious) * 100, misc=len(np.where(gc != pc)[0]) / len(gc), miou=np.mean(ious),
                rmse=float(UB.calc_rmse(gt, pred)))


def main():
    out = {"numpy_version": np.array([np.__version__]), "decoding": np.array([DECODING]), "method": np.array([METHOD]),
           "z": stats.norm.ppf((1 - np.linspace(0, 1, 100)) / 2), "class_ids": np.array([1.0, 2.0, 3.0])}
    assert out["z"][0] == 0.0 and out["z"][99] == -np.inf
    for case, n, seed in (("n1", 1, 11), ("n5", 5, 12), ("n300", 300, 13)):
        gt, pred, sig, gc, pc = make_case(n, seed, case)
        for k, v in (("gt", gt), ("pred", pred), ("sigma", sig), ("gt_classes", gc), ("classes", pc)):
            out["%s_%s" % (case, k)] = v
        for k, v in header_numbers(gt, pred, gc, pc).items():
            out["%s_%s" % (case, k)] = np.asarray(v)
        for col in range(2):
            for k, v in column_numbers(gt, pred, sig[col]).items():
                out["%s_c%d_%s" % (case, col, k)] = np.asarray(v)
        with tempfile.TemporaryDirectory() as tmp:
            params = {"num_classes": 3, "uncert_adjust_method": DECODING}
            UE.ValidUncertPlot(gt, pred, gc, pc, sig[0], None, tmp + "/aleatoric", params)
            UE.ValidUncertPlot(gt, pred, gc, pc, sig[1], None, tmp + "/mcdropout", params)
            out[case + "_model_performance"] = np.array([open(tmp + "/model_performance.txt").read()])
            if case != "n5":
                rc = CR.RegressionCalib.__new__(CR.RegressionCalib)
                rc.saving_path, rc.model_name = tmp, "/m"
                os.makedirs(tmp + "/m")
                rc._conf_all(gt, pred, sig[0], sig[0], split=0, calib=False)
                rc._conf_all(gt, pred, sig[0], sig[1], split=0, calib=True, method=METHOD)
                text = open(tmp + "/m/regression_logging.txt").read()
                out[case + "_regression_logging"] = np.array([text])
                for col, line in zip(range(2), text.split("\n")[0::2]):
                    assert line.rstrip().endswith(str(round(out["%s_c%d_covered" % (case, col)] / n * 100, 1))), (case, col, line)
        if case == "n5":
            assert (sig[0, 0] == 0).all() and (pred[1] == gt[1]).all() and (sig[0, 2] == 0).all() and (pred[2] == gt[2]).all()
            assert gt[3, 0] == 0 and out["n5_ious"][4] == 0
        if case == "n300":
            assert np.where(out["n300_ious"] == 0)[0].tolist() == [50, 260] and (gt == 0).sum() == 2 and (np.abs(gt - pred) == 0).sum() == 5
            assert not (gc == 2).any() and (gc == 1).any() and (gc == 3).any() and (gc != pc).any()
            for c in (1, 3):
                m = gc == c
                for k, v in header_numbers(gt[m], pred[m], gc[m], pc[m]).items():
                    out["n300_cls%d_%s" % (c, k)] = np.asarray(v)
                for col in range(2):
                    for k, v in column_numbers(gt[m], pred[m], sig[col][m]).items():
                        out["n300_cls%d_c%d_%s" % (c, col, k)] = np.asarray(v)
    np.savez_compressed(os.path.join(HERE, "uncert_report_golden.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
