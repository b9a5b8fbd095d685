"""Generates tests/golden/class_report_golden.npz by running the REAL reference functions `ClassificationCalib._calibr_bins`
(src/calibrate_classification.py:97-143) and `stable_softmax` (src/utils_class.py:36-41) on arrays made here.  Run once where a
checkout of the reference exists; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_class_report_golden.py <src directory of the reference's checkout>

How the functions are reached: tensorflow and friends, sklearn, matplotlib, absl and yaml are stubbed (neither function touches
them); `_calibr_bins` runs on an object made with `__new__` whose `all_classes`, `quantilestrategy` and `n_bins` are set as
`_calibr_plot` sets them, once per class with the column as `_calibr_plot` passes it (:353-356) and once with `all_classes`
(:392-393).  The edges it bins with are not kept by the reference: they are read off its `np.digitize` call.

Cases: n1, n7 and n300 rows of C = 3 probabilities in [0, 1], each under the uniform and the quantile strategy.  n300 is the real
`stable_softmax` of seeded float32 logits (recorded as `n300_logits` / `n300_softmax`) with planted rows on top; a C = 10 softmax
is recorded too (`c10_logits` / `c10_softmax`).  Planted, and asserted in main(): a probability exactly on an edge (element k
of np.linspace(0, 1 + 1e-8, 11)), p = 0, p = 1, a two-way tie of the row maximum, and a (case, target) with an empty bin in the
middle.  All probabilities lie in [0, 1], so the reference's `bins[nonzero]` never raises on these inputs: asserted by running it.
Recorded per (case, strategy, target t0 / t1 / t2 / all): edges, freq, prob, bin_prob, bin_count, ece, mce; per case the Brier
expressions of _calibr_plot (:370 per class, :391 over all) restated here; numpy's version."""
import os
import sys
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_class_report_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
import numpy as np                       # noqa: E402

for name in ("tensorflow", "tensorflow.python", "tensorflow.python.training", "tensorflow_probability", "sklearn", "sklearn.isotonic",
             "matplotlib", "absl", "yaml"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
import calibrate_classification as CC    # noqa: E402  (the reference modules)
import utils_class as UC                 # noqa: E402

C = 3
EDGES = np.linspace(0.0, 1.0 + 1e-8, 11)


def make_case(case):
    if case == "n1":
        return np.array([[0.2, 0.7, 0.1]]), np.array([1]), None
    if case == "n7":
        p = np.array([[0.0, 1.0, 0.0],                       # p = 0 and p = 1
                      [EDGES[3], 0.5, 0.2],                  # exactly on an edge
                      [0.4, 0.4, 0.2],                       # the row maximum twice: argmax takes the first
                      [0.05, 0.15, 0.8], [0.33, 0.33, 0.34], [0.9, 0.05, 0.05], [0.25, 0.65, 0.1]])
        return p, np.array([1, 0, 1, 2, 0, 0, 2]), None
    rng = np.random.default_rng(21)
    logits = rng.normal(0, 2.5, (300, C)).astype(np.float32)
    soft = UC.stable_softmax(logits)
    p = soft.astype(np.float64)
    label = np.where(rng.uniform(size=300) < 0.7, p.argmax(axis=1), rng.integers(0, C, 300))
    p[3] = [0.0, 1.0, 0.0]
    p[10] = [EDGES[7], 0.2, 0.1]
    p[11] = [0.1, EDGES[1], 0.6]
    p[20] = [0.45, 0.45, 0.1]
    mid = (p[:, 1] >= EDGES[5]) & (p[:, 1] < EDGES[6])       # empty the sixth bin of class 1
    p[mid, 1] += 0.1
    return p, label, (logits, soft)


def run_bins(y_true, y_pred, all_classes, quantile):
    obj = CC.ClassificationCalib.__new__(CC.ClassificationCalib)
    obj.all_classes, obj.quantilestrategy, obj.n_bins = all_classes, quantile, 10
    seen = {}
    real = np.digitize

    def digitize(x, bins):
        seen["edges"] = np.array(bins, np.float64)
        return real(x, bins)
    with mock.patch.object(np, "digitize", digitize):
        obj._calibr_bins(y_true=y_true, y_pred=y_pred)       # (raises an IndexError for a value at or above the last edge)
    return dict(edges=seen["edges"], freq=obj.freq, prob=obj.prob, bin_prob=obj.bin_prob, bin_count=obj.bin_count,
                ece=np.asarray(obj.ece), mce=np.asarray(obj.mce))


def main():
    out = {"numpy_version": np.array([np.__version__]), "uniform_edges": EDGES}
    rng = np.random.default_rng(22)
    c10 = rng.normal(0, 3, (40, 10)).astype(np.float32)
    out["c10_logits"], out["c10_softmax"] = c10, UC.stable_softmax(c10)
    empty_middle = False
    for case in ("n1", "n7", "n300"):
        p, label, extra = make_case(case)
        assert p.min() >= 0.0 and p.max() <= 1.0 and p.dtype == np.float64
        y_true = np.squeeze(np.eye(C)[label.astype(int).reshape(-1)]).reshape(len(p), C)     # (:40)
        out[case + "_prob"], out[case + "_label"] = p, label.astype(np.int32)
        if extra is not None:
            out[case + "_logits"], out[case + "_softmax"] = extra
        out[case + "_brier"] = np.array([np.mean((p[:, t] - y_true[:, t]) ** 2) for t in range(C)])       # (:370)
        out[case + "_brier_all"] = np.asarray(np.mean((p - y_true) ** 2))                                  # (:391)
        for strategy, quantile in (("uniform", False), ("quantile", True)):
            for t in list(range(C)) + ["all"]:
                if t == "all":
                    r = run_bins(y_true, p, True, quantile)
                else:
                    r = run_bins(y_true[:, t], p[:, t].astype("float64"), False, quantile)
                for k, v in r.items():
                    out["%s_%s_t%s_%s" % (case, strategy, t, k)] = np.asarray(v)
                if not quantile:
                    assert np.array_equal(r["edges"], EDGES)
                    x = p[:, t] if t != "all" else p[np.arange(len(p)), p.argmax(axis=1)]
                    total = np.bincount(np.digitize(x, EDGES), minlength=11)
                    filled = np.where(total != 0)[0]
                    empty_middle |= bool(len(filled)) and bool((total[filled[0]:filled[-1]] == 0).any())
        if case in ("n7", "n300"):
            assert (p == 0.0).any() and (p == 1.0).any() and np.isin(p, EDGES[1:-1]).any()
            top = p.max(axis=1, keepdims=True)
            assert ((p == top).sum(axis=1) == 2).any()
    assert empty_middle
    assert out["n300_uniform_t1_bin_count"].shape == (9,) and EDGES[6] not in out["n300_uniform_t1_bin_prob"]
    np.savez_compressed(os.path.join(HERE, "class_report_golden.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
