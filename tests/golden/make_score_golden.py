"""Generates tests/golden/score_golden.npz by running the REAL reference functions `ActiveLearning.score_image` and
`ActiveLearning.select_images` (src/active_learning_loop.py:528-840) on prediction files written here.  Their bodies are numpy
only; the module imports TensorFlow and friends at the top, which are stubbed.  Run once where a checkout of the reference
exists; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_score_golden.py <src directory of the reference's checkout>

For every dataset (a pool of images with M = 100 rows each) a temporary prediction_data.txt of plain-float literals is written,
one dict per row above min_score as `Infer.iterate_infer` does (infer_model.py:836-960).  The fixture holds the columns as
float64 [n, M, ...] - exactly the parsed literals - and per case (dataset, strategy, num_per_iter) what the reference returned:
the per-image columns before the dataset-wide combination (captured where the reference hands them to its min_max_scaler /
z_score_normalization), the per-image score after it, and the indices `select_images` returns.

The conditions the tests rely on are asserted below: every branch of the strategy grammar, images with 1, 2, 7, 8, 9 and 100
kept rows and one with none, C = 3 and C = 10, a `perc` case whose middle class nobody predicts, num_per_iter >= 5 for `nee`,
box sides >= 8 px, non-negative uncertainties / entropies / weights, every scaled column with spread > 0 and final per-image
scores pairwise further apart than 1e-6."""
import os
import sys
import tempfile
import types
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_score_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
for name in ("tensorflow", "tensorflow_probability", "uncertainty_toolbox", "uncertainty_toolbox.viz", "absl", "absl.logging",
             "imagehash", "uncertainty_analysis", "cv2", "datasets", "datasets.BDD100K", "datasets.BDD100K.bdd_tf_creator",
             "datasets.KITTI", "datasets.KITTI.kitti_tf_creator"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np                       # noqa: E402
import active_learning_loop as ALL      # noqa: E402  (the reference module)
import score_ref as S                    # noqa: E402  (only for the separation check of the `perc` cases)

AL = ALL.ActiveLearning
M = 100
MIN_SCORE = 0.3
KEPT = [1, 2, 7, 8, 0, 9, 100, 3, 5, 16, 33, 64, 4]           # kept rows per image; the image with 0 never reaches the file
# name -> (num_classes, classes that occur)
DATASETS = {"a": (3, [1, 2, 3]), "b": (10, list(range(1, 11))), "c": (3, [1, 3])}
OPT = (0.7, 1.3)
# (dataset, strategy, num_per_iter)
CASES = [("a", "entropy", 4), ("a", "mean_entropy", 4), ("b", "alluncert", 5), ("b", "mean_alluncert_highep_lowal", 3),
         ("b", "sota", 4), ("b", "epuncert", 4), ("a", "ental", 4), ("a", "mean_ental", 2), ("a", "combo", 4),
         ("a", "box_norm_albox", 4), ("a", "box_albox", 4), ("b", "class_mcclass", 4), ("a", "class_mcclass", 4),
         ("a", "box_norm_mcbox", 3), ("a", "foo", 4), ("c", "perc_entropy", 4), ("b", "perc_mean_alluncert", 6),
         ("b", "nee_entropy", 7), ("a", "nee_mean_epuncert", 5), ("a", "bottomk_entropy", 4), ("b", "bottomk_sota", 3)]


def make_dataset(rng, C, present):
    n = len(KEPT)
    r4 = lambda a: np.round(a, 4)          # noqa: E731  (the writer rounds uncertainties to 4 decimals)
    cols = dict(boxes=np.zeros((n, M, 4)), scores=np.zeros((n, M)), classes=np.zeros((n, M)), entropy=np.zeros((n, M)),
                albox=np.zeros((n, M, 4)), mcbox=np.zeros((n, M, 4)), mcclass=np.zeros((n, M, C)))
    for i, k in enumerate(KEPT):
        below = min(M - k, 6)               # a few real rows under the threshold, then padding (score 0)
        sc = np.concatenate([np.sort(rng.uniform(MIN_SCORE + 0.01, 0.99, k))[::-1], np.sort(rng.uniform(0.02, MIN_SCORE, below))[::-1]])
        if below:
            sc[k] = MIN_SCORE               # exactly at the threshold: not kept (strict compare)
        rows = k + below
        cols["scores"][i, :rows] = np.round(sc, 6)
        y1, x1 = rng.uniform(0, 300, rows), rng.uniform(0, 1100, rows)
        h, w = rng.uniform(8.01, 70, rows), rng.uniform(8.01, 140, rows)
        cols["boxes"][i, :rows] = np.round(np.column_stack([y1, x1, y1 + h, x1 + w]), 3)
        cols["classes"][i, :rows] = rng.choice(present, rows).astype(np.float64)
        scale = rng.uniform(0.3, 3.0)       # images differ in how uncertain they are
        cols["entropy"][i, :rows] = r4(rng.uniform(0, np.log2(C), rows) * min(scale, 1.0))
        cols["albox"][i, :rows] = r4(rng.gamma(2.0, 1.5, (rows, 4)) * scale)
        cols["mcbox"][i, :rows] = r4(rng.gamma(2.0, 0.8, (rows, 4)) * rng.uniform(0.3, 3.0))
        cols["mcclass"][i, :rows] = r4(rng.gamma(2.0, 0.2, (rows, C)) * rng.uniform(0.3, 3.0))
        if k:
            cols["classes"][i, :min(k, len(present))] = present[:min(k, len(present))]
    kept = cols["scores"] > MIN_SCORE
    assert sorted(set(cols["classes"][kept].astype(int))) == sorted(present)
    side = np.minimum(cols["boxes"][..., 2] - cols["boxes"][..., 0], cols["boxes"][..., 3] - cols["boxes"][..., 1])
    assert side[cols["scores"] > 0].min() >= 8
    assert min(cols[k].min() for k in ("entropy", "albox", "mcbox", "mcclass")) >= 0
    return cols


def write_file(path, cols, names):
    lines = 0
    with open(path, "w") as f:
        for i, name in enumerate(names):
            for r in np.where(cols["scores"][i] > MIN_SCORE)[0]:
                d = {"image_name": name, "score_thresh": MIN_SCORE, "det_score": float(cols["scores"][i, r]),
                     "bbox": [float(v) for v in cols["boxes"][i, r]], "class": float(cols["classes"][i, r]),
                     "entropy": float(cols["entropy"][i, r]), "uncalib_mcclass": [float(v) for v in cols["mcclass"][i, r]],
                     "uncalib_albox": [float(v) for v in cols["albox"][i, r]], "uncalib_mcbox": [float(v) for v in cols["mcbox"][i, r]]}
                f.write(str(d) + "\n")
                lines += 1
    return lines


def run_reference(path, strategy, num_per_iter, im_names):
    seen = []

    def rec(fn):
        def wrapped(col):
            seen.append(np.array(col, np.float64))
            return fn(col)
        return wrapped

    ns = types.SimpleNamespace(scoring_strategy=strategy, opt_params=list(OPT), min_max_scaler=rec(AL.min_max_scaler),
                               z_score_normalization=rec(AL.z_score_normalization), num_per_iter=num_per_iter, im_names=im_names)
    ns.score_image = lambda p: AL.score_image(ns, p)
    per_image, pred_classes, names = AL.score_image(ns, path)
    comps = np.stack(seen, 1) if seen else np.asarray(per_image, np.float64)[:, None]
    del seen[:]
    picked = AL.select_images(ns, path)
    return comps, np.asarray(per_image, np.float64), pred_classes, list(names), np.asarray(picked, np.int64)


def main():
    rng = np.random.default_rng(20241017)
    n = len(KEPT)
    names = ["%06d.jpg" % (7 * i + 3) for i in range(n)]                 # served sorted: np.unique keeps the order
    im_names = [nm.replace(".jpg", ".png") for nm in names[::-1]] + ["999999.png"]
    out = {"M": np.array([M]), "min_score": np.array([MIN_SCORE]), "names": np.array(names), "im_names": np.array(im_names),
           "opt_params": np.array(OPT), "kept": np.array(KEPT), "datasets": np.array(sorted(DATASETS)),
           "case_dataset": np.array([c[0] for c in CASES]), "case_strategy": np.array([c[1] for c in CASES]),
           "case_num_per_iter": np.array([c[2] for c in CASES])}
    data = {}
    with tempfile.TemporaryDirectory() as td:
        for ds, (C, present) in DATASETS.items():
            cols = make_dataset(rng, C, present)
            data[ds] = cols
            path = os.path.join(td, ds + ".txt")
            assert write_file(path, cols, names) == sum(KEPT)
            out["%s_num_classes" % ds] = np.array([C])
            for k, v in cols.items():
                out["%s_%s" % (ds, k)] = v
            assert (np.sum(cols["scores"] > MIN_SCORE, 1) == KEPT).all()
        kept_names = [nm for nm, k in zip(names, KEPT) if k]
        for ci, (ds, strategy, npi) in enumerate(CASES):
            comps, final, pred_classes, ref_names, picked = run_reference(os.path.join(td, ds + ".txt"), strategy, npi, im_names)
            assert ref_names == kept_names and comps.shape[0] == len(kept_names) and final.shape == (len(kept_names),)
            assert [len(c) for c in pred_classes] == [k for k in KEPT if k]
            assert "nee" not in strategy or npi >= 5
            if comps.shape[1] > 1:
                assert (comps.max(0) - comps.min(0)).min() > 0
            ranked = final
            if "perc" in strategy:
                C = DATASETS[ds][0]
                cc = np.stack([np.bincount(np.asarray(c, int) - 1, minlength=C) for c in pred_classes])
                ranked = S.class_weighted(final, cc)
            gaps = np.diff(np.sort(ranked))
            assert gaps.min() > 1e-6, (strategy, gaps.min())
            assert 0 < len(picked) <= npi and ("nee" in strategy or len(picked) == npi), (strategy, picked)
            out["k%d_components" % ci], out["k%d_scores" % ci], out["k%d_selected" % ci] = comps, final, picked
            print("%-2s %-30s columns %d  min gap %.3g  selected %s" % (ds, strategy, comps.shape[1], gaps.min(), picked.tolist()))
    strategies = " ".join(c[1] for c in CASES)
    for word in ("entropy", "mean_entropy", "alluncert", "highep_lowal", "sota", "epuncert", "ental", "combo", "box_norm_albox",
                 "box_albox", "class_mcclass", "foo", "perc_", "nee_", "bottomk_"):
        assert word in strategies, word
    assert {1, 2, 7, 8, 9, 100, 0} <= set(KEPT)
    dst = os.path.join(HERE, "score_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 1000000


if __name__ == "__main__":
    main()
