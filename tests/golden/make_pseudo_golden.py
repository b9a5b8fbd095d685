"""Generates tests/golden/pseudo_golden.npz by running the REAL reference functions `STAC.score_image`,
`STAC.write_KITTI_pseudo_gt_txt` and `STAC.write_BDD_pseudo_gt_json` (src/SSL_stac.py:202-642) on prediction files written here,
through a SimpleNamespace self.  Their bodies are numpy and json only; the module imports TensorFlow and friends at the top, which
are stubbed (`utils_box.relativize_uncert` stays real).  Run once where a checkout of the reference exists; the .npz (data only) is
committed and is what the tests read.

    python tests/golden/make_pseudo_golden.py <src directory of the reference's checkout>

For every dataset (images with M = 100 rows each) a temporary prediction_data.txt of plain-float literals is written, one dict per
row above min_score = 0.1 as `Infer.iterate_infer` does (infer_model.py:836-960).  The fixture holds the columns as float64
[n, M, ...] - exactly the parsed literals - and per case (dataset, strategy, tau):

  what score_image returned   names, classes, boxes - and the pseudo score of every survivor, for which score_image runs with
                              activate_pseudoscore = True whatever the strategy says (the attribute only adds the fourth return)
  the written files' text     both writers, with activate_pseudoscore as STAC.__init__ derives it from the strategy (n_dets
                              for every case, the text for tau 0.9 and the dataset "z")
  the candidates              rows with det_score > tau among an image's first 99 (gate 0), or the survivors themselves (the
                              single-column branch).  For gate 0 they are what the reference returns for `ental` on the same
                              file and tau (its final filter IS filter_based_on_sigmoid); rows are found by their boxes
  the intermediate v          of every row that takes part, where the reference's own arithmetic exposes it: the numpy module
                              score_image sees is a recording proxy, so 1 / np.mean([...], axis=0) gives v of the multi-column
                              branches; for `combo` the proxy records np.mean(relativize_uncert(...)) per row and v is the
                              reference's expression opt_params[0] * entropy + opt_params[1] * that; in the single-column
                              branch the survivors' pseudo score is v and the other rows' v is not stored

The conditions the tests rely on are asserted below: every branch of the grammar; images with 0, 1, 2, 63, 64, 65, 98, 99 kept rows
for every branch and one with 100 for the single-column branches (the multi-column branches of the reference raise IndexError on
it; `check_reference_fails_on_100` shows that), whose 100th row would pass the filter; C = 3 and C = 10; tau 0.4 and 0.9; in every
case both outcomes of the final filter, an image dropped and an image kept; a det_score equal to tau (not kept); under `combo` the
dataset's minimum, which normalises to exactly 0 (dropped) although its det_score passes; apart from those, no compared quantity
within 1e-6 of its threshold.  The dataset "z" holds the non-finite cases - a zero-height box (v = inf) and a zero-width box with
sigma 0 on that side (0 / 0 = NaN) - for which the outcome assertions do not apply (under `combo` the maximum inf sends every
finite value to 0 and nothing survives: that is the point)."""
import json
import os
import sys
import tempfile
import types
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_pseudo_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
for name in ("tensorflow", "tensorflow_probability", "uncertainty_toolbox", "uncertainty_toolbox.viz", "absl", "absl.logging",
             "imagehash", "uncertainty_analysis", "cv2", "datasets", "datasets.BDD100K", "datasets.BDD100K.bdd_tf_creator",
             "datasets.KITTI", "datasets.KITTI.kitti_tf_creator"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
import numpy as np                       # noqa: E402
import SSL_stac as SS                    # noqa: E402  (the reference module)

STAC = SS.STAC
M = 100
MIN_SCORE = 0.1
MAX_ROWS = 99
KEPT = [1, 2, 0, 63, 64, 65, 98, 99, 7, 100]       # kept rows per image; the image with 100 is the last: the multi-column cases stop before it
OPT = (0.7, 1.3)
OPT_THRS = (0.04, 0.12)
TAUS = (0.4, 0.9)
KITTI = ["car", "van", "truck", "pedestrian", "person_sitting", "cyclist", "tram"]          # STAC.select_classes
BDD = ["pedestrian", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle", "traffic light", "traffic sign"]
DATASETS = {"a": (3, KITTI), "b": (10, BDD), "z": (3, KITTI)}
MULTI = ("combo", "alluncert", "epuncert", "ental")
STRATEGIES = ["score", "pseudoscore_score", "combo", "pseudoscore_combo", "alluncert", "pseudoscore_epuncert", "ental", "entropy",
              "box_norm_albox", "box_albox", "class_mcclass", "sota"]
CASES = [("a", s, t) for s in STRATEGIES for t in TAUS]
CASES += [("b", s, t) for s in ("class_mcclass", "alluncert", "pseudoscore_epuncert", "pseudoscore_combo", "entropy") for t in TAUS]
CASES += [("z", s, 0.4) for s in ("pseudoscore_combo", "pseudoscore_box_norm_albox", "pseudoscore_ental", "alluncert")]


class NumpyProxy:
    """numpy as score_image sees it: everything forwarded, the results of np.mean recorded."""

    def __init__(self):
        self.rel, self.axis0 = [], []

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, a, axis=None):
        res = np.mean(a, axis=axis)
        if axis == 0:
            self.axis0.append(np.array(res, np.float64))
        elif isinstance(a, np.ndarray) and a.shape == (1, 4):
            self.rel.append(float(res))
        return res


def is_multi(strategy):
    return any(w in strategy for w in MULTI)


def make_dataset(rng, C, kept_list, nonfinite=False):
    n = len(kept_list)
    r4 = lambda a: np.round(a, 4)          # noqa: E731  (the writer rounds uncertainties to 4 decimals)
    cols = dict(boxes=np.zeros((n, M, 4)), scores=np.zeros((n, M)), classes=np.zeros((n, M)), entropy=np.zeros((n, M)),
                albox=np.zeros((n, M, 4)), mcbox=np.zeros((n, M, 4)), mcclass=np.zeros((n, M, C)))
    for i, k in enumerate(kept_list):
        below = min(M - k, 4)               # a few real rows under the writer's threshold, then padding (score 0)
        sc = np.concatenate([np.sort(rng.uniform(MIN_SCORE + 0.01, 0.99, k))[::-1], np.sort(rng.uniform(0.02, MIN_SCORE, below))[::-1]])
        rows = k + below
        cols["scores"][i, :rows] = np.round(sc, 6)
        y1, x1 = rng.uniform(0, 300, rows), rng.uniform(0, 1100, rows)
        h, w = np.exp(rng.uniform(np.log(0.5), np.log(80), rows)), np.exp(rng.uniform(np.log(0.5), np.log(80), rows))
        cols["boxes"][i, :rows] = np.round(np.column_stack([y1, x1, y1 + h, x1 + w]), 3)
        cols["classes"][i, :rows] = rng.integers(1, C + 1, rows).astype(np.float64)
        scale = lambda: rng.uniform(0.3, 3.0, (rows, 1))          # noqa: E731  (rows differ in how uncertain they are)
        cols["entropy"][i, :rows] = r4(rng.uniform(0.05, np.log2(C), rows) * rng.uniform(0.2, 1.0, rows))
        cols["albox"][i, :rows] = r4(0.02 + rng.gamma(2.0, 0.25, (rows, 4)) * scale())
        cols["mcbox"][i, :rows] = r4(0.02 + rng.gamma(2.0, 0.2, (rows, 4)) * scale())
        cols["mcclass"][i, :rows] = r4(0.02 + rng.gamma(2.0, 0.2, (rows, C)) * scale())
    if nonfinite:
        cols["boxes"][0, 0, 2] = cols["boxes"][0, 0, 0]                       # zero height, sigma > 0: x / 0 = inf
        cols["boxes"][1, 0, 3] = cols["boxes"][1, 0, 1]                       # zero width, sigma 0 on that side: 0 / 0 = NaN
        cols["albox"][1, 0, [1, 3]] = 0.0
        cols["scores"][:, 1:] = np.minimum(cols["scores"][:, 1:], 0.94)
        cols["scores"][0, 0], cols["scores"][1, 0] = 0.95, 0.96               # (both pass the det_score filter)
        return cols
    # designed rows.  Image 3 (63 kept): row 0 is the dataset's most certain row - every uncertainty at its floor in a big box, so
    # it is the maximum of every 1 / mean and normalises to 1 - and row 1 the dataset's `combo` minimum, exactly 0; both pass the
    # det_score filter at either tau.
    cols["scores"][3, 0], cols["scores"][3, 1] = 0.985, 0.975
    cols["scores"][3, 2:63] = np.minimum(cols["scores"][3, 2:63], 0.97)
    cols["boxes"][3, 0], cols["boxes"][3, 1] = [10.0, 20.0, 90.0, 100.0], [12.0, 22.0, 92.0, 102.0]
    cols["entropy"][3, 0], cols["albox"][3, 0], cols["mcbox"][3, 0], cols["mcclass"][3, 0] = 0.1, 0.02, 0.02, 0.1
    cols["entropy"][3, 1], cols["albox"][3, 1] = 0.0, 0.0
    # image 0 (1 kept): a sure, low-scored row - no filter passes it, the image is dropped in every case
    cols["scores"][0, 0], cols["boxes"][0, 0] = 0.2, [30.0, 40.0, 95.0, 111.0]
    cols["entropy"][0, 0], cols["albox"][0, 0], cols["mcbox"][0, 0], cols["mcclass"][0, 0] = 0.3, 0.05, 0.05, 0.3
    # image 4 (64 kept): det_scores exactly at the two taus - not kept at their own tau
    for tau in TAUS:
        r = int(np.argmin(np.abs(cols["scores"][4, :64] - tau)))
        cols["scores"][4, r] = tau
    assert (np.diff(cols["scores"][4, :64]) <= 0).all() and (np.diff(cols["scores"][3, :63]) <= 0).all()
    # the image with 100 kept rows: its 100th row is very uncertain, so every single-column uncertainty filter would pass it
    last = len(kept_list) - 1
    assert kept_list[last] == 100
    cols["entropy"][last, 99], cols["albox"][last, 99], cols["mcclass"][last, 99] = 1.5, 9.0, 5.0
    cols["boxes"][last, 99] = [5.0, 5.0, 6.0, 6.0]
    return cols


def write_file(path, cols, names, n):
    per_image = []
    with open(path, "w") as f:
        for i, name in enumerate(names[:n]):
            rows = np.where(cols["scores"][i] > MIN_SCORE)[0]
            per_image.append(len(rows))
            for r in rows:
                d = {"image_name": name, "score_thresh": MIN_SCORE, "det_score": float(cols["scores"][i, r]),
                     "bbox": [float(v) for v in cols["boxes"][i, r]], "class": float(cols["classes"][i, r]),
                     "entropy": float(cols["entropy"][i, r]), "uncalib_mcclass": [float(v) for v in cols["mcclass"][i, r]],
                     "uncalib_albox": [float(v) for v in cols["albox"][i, r]], "uncalib_mcbox": [float(v) for v in cols["mcbox"][i, r]]}
                f.write(str(d) + "\n")
    return per_image


def run_reference(path, strategy, tau, pseudoscore):
    proxy = NumpyProxy()
    ns = types.SimpleNamespace(selection_strategy=strategy, opt_params=list(OPT), opt_thrs=list(OPT_THRS), tau=tau,
                               activate_pseudoscore=pseudoscore)
    SS.np = proxy
    try:
        with np.errstate(all="ignore"):
            out = STAC.score_image(ns, path, None)
    finally:
        SS.np = np
    return out, proxy


def run_writers(td, strategy, returned, select_classes):
    """Both writers on what score_image returned, as predict_teacher hands it over (:1013-1033)."""
    pseudoscore = "pseudoscore" in strategy                   # STAC.__init__:76-78
    ns = types.SimpleNamespace(activate_pseudoscore=pseudoscore, pred_imgs_names=returned[0],
                               pred_classes=[[select_classes[int(c) - 1] for c in c_im] for c_im in returned[1]], pred_boxes=returned[2])
    if pseudoscore:
        ns.pseudo_score = returned[3]
    ns.output_dir = os.path.join(td, "kitti_out")
    n_k = STAC.write_KITTI_pseudo_gt_txt(ns)
    files = sorted(os.listdir(ns.output_dir))
    texts = [open(os.path.join(ns.output_dir, f)).read() for f in files]
    for f in files:
        os.remove(os.path.join(ns.output_dir, f))
    ns.output_dir = os.path.join(td, "bdd_out")
    n_b = STAC.write_BDD_pseudo_gt_json(ns)
    bdd = open(os.path.join(ns.output_dir, "pseudo_labels.json")).read()
    json.loads(bdd.replace("Infinity", "1e999"))
    assert n_k == n_b == sum(len(c) for c in returned[1])
    return files, texts, bdd, n_k


def rows_of(cols, names, returned):
    """(image, row) of every returned detection, found by its box among the image's first 99 written rows."""
    img, row = [], []
    for name, boxes in zip(returned[0], returned[2]):
        i = names.index(str(name))
        for b in boxes:
            hit = np.where((cols["boxes"][i] == np.asarray(b)).all(1))[0]
            assert len(hit) == 1, (name, b)
            img.append(i)
            row.append(int(hit[0]))
    return np.asarray(img, np.int64), np.asarray(row, np.int64)


def far(values, threshold, what, eps=1e-6):
    v = np.asarray(values, np.float64)
    v = v[np.isfinite(v)]
    assert not len(v) or np.abs(v - threshold).min() > eps, (what, threshold, float(np.abs(v - threshold).min()))


def check_reference_fails_on_100(td, cols, names):
    path = os.path.join(td, "full.txt")
    write_file(path, cols, names, len(names))
    for strategy in ("combo", "alluncert", "epuncert", "ental"):
        try:
            run_reference(path, strategy, 0.0, False)          # (tau 0: the image has survivors, which is what it takes)
        except IndexError:
            continue
        raise AssertionError("the reference's %s branch did not raise on an image with 100 written rows" % strategy)


def main():
    rng = np.random.default_rng(20241018)
    names = ["%06d.png" % (7 * i + 3) for i in range(len(KEPT))]
    out = {"M": np.array([M]), "min_score": np.array([MIN_SCORE]), "max_rows": np.array([MAX_ROWS]), "names": np.array(names),
           "opt_params": np.array(OPT), "opt_thrs": np.array(OPT_THRS), "kept": np.array(KEPT), "datasets": np.array(sorted(DATASETS)),
           "case_dataset": np.array([c[0] for c in CASES]), "case_strategy": np.array([c[1] for c in CASES]),
           "case_tau": np.array([c[2] for c in CASES])}
    data, kept_of = {}, {}
    with tempfile.TemporaryDirectory() as td:
        for ds, (C, select_classes) in DATASETS.items():
            kept_list = [5, 6, 0, 4] if ds == "z" else KEPT
            cols = make_dataset(rng, C, kept_list, nonfinite=(ds == "z"))
            data[ds], kept_of[ds] = cols, kept_list
            out["%s_num_classes" % ds], out["%s_kept" % ds] = np.array([C]), np.array(kept_list)
            out["%s_class_names" % ds] = np.array(select_classes)
            for k, v in cols.items():
                out["%s_%s" % (ds, k)] = v
            assert (np.sum(cols["scores"] > MIN_SCORE, 1) == kept_list).all()
            # two files per dataset: every image (single-column branches), and without the image of 100 rows (multi-column)
            for tag, n in (("all", len(kept_list)), ("multi", len(kept_list) - (ds != "z"))):
                assert write_file(os.path.join(td, "%s_%s.txt" % (ds, tag)), cols, names, n) == kept_list[:n]
        check_reference_fails_on_100(td, data["a"], names)
        reached = set()
        for ci, (ds, strategy, tau) in enumerate(CASES):
            cols, kept_list = data[ds], kept_of[ds]
            C, select_classes = DATASETS[ds]
            multi = is_multi(strategy)
            n = len(kept_list) - (1 if multi and ds != "z" else 0)
            path = os.path.join(td, "%s_%s.txt" % (ds, "multi" if multi else "all"))
            returned, proxy = run_reference(path, strategy, tau, True)
            plain, _ = run_reference(path, strategy, tau, False)
            assert len(plain) == 3 and all(np.array_equal(a, b) for a, b in zip(plain[1], returned[1]))
            files, texts, bdd, n_dets = run_writers(td, strategy, returned if "pseudoscore" in strategy else plain, select_classes)
            img, row = rows_of(cols, names, returned)
            pseudo = np.concatenate(returned[3]) if len(returned[3]) else np.zeros((0,))
            written = [i for i in range(n) if kept_list[i]]
            part = {i: np.where(cols["scores"][i] > MIN_SCORE)[0][:MAX_ROWS] for i in written}
            out["k%d_n" % ci] = np.array([n])
            out["k%d_names" % ci] = np.asarray(returned[0])
            out["k%d_count" % ci] = np.array([len(c) for c in returned[1]])
            out["k%d_image" % ci], out["k%d_row" % ci] = img, row
            out["k%d_classes" % ci] = np.concatenate(returned[1]) if len(returned[1]) else np.zeros((0,))
            out["k%d_boxes" % ci] = np.concatenate(returned[2]) if len(returned[2]) else np.zeros((0, 4))
            out["k%d_pseudo" % ci] = pseudo
            out["k%d_n_dets" % ci] = np.array([n_dets])
            if tau == TAUS[1] or ds == "z":                  # (the texts of the smaller selections: the fixture stays small)
                out["k%d_kitti_files" % ci], out["k%d_kitti_texts" % ci] = np.array(files), np.array(texts)
                out["k%d_bdd" % ci] = np.array([bdd])
            # the candidates and the intermediate v
            if multi:
                sig, _ = run_reference(path, "ental", tau, True)
                cimg, crow = rows_of(cols, names, sig)
                if "combo" in strategy:
                    rel = iter(proxy.rel)
                    v_all = {i: np.asarray([OPT[0] * float(cols["entropy"][i, r]) + OPT[1] * next(rel) for r in np.where(cols["scores"][i] > MIN_SCORE)[0]])[:MAX_ROWS] for i in written}
                    assert next(rel, None) is None
                    branch = "combo"
                else:
                    assert len(proxy.axis0) == len(written)
                    with np.errstate(all="ignore"):
                        v_all = {i: 1 / a for i, a in zip(written, proxy.axis0)}
                    branch = [w for w in MULTI[1:] if w in strategy][0]
                assert all(len(v_all[i]) == len(part[i]) for i in written)
                minmax = np.tile([np.inf, -np.inf], (n, 1))
                for i in written:
                    for item in v_all[i]:                       # find_global_min_max's running rule
                        minmax[i] = min(minmax[i, 0], item), max(minmax[i, 1], item)
                cv = np.asarray([v_all[i][list(part[i]).index(r)] for i, r in zip(cimg, crow)])
                out["k%d_minmax" % ci] = minmax
            else:
                cimg, crow, cv = img, row, pseudo
                branch = "single:" + ("det_score" if strategy.split("_")[-1] in ("score", "sota") else strategy.split("_")[-1])
            reached.add(branch)
            out["k%d_cand_image" % ci], out["k%d_cand_row" % ci], out["k%d_cand_v" % ci] = cimg, crow, cv
            out["k%d_cand_classes" % ci] = np.asarray([cols["classes"][i, r] for i, r in zip(cimg, crow)])
            out["k%d_cand" % ci] = np.bincount(cimg, minlength=n)[:n]
            surv, ncand = len(img), len(cimg)
            print("%-2s %-28s tau %.1f  images %d -> %d  candidates %d  survivors %d" % (ds, strategy, tau, len(written), len(returned[0]), ncand, surv))
            if ds == "z":
                continue
            total = sum(len(part[i]) for i in written)
            assert 0 < surv < total, (strategy, tau, surv, total)                      # both outcomes of the final filter
            assert 0 < len(returned[0]) < len(written), (strategy, tau)                  # an image dropped, an image kept
            sc = np.concatenate([cols["scores"][i, part[i]] for i in written])
            if multi:
                assert (sc == tau).sum() == 1 and not any((i == 4 and cols["scores"][i, r] == tau) for i, r in zip(cimg, crow))
                far(sc[sc != tau], tau, "det_score")
                lo, hi = min(minmax[:, 0]), max(minmax[:, 1])
                with np.errstate(all="ignore"):
                    norm = (cv - lo) / (hi - lo)
                if "combo" in strategy:
                    assert (norm == 0).sum() == 1 and ncand > surv                      # the dataset's minimum passes det_score and is dropped
                    far(norm[norm != 0], 0.0, "combo > 0")
                    far(norm, np.mean(OPT_THRS), "combo bound")
                    assert ((norm > 0) & (norm <= np.mean(OPT_THRS))).sum() == surv and (norm > np.mean(OPT_THRS)).any()
                elif "alluncert" in strategy:
                    far(norm, tau, "alluncert")
                    assert (norm > tau).sum() == surv and ncand > surv
            else:
                if branch == "single:det_score":
                    assert (sc == tau).sum() == 1
                    far(sc[sc != tau], tau, "det_score")
                far(cv, tau, "v")
        for word in ("combo", "alluncert", "epuncert", "ental", "single:det_score", "single:entropy", "single:albox", "single:mcclass"):
            assert word in reached, word
        # the cap is pinned: the 100th row of the last image passes a single-column filter, and the reference drops it
        ci = CASES.index(("a", "entropy", 0.4))
        last = len(KEPT) - 1
        assert data["a"]["entropy"][last, 99] > 0.9 and not ((out["k%d_image" % ci] == last) & (out["k%d_row" % ci] == 99)).any()
        assert ((out["k%d_image" % ci] == last)).any()
    assert {0, 1, 2, 63, 64, 65, 98, 99, 100} <= set(KEPT)
    dst = os.path.join(HERE, "pseudo_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 1000000


if __name__ == "__main__":
    main()
