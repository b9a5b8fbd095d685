"""numpy restatement of the reference's active-learning scoring (src/active_learning_loop.py:528-840) on COLUMNS instead of
parsed file lines: what `ActiveLearning.score_image` computes per detection and per image, the dataset-wide combination, and
`select_images`.  The numpy calls are the reference's own (np.mean / np.max of python lists, np.insert, np.array_split,
sorted), so the results are the reference's to the last bit for equal inputs; tests/golden/score_golden.npz holds what the
reference itself returned.

Columns: dict with boxes [n, M, 4], scores [n, M], classes [n, M] and, as needed, entropy [n, M], albox / mcbox [n, M, 4],
mcclass [n, M, C'] - float64 (the parsed literals of a file, or float32 device columns converted)."""
import numpy as np


def relativize_uncert(pred_boxes, box_uncert):
    """utils_box.relativize_uncert (utils_box.py:279-292)."""
    pred_boxes, box_uncert = np.asarray(pred_boxes), np.asarray(box_uncert)
    width = pred_boxes[:, 3] - pred_boxes[:, 1]
    height = pred_boxes[:, 2] - pred_boxes[:, 0]
    return box_uncert / np.swapaxes([height, width, height, width], 0, 1)


def components_of(strategy, opt_params=None):
    """(components, reduce_mean) of an UNCALIBRATED strategy for a model that emits every column: per component a list of
    (source, transform, weight).  Branch order of score_image:571-708."""
    s = strategy
    rel = lambda src: (src, "rel_mean", 1.0)      # noqa: E731
    if "combo" in s:
        comps = [[("entropy", "scalar", opt_params[0]), ("albox", "rel_mean", opt_params[1])]]
    elif "alluncert" in s or "sota" in s:
        comps = [[rel("mcbox")], [rel("albox")], [("mcclass", "mean", 1.0)]]
    elif "epuncert" in s:
        comps = [[rel("mcbox")], [("mcclass", "mean", 1.0)]]
    elif "ental" in s:
        comps = [[rel("albox")], [("entropy", "scalar", 1.0)]]
    else:
        key = ("uncalib_" if ("box" in s or "class" in s) else "") + s.split("_")[-1]
        table = {"entropy": "entropy", "uncalib_albox": "albox", "uncalib_mcbox": "mcbox", "uncalib_mcclass": "mcclass"}
        if key in table:
            src = table[key]
            tr = "scalar" if src == "entropy" else ("rel_mean" if ("box" in s and "norm" in s) else "mean")
            comps = [[(src, tr, 1.0)]]
        else:
            comps = [[("det_score", "scalar", 1.0)]]
    return comps, "mean" in s


def combine_of(strategy, n_comp):
    if n_comp == 1:
        return None
    return "highep_lowal" if "highep_lowal" in strategy else ("sota" if "sota" in strategy else "sum")


def _term(cols, i, r, src, tr):
    if src == "entropy":
        return float(cols["entropy"][i][r])
    if src == "det_score":
        return float(cols["scores"][i][r])
    vals = [float(v) for v in np.ravel(cols[src][i][r])]
    if tr == "rel_mean":
        return np.mean(relativize_uncert([[float(v) for v in cols["boxes"][i][r][:4]]], [vals]))
    return np.mean(vals)


def score_columns(cols, components, reduce_mean, min_score, num_classes):
    """-> components [n, n_comp] float64 (0: nothing kept), count [n] int32, class_counts [n, num_classes] int32."""
    scores = np.asarray(cols["scores"])
    n = scores.shape[0]
    out = np.zeros((n, len(components)), np.float64)
    count = np.zeros((n,), np.int32)
    cls = np.zeros((n, num_classes), np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            kept = np.where(scores[i] > min_score)[0]
            count[i] = len(kept)
            for r in kept:
                cls[i, int(cols["classes"][i][r]) - 1] += 1
            if not len(kept):
                continue
            for k, comp in enumerate(components):
                per_det = []
                for r in kept:
                    v = comp[0][2] * _term(cols, i, r, comp[0][0], comp[0][1])      # (a weight of 1.0 changes nothing)
                    if len(comp) > 1:
                        v = v + comp[1][2] * _term(cols, i, r, comp[1][0], comp[1][1])
                    per_det.append(v)
                out[i, k] = np.mean(per_det) if reduce_mean else np.max(per_det)
    return out, count, cls


def combine(components, how):
    """active_learning_loop.py:733-764 on the kept images' columns [K, n_comp]."""
    comp = np.asarray(components, np.float64)
    if how is None:
        return comp[:, 0]
    mm = lambda d: [(x - min(d)) / (max(d) - min(d)) for x in d]           # noqa: E731
    if how == "highep_lowal":
        sc = np.asarray([mm(comp[:, i]) for i in range(comp.shape[1])])
        return np.sum([sc[i] for i in [0, 2]], axis=0) - sc[1]
    if how == "sota":
        return np.max([(comp[:, i] - np.mean(comp[:, i])) / np.std(comp[:, i]) for i in range(comp.shape[1])], axis=0)
    return np.sum([mm(comp[:, i]) for i in range(comp.shape[1])], axis=0)


def class_weighted(scores, class_counts):
    """The `perc` weighting of select_images:774-801 from per-image class counts."""
    cc = np.asarray(class_counts)
    pred_classes = [np.repeat(np.arange(1, cc.shape[1] + 1), row).astype(np.float64) for row in cc]
    class_names = np.unique(np.concatenate(pred_classes))
    n_ideal_classes = np.arange(np.max(class_names)) + 1
    class_distribution = [sum(np.concatenate(pred_classes) == c) for c in class_names]
    weights = np.asarray([sum(class_distribution) / class_distribution[i] for i in range(len(class_names))])
    weights = np.insert(weights, [int(i - 1) for i in n_ideal_classes if i not in class_names], 0)
    per_image = [np.mean([weights[int(np.unique(im)[i] - 1)] for i in range(len(np.unique(im)))]) for im in pred_classes]
    return np.multiply(per_image, scores)


def select(scores, names, class_counts, strategy, num_per_iter, im_names):
    """select_images:767-840; names[i] belongs to scores[i]."""
    per_image = class_weighted(scores, class_counts) if "perc" in strategy else np.asarray(scores)
    names = np.asarray(names)
    if "nee" in strategy:
        n = 5
        bs, rem = num_per_iter // n, num_per_iter % n
        sel = []
        bins = np.array_split(np.argsort(per_image), n)
        for i in range(n - 1):
            sel.extend(bins[i][-bs:])
        sel.extend(bins[-1][: bs + rem])
        chosen = [x.split(".")[0] for x in names[sel]]
    else:
        order = [x.split(".")[0] for _, x in sorted(zip(per_image, names), key=lambda p: p[0])]
        chosen = order[:num_per_iter] if "bottomk" in strategy else order[-num_per_iter:]
    return [i for i, item in enumerate(im_names) if item.split(".")[0] in chosen]
