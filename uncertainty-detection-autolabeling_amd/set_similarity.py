"""The set-similarity analysis of the reference's active-learning evaluation (src/active_learning_eval.py:458-583
`emp_KL_divergence`, `empirical_jensen_shannon_divergence`; :946-1029 `Similarity.calculate_set_similarity`) with its neighbour
search on the device.

"How close is the set an AL method selected to the validation set", per class: a Gaussian KDE of each set's crop metrics in log
space, `num_samples` resampled points per set, the Perez-Cruz (2008) KL estimator from nearest-neighbour distances, JSD =
(KL(P||M) + KL(Q||M)) / 2.  The reference builds four KD-trees per (class, method) and walks the table one pair at a time; here
every nearest-neighbour search of a table is one problem of ONE device call (C entry point uda_nn_dist2_np: brute-force
all-pairs minimum of squared distances in float64, exact).  KDE, resampling, roots, logarithms and sums stay on the host.

  nn_dist2                             squared nearest-neighbour distances of many (queries, refs) problems, on the device
  emp_kl_divergence(s)                 the estimator (:489-491) for one pair / many pairs in one call
  resample_sets                        log transform, filter, KDE and the three resampled sets of a (P, Q) pair (:498-531)
  jensen_shannon_from_samples          two KLs per (P, Q, M) triple, all in one call
  empirical_jensen_shannon_divergence  the reference's function
  jensen_shannon_divergences           the same for many pairs: all resampling first, then one call
  calculate_set_similarity             the reference's table, ratios, weights and sort (:946-1029)

One deviation: the reference asks its KD-trees for eps=0.01 - any neighbour within a factor 1.01 of the nearest may
be returned - where this search is exact; |KL| moves by at most D * ln 1.01.  `collect_metrics`, the plots and `similarity_vs_*`
are not built.  scipy (gaussian_kde) is imported where it is used, as dataset_pruning.phash does.
"""
import numpy as np

from . import capi

MAX_D = capi.KNN_MAX_D
RANDOM_STATE_SEED = 42


def _points(a, what):
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("%s must be points [n, D], got shape %s" % (what, a.shape))
    a = np.ascontiguousarray(a, np.float64)
    if a.shape[0] < 1:
        raise ValueError("%s is an empty set" % what)
    if not np.isfinite(a).all():
        raise ValueError("%s holds values that are not finite" % what)
    return a


def _problems(problems):
    """[(queries, refs or None)] -> [(queries float64 [n, D], refs float64 [m, D] or None)], one D for all, checked."""
    out = []
    for k, (q, r) in enumerate(problems):
        q = _points(q, "queries of problem %d" % k)
        r = None if r is None else _points(r, "refs of problem %d" % k)
        if r is not None and r.shape[1] != q.shape[1]:
            raise ValueError("Both sample sets must have the same number of dimensions.")
        out.append((q, r))
    if not out:
        return out
    d = out[0][0].shape[1]
    if any(q.shape[1] != d for q, _ in out):
        raise ValueError("the problems of one call share one dimension, got %s" % sorted({q.shape[1] for q, _ in out}))
    if not 1 <= d <= MAX_D:
        raise ValueError("points of %d dimensions: 1..%d are taken" % (d, MAX_D))
    return out


def nn_dist2(problems, device=0):
    """For every problem (queries [n, D], refs [m, D]) the squared Euclidean distance from each query to its nearest reference,
    float64 [n], all problems in one device call.  refs=None is the set against itself: a point's own row is left out (an exact
    copy elsewhere is not), and a set of one point gives +inf.  Exact: ((x0-y0)^2 + (x1-y1)^2) + ..., each operation rounded on
    its own, then the minimum - whatever the device does with the order."""
    probs = _problems(problems)
    if not probs:
        return []
    if len(probs) > capi.KNN_MAX_B:
        raise ValueError("%d problems in one call, at most %d" % (len(probs), capi.KNN_MAX_B))
    d = probs[0][0].shape[1]
    q_off = np.zeros(len(probs) + 1, np.int64)
    r_off = np.zeros(len(probs) + 1, np.int64)
    q_off[1:] = np.cumsum([q.shape[0] for q, _ in probs])
    r_off[1:] = np.cumsum([(q if r is None else r).shape[0] for q, r in probs])
    queries = np.concatenate([q for q, _ in probs])
    refs = np.concatenate([q if r is None else r for q, r in probs])
    self = np.array([r is None for _, r in probs], np.uint8)
    out = np.empty(int(q_off[-1]), np.float64)
    lib = capi.load()
    rc = lib.uda_nn_dist2_np(int(device), d, len(probs), queries.ctypes.data, q_off.ctypes.data, refs.ctypes.data, r_off.ctypes.data,
                             self.ctypes.data, out.ctypes.data)
    capi.check(lib, None, rc, "uda_nn_dist2_np")
    return [out[a:b] for a, b in zip(q_off[:-1], q_off[1:])]


def _search(nn, device):
    return (lambda problems: nn_dist2(problems, device)) if nn is None else nn


def _kl_from_d2(d2_p, d2_q, n, m, d):
    """:489-491 - Eq. 14 of Perez-Cruz with the sign fixed - from the squared distances."""
    dp, dq = np.sqrt(d2_p), np.sqrt(d2_q)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.log(dp / dq).sum() * d / n + np.log(m / (n - 1))


def emp_kl_divergences(pairs, nn_dist2=None, device=0):
    """The estimated KL divergence of every (sample_p [n, D], sample_q [m, D]) pair, two problems per pair in one call: each
    point of P to its nearest OTHER point of P, and to its nearest point of Q.  A duplicate inside P gives +inf (or nan with a
    common point), a point common to P and Q -inf, as the reference's expression does."""
    pairs = [(np.asarray(p), np.asarray(q)) for p, q in pairs]
    for p, q in pairs:
        if p.ndim == 2 and q.ndim == 2 and p.shape[1] != q.shape[1]:
            raise ValueError("Both sample sets must have the same number of dimensions.")
    probs = _problems([pr for p, q in pairs for pr in ((p, None), (p, q))])
    d2 = _search(nn_dist2, device)(probs)
    return [_kl_from_d2(d2[2 * k], d2[2 * k + 1], probs[2 * k][0].shape[0], probs[2 * k + 1][1].shape[0], probs[2 * k][0].shape[1])
            for k in range(len(pairs))]


def emp_kl_divergence(sample_p, sample_q, nn_dist2=None, device=0):
    """KL(P || Q) estimated from samples, each row a sample (reference emp_KL_divergence)."""
    return emp_kl_divergences([(sample_p, sample_q)], nn_dist2, device)[0]


def resample_sets(P, Q, num_samples, seed=RANDOM_STATE_SEED):
    """The host half of the reference's JSD (:498-531): P [n, D], Q [m, D] -> the log transform, the boxes with a non-finite
    logarithm dropped, a Gaussian KDE per set, `num_samples` points drawn from each with the same seed, a third KDE on both
    draws together for the midpoint M, and back through exp.  Returns (samples_p, samples_q, samples_m), each [num_samples, D]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        log_p, log_q = np.log(np.asarray(P).T), np.log(np.asarray(Q).T)
    log_p = log_p[:, np.all(np.isfinite(log_p), axis=0)]
    log_q = log_q[:, np.all(np.isfinite(log_q), axis=0)]
    if log_p.size == 0 or log_q.size == 0:
        raise ValueError("Filtered data is empty, cannot proceed with KDE.")
    from scipy.stats import gaussian_kde
    draw_p = gaussian_kde(log_p).resample(size=num_samples, seed=seed)
    draw_q = gaussian_kde(log_q).resample(size=num_samples, seed=seed)
    draw_m = gaussian_kde(np.concatenate((draw_p, draw_q), axis=1)).resample(size=num_samples, seed=seed)
    return tuple(np.ascontiguousarray(np.exp(s).T) for s in (draw_p, draw_q, draw_m))


def jensen_shannon_from_samples(triples, nn_dist2=None, device=0):
    """(KL(P||M) + KL(Q||M)) / 2 for every (samples_p, samples_q, samples_m): four problems per triple, all in one call.
    Returns a list of (jsd, kl_pm, kl_qm)."""
    kl = emp_kl_divergences([pr for p, q, m in triples for pr in ((p, m), (q, m))], nn_dist2, device)
    return [(0.5 * (kl[2 * k] + kl[2 * k + 1]), kl[2 * k], kl[2 * k + 1]) for k in range(len(triples))]


def jensen_shannon_divergences(pairs, num_samples, seed=RANDOM_STATE_SEED, nn_dist2=None, device=0):
    """The JSD of every (P, Q) pair: all resampling on the host first, then one device call."""
    triples = [resample_sets(p, q, num_samples, seed) for p, q in pairs]
    return [j for j, _, _ in jensen_shannon_from_samples(triples, nn_dist2, device)]


def empirical_jensen_shannon_divergence(P, Q, num_samples, seed=RANDOM_STATE_SEED, nn_dist2=None, device=0):
    """Jensen-Shannon divergence between two samples P [n, D] and Q [m, D] of positive values (the reference's function)."""
    return jensen_shannon_divergences([(P, Q)], num_samples, seed, nn_dist2, device)[0]


def calculate_set_similarity(crops_metrics_perc, classes, methods, return_perclass=False, nn_dist2=None, num_samples=10000,
                             device=0):
    """The similarity of every AL method's set to the reference set (reference Similarity.calculate_set_similarity).
    crops_metrics_perc: one entry per set, the reference set LAST; entry[cl] holds the D metric rows of the class's crops, or
    nothing when the set has no box of it.  Returns (the (method, similarity) pairs in ascending order, whether the class
    weighting was activated, the per-class metrics [classes, methods] or None).  A method without boxes of a class counts nan
    there.  Every JSD of the table goes through one device call."""
    sets, val = crops_metrics_perc[:-1], crops_metrics_perc[-1]
    n_boxes = [[len(s[cl][0]) if len(s[cl]) > 0 else 0 for s in sets] for cl in classes]           # [classes][methods]
    cells = [(c, i) for c in range(len(classes)) for i in range(len(sets)) if len(sets[i][classes[c]]) > 0]
    pairs = [(np.asarray(sets[i][classes[c]]).T, np.asarray(val[classes[c]]).T) for c, i in cells]
    jsds = [[np.nan] * len(sets) for _ in classes]
    class_ratio = [[np.nan] * len(sets) for _ in classes]
    for (c, i), j in zip(cells, jensen_shannon_divergences(pairs, num_samples, nn_dist2=nn_dist2, device=device)):
        jsds[c][i] = j
        class_ratio[c][i] = len(val[classes[c]][0]) / n_boxes[c][i]
    total_dets = [np.sum([n_boxes[c][i] for c in range(len(classes))]) for i in range(len(sets))]
    class_weights = np.mean([n_boxes[c] / np.asarray(total_dets) for c in range(len(classes))], axis=-1)
    classes_low_dets = class_weights < np.percentile(class_weights, 25)
    class_weights = 1 / class_weights
    activate_class_weight = np.round(np.nanstd(class_weights) / np.nanmean(class_weights), 1) > 1.3
    if activate_class_weight:                                  # too much variation between the classes' shares
        class_weights[classes_low_dets] = 0
    else:
        class_weights = np.ones_like(class_weights)
    beta = np.maximum(1, np.asarray(total_dets / np.percentile(total_dets, 25), dtype="int"))
    combined = []
    for c in range(len(classes)):
        metrics = np.add(jsds[c], 0.25 * (class_ratio[c] * beta) + 0.5)
        metrics[np.isinf(metrics)] = np.nan
        combined.append(metrics)
    sim = np.nansum(1 / np.asarray(combined) * class_weights.reshape([-1, 1]), axis=0) / np.sum(class_weights)
    methods_sim = {methods[i]: sim[i] for i in range(len(methods))}
    return sorted(methods_sim.items(), key=lambda x: x[1]), activate_class_weight, combined if return_perclass else None
