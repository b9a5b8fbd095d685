"""Numpy mirror of the contract of uda_class_report_np (include/uda_hip.h): the tallies behind the classification calibration report
for ragged segments of rows, M probability tables and the C + 1 targets.  The bin id is the number of edges e with `!(x < e)`;
every float64 sum is the root of the zero-padded pairwise tree over the segment's rows (`tree`: b = b[0::2] + b[1::2]), the term of
a row outside the bin being +0.0; the NLL term is Keras's CategoricalCrossentropy() row term on probabilities in float64.  `report`
has the signature and the result of `class_report.report_np`, so it can stand in for the device wherever that module takes
`engine=`."""
import numpy as np

import tree_ref

EPS = 1e-7
tree = tree_ref.tree


def uniform_edges(n_bins=10):
    return np.linspace(0.0, 1.0 + 1e-8, n_bins + 1)


def bin_ids(x, edges):
    """The number of edges e with !(x < e): np.digitize for ascending edges, n_edges for a NaN."""
    return (~(np.asarray(x)[:, None] < np.asarray(edges)[None, :])).sum(axis=1)


def argmax_rule(p):
    """[n, C] -> per row the first index holding a NaN if there is one, else the first maximum."""
    nan = np.isnan(p)
    first_max = np.argmax(np.where(nan, -np.inf, p), axis=1)
    return np.where(nan.any(axis=1), np.argmax(nan, axis=1), first_max)


def nll_terms(p, label):
    """[n, C], [n] -> the row terms of nll_sum (0.0 for a row left out), the clipped mask, the left-out mask."""
    n, C = p.shape
    rowsum = np.zeros(n)
    for c in range(C):                                       # left to right, from 0.0
        rowsum = rowsum + p[:, c]
    out = ~np.isfinite(p).all(axis=1) | (rowsum == 0.0)
    q = p[np.arange(n), label] / np.where(out, 1.0, rowsum)
    clipped = ~out & ((q < EPS) | (q > 1.0 - EPS))
    qc = np.where(q < EPS, EPS, np.where(q > 1.0 - EPS, 1.0 - EPS, q))
    return np.where(out, 0.0, -np.log(np.where(out, 1.0, qc))), clipped, out


def _edge_rows(edges, B, M, C):
    """edges: None, one 1-D row, or a sequence of B * M * (C + 1) rows -> list of float64 rows."""
    if edges is None:
        return [uniform_edges()]
    if np.ndim(edges[0]) == 0:
        return [np.asarray(edges, np.float64)]
    return [np.asarray(e, np.float64) for e in edges]


def report(prob, label, segments=None, edges=None, device=0):
    prob = np.asarray(prob, np.float64)
    M, N, C = prob.shape
    label = np.asarray(label, np.int32).reshape(-1)
    off = np.asarray([0, N] if segments is None else segments, np.int64)
    B = len(off) - 1
    rows = _edge_rows(edges, B, M, C)
    G, E = len(rows), max(len(r) for r in rows)
    assert G in (1, B * M * (C + 1))
    ed = np.zeros((G, E))
    for g, r in enumerate(rows):
        ed[g, :len(r)] = r
    ne = np.array([len(r) for r in rows], np.int32)
    out = dict(bin_count=np.zeros((B, M, C + 1, E + 1), np.int64), bin_hits=np.zeros((B, M, C + 1, E + 1), np.int64),
               bin_sum=np.zeros((B, M, C + 1, E + 1)), brier_sum=np.zeros((B, M, C)), nll_sum=np.zeros((B, M)),
               tab_counts=np.zeros((B, M, 2), np.int64), off=off, edges=ed, n_edges=ne)
    with np.errstate(all="ignore"):
        for b in range(B):
            lab = label[off[b]:off[b + 1]]
            n = len(lab)
            for m in range(M):
                p = prob[m, off[b]:off[b + 1]]
                a = argmax_rule(p) if n else np.zeros(0, np.int64)
                for t in range(C + 1):
                    x = p[:, t] if t < C else p[np.arange(n), a]
                    y = (lab == t) if t < C else (lab == a)
                    e = rows[0] if G == 1 else rows[(b * M + m) * (C + 1) + t]
                    ids = bin_ids(x, e)
                    for k in range(len(e) + 1):
                        inside = ids == k
                        out["bin_count"][b, m, t, k] = np.count_nonzero(inside)
                        out["bin_hits"][b, m, t, k] = np.count_nonzero(inside & y)
                        out["bin_sum"][b, m, t, k] = tree(np.where(inside, x, 0.0))
                    if t < C:
                        d = x - np.where(y, 1.0, 0.0)
                        out["brier_sum"][b, m, t] = tree(d * d)
                terms, clipped, left = nll_terms(p, lab)
                out["nll_sum"][b, m] = tree(terms)
                out["tab_counts"][b, m] = [np.count_nonzero(clipped), np.count_nonzero(left)]
    return out


def nll_abs_terms(p, label):
    """Sum |term| of nll_sum over one segment and table (the terms are -log q, so this is also sum |log q|)."""
    with np.errstate(all="ignore"):
        return np.abs(nll_terms(np.asarray(p, np.float64), np.asarray(label, np.int32))[0]).sum()
