"""Plain-numpy mirror of the neighbour search of the set-similarity analysis (reference src/active_learning_eval.py:481-487:
four KD-tree queries per emp_KL_divergence) and of the estimator built on it (:489-491), pinned to the reference by
tests/golden/similarity_golden.npz (tests/test_similarity_host.py).

The squared distance is summed coordinate by coordinate in ascending order, every operation rounded on its own, the minimum is
taken over it, and the root is taken last.  For D <= 5 that is scipy's cKDTree queried with eps=0 bit for bit (for D = 8 scipy
unrolls the sum by four and differs by one ulp).  Rows go through in blocks, so nothing larger than block x m is ever held."""
import numpy as np


def dist2(queries, refs, self=False, block=512):
    """queries [n, D], refs [m, D] float64 -> d2 [n]: the smallest ((x0-y0)^2 + (x1-y1)^2) + ... over the references; with
    `self`, reference row j == query row i is left out (+inf when there is no other row)."""
    q = np.ascontiguousarray(queries, np.float64).reshape(len(queries), -1)
    r = np.ascontiguousarray(refs, np.float64).reshape(len(refs), -1)
    out = np.empty(q.shape[0], np.float64)
    with np.errstate(over="ignore"):
        for i in range(0, q.shape[0], block):
            rows = q[i:i + block]
            e = rows[:, None, 0] - r[None, :, 0]
            d = e * e
            for k in range(1, q.shape[1]):
                e = rows[:, None, k] - r[None, :, k]
                d = d + e * e
            if self:
                own = np.arange(i, i + rows.shape[0])
                inside = own < r.shape[0]
                d[np.flatnonzero(inside), own[inside]] = np.inf
            out[i:i + block] = d.min(axis=1)
    return out


def nn_dist2(problems):
    """The package's `nn_dist2=` hook on the mirror: a list of (queries, refs or None) -> a list of d2 arrays."""
    return [dist2(q, q if r is None else r, self=r is None) for q, r in problems]


def emp_kl(sample_p, sample_q):
    """emp_KL_divergence on the mirror (:489-491, the reference's own expression)."""
    n, d = sample_p.shape
    m = sample_q.shape[0]
    dp = np.sqrt(dist2(sample_p, sample_p, self=True))
    dq = np.sqrt(dist2(sample_p, sample_q))
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.log(dp / dq).sum() * d / n + np.log(m / (n - 1))
