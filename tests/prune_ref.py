"""Plain-numpy mirror of the pruning step (reference src/active_learning_loop.py:198-316), written from the reference's text
and pinned to it by tests/golden/prune_golden.npz (tests/test_prune_host.py).  It builds the N x N distance matrix the way the
reference does - that is the point of a mirror - in uint16, so keep N in the low thousands."""
import numpy as np


def distance_matrix(words):
    """words uint64 [N, W] -> d [N, N] uint16, d[i, j] = differing bits (ImageHash.__sub__)."""
    words = np.asarray(words, np.uint64).reshape(len(words), -1)
    n = words.shape[0]
    d = np.zeros((n, n), np.uint16)
    for w in range(words.shape[1]):
        col = words[:, w]
        d += np.bitwise_count(col[:, None] ^ col[None, :]).astype(np.uint16)
    return d


def limit_of(max_dist, prune_thr=None, max_distance=None):
    """The right-hand side of :267: an integer times a Python float, in float64; or an absolute number of bits."""
    return float(max_distance) if max_distance is not None else int(max_dist) * float(prune_thr)


def neighbours(words, prune_thr=None, max_distance=None):
    """(max_dist, row_off int64 [N + 1], idx int32 [total]): row i = np.where(d[i] <= limit)[0]."""
    d = distance_matrix(words)
    max_dist = int(d.max())
    rows = [np.where(d[i] <= limit_of(max_dist, prune_thr, max_distance))[0] for i in range(d.shape[0])]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([r.size for r in rows])
    return max_dist, off, np.concatenate(rows).astype(np.int32)


def neighbours_blocked(words, prune_thr=None, max_distance=None, block=512):
    """The same for a large N, a block of rows at a time (two passes: the maximum, then the rows); W = 1 only."""
    col = np.asarray(words, np.uint64).reshape(-1)
    n = col.size
    max_dist = max(int(np.bitwise_count(col[i:i + block, None] ^ col[None, :]).max()) for i in range(0, n, block))
    lim = limit_of(max_dist, prune_thr, max_distance)
    rows = []
    for i in range(0, n, block):
        d = np.bitwise_count(col[i:i + block, None] ^ col[None, :])
        rows.extend(np.where(r <= lim)[0] for r in d)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([r.size for r in rows])
    return max_dist, off, np.concatenate(rows).astype(np.int32)


def groups_of(off, idx):
    return [np.asarray(idx[off[i]:off[i + 1]], np.int64) for i in range(off.size - 1) if off[i + 1] - off[i] > 1]


def kept_from_groups(groups, n, rng):
    """:281-294 with the reference's own expressions; no group keeps everything (the reference raises there)."""
    rep = [rng.choice(groups[i]) for i in range(len(groups))]
    if not groups:
        return np.arange(n)
    removed = np.unique(np.concatenate([groups[i][groups[i] != rep[i]] for i in range(len(groups))]))
    return np.asarray([i for i in np.arange(n) if i not in removed])


def adjust_budget(budget, n_before, n_after, full_prune):
    if full_prune:
        return [100]
    new = np.asarray(budget) * n_before / n_after
    return new[new.cumsum() <= 100]


def prune_pool(strategy, words, available, budget, prune_thr, rng):
    """extract_hash_matrix: (available_indices, iteration_budget, kept_inds)."""
    n = len(available)
    if "rand" in strategy:
        kept = rng.choice(np.arange(n), size=int((1 - prune_thr) * n), replace=False)
    else:
        _, off, idx = neighbours(words, prune_thr)
        kept = kept_from_groups(groups_of(off, idx), n, rng)
    avail = [available[i] for i in kept]
    return avail, adjust_budget(budget, n, len(avail), "full_prune" in strategy), kept
