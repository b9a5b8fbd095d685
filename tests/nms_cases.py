"""Shared NMS test inputs (no GPU, no library import): boxes and scores at the edges of NonMaxSuppressionV5.

`make(kind, n, seed)` returns float32 `(boxes [n, 4], scores [n])`, deterministically (seeded `default_rng`).  Box
coordinates are finite in every kind; only scores take NaN / +-inf (kind `special_scores`).  `PARAM_SETS` is the one list
of (max_out, iou_thresh, score_thresh, soft_sigma) the host and the device tests run every kind under.

Kinds:
  plain             centre +- wh / 2 with wh in [4, 120], uniform scores: the control (`plain_boxes`, the generator the
                    older NMS tests use)
  inverted          half the boxes have y0 / y2 swapped and, independently, half have x1 / x3 swapped
  zero_area         ~30 % flat in y (y2 = y0), ~20 % flat in x (x3 = x1), a few single points; flat boxes hold the top scores
  grid              integer boxes [y, x, y + 1, x + w], w in {2, 3}, x in 0..11, y in 0..2: IoUs exactly 0, 1/3, 1/2, 1, boxes
                    that touch edge to edge, scores from {1/8 .. 8/8} (massive ties)
  nested_identical  clusters of identical boxes and boxes strictly inside one another
  negative          plain boxes, scores uniform in [-1, 0.2]
  special_scores    plain boxes; 10 % NaN (both signs), 10 % -inf, 10 % -0.0, 10 % +0.0 and (with_inf) three +inf scores
"""
import numpy as np

KINDS = ("plain", "inverted", "zero_area", "grid", "nested_identical", "negative", "special_scores")

NEG_INF = float("-inf")
THIRD = float(np.float32(1.0) / np.float32(3.0))       # the float32 quotient the grid's IoU 1/3 evaluates to

# (max_out, iou_thresh, score_thresh, soft_sigma)
PARAM_SETS = (
    (100, 0.5, 0.001, 0.25),
    (128, 0.5, NEG_INF, 0.0),
    (1, 0.5, NEG_INF, 0.25),
    (65, THIRD, -0.5, 0.0),
    (64, 0.5, -2.0, 0.15),
    (63, 0.5, 0.001, 0.25),
    (100, 0.0, NEG_INF, 0.0),
    (100, -1.0, NEG_INF, 0.0),
    (100, 1.0, 0.25, 0.0),
    (100, 0.5, 0.5, 0.0),
    (128, 0.5, NEG_INF, 0.25),       # soft with every finite score live (the table above this line is the issue's)
    (2, THIRD, NEG_INF, 0.0),
)


def is_soft(ps):
    return ps[3] > 0.0


def takes_inf(ps):
    """Parameter sets `special_scores` is run under WITH its three +inf scores: the soft sigma = 0.25 sets (a weight is
    at least exp(-2), inf stays inf) and every hard set (a weight is exactly 1, or the candidate is dropped before its
    inf * 0 is looked at).  Under the remaining set (soft, sigma = 0.15) the kind is generated without +inf."""
    return ps[3] == 0.25 or ps[3] == 0.0


def grows(ps, scores):
    """Soft NMS with a negative threshold over a live negative score: a weight below 1 moves that score UP, the regime in
    which a cached exact score is no upper bound.  (-0.0 is not below 0: it never changes.)"""
    s = np.asarray(scores, np.float32)
    with np.errstate(invalid="ignore"):
        return bool(is_soft(ps) and ps[2] < 0.0 and np.any((s < 0) & (s > np.float32(ps[2]))))


def plain_boxes(rng, n, span=400.0, tied=False):
    c = rng.uniform(0, span, (n, 2))
    wh = rng.uniform(4, 120, (n, 2))
    b = np.stack([c[:, 0] - wh[:, 0] / 2, c[:, 1] - wh[:, 1] / 2, c[:, 0] + wh[:, 0] / 2,
                  c[:, 1] + wh[:, 1] / 2], 1).astype(np.float32)
    if tied:
        s = (0.01 + rng.normal(0, 1e-4, n)).astype(np.float32)
        s[rng.integers(0, n, n // 8)] = s[0]            # exact ties -> index tie-break
    else:
        s = rng.uniform(0, 1, n).astype(np.float32)
    return b, s


def _span(n):
    """Side of the square the boxes are thrown into: grows with n so that a few hundred selections stay possible while
    every candidate still overlaps some neighbours."""
    return 400.0 * max(1.0, np.sqrt(n / 1500.0))


def make(kind, n, seed=0, with_inf=True):
    rng = np.random.default_rng([KINDS.index(kind), n, seed])
    if kind == "plain":
        return plain_boxes(rng, n, _span(n))
    if kind == "inverted":
        b, s = plain_boxes(rng, n, _span(n))
        fy, fx = rng.random(n) < 0.5, rng.random(n) < 0.5
        b[fy] = b[fy][:, [2, 1, 0, 3]]
        b[fx] = b[fx][:, [0, 3, 2, 1]]
        return b, s
    if kind == "zero_area":
        b, s = plain_boxes(rng, n, _span(n))
        u = rng.random(n)
        flat_y, flat_x, point = u < 0.3, (u >= 0.3) & (u < 0.5), (u >= 0.5) & (u < 0.53)
        b[flat_y, 2] = b[flat_y, 0]
        b[flat_x, 3] = b[flat_x, 1]
        b[point, 2] = b[point, 0]
        b[point, 3] = b[point, 1]
        flat = np.nonzero(flat_y | flat_x | point)[0]
        top = flat[: max(1, len(flat) // 4)] if len(flat) else np.arange(min(n, 1))
        if len(flat) == 0:                              # (n = 1, 2 ...: make the first box flat)
            b[0, 2] = b[0, 0]
        s[top] = (1.0 + rng.random(len(top))).astype(np.float32)      # above every other score
        return b, s
    if kind == "grid":
        y = rng.integers(0, 3, n)
        x = rng.integers(0, 12, n)
        w = rng.integers(2, 4, n)
        b = np.stack([y, x, y + 1, x + w], 1).astype(np.float32)
        s = (rng.integers(1, 9, n) / 8.0).astype(np.float32)
        return b, s
    if kind == "nested_identical":
        m = max(1, n // 6)                              # cluster centres
        c = rng.uniform(0, _span(n), (m, 2))
        wh = rng.uniform(16, 120, (m, 2))
        own = rng.integers(0, m, n)
        shrink = rng.choice(np.array([1.0, 1.0, 1.0, 0.75, 0.5, 0.25]), n)[:, None]     # 1.0: identical to the cluster's box
        cc, hw = c[own], wh[own] * shrink / 2
        b = np.concatenate([cc - hw, cc + hw], 1).astype(np.float32)
        s = rng.uniform(0, 1, n).astype(np.float32)
        return b, s
    if kind == "negative":
        b, _ = plain_boxes(rng, n, _span(n))
        return b, rng.uniform(-1.0, 0.2, n).astype(np.float32)
    if kind == "special_scores":
        b, s = plain_boxes(rng, n, _span(n))
        s = (s - np.float32(0.3)).astype(np.float32)   # finite scores on both sides of zero
        u = rng.random(n)
        s[u < 0.05] = np.float32(np.nan)
        s[(u >= 0.05) & (u < 0.1)] = -np.float32(np.nan)
        s[(u >= 0.1) & (u < 0.2)] = -np.inf
        s[(u >= 0.2) & (u < 0.3)] = -0.0
        s[(u >= 0.3) & (u < 0.4)] = 0.0
        if with_inf and n >= 4:
            s[rng.choice(n, 3, replace=False)] = np.inf
        if n < 4:                                        # tiny problems: one of each that fits, zeros first
            s[:] = np.array([-0.0, 0.0, np.nan], np.float32)[:n]
        return b, s
    raise ValueError("unknown kind %r" % (kind,))


def make_for(kind, n, ps, seed=0):
    """The inputs of `kind` as they are run under parameter set `ps`."""
    return make(kind, n, seed, with_inf=takes_inf(ps))


def half_below(scores, ps, seed=0):
    """A copy of `scores` with half of the candidates moved to or below the set's score threshold (exactly at it, and
    one float below); under a -inf threshold they become -inf."""
    s = np.array(scores, np.float32)
    rng = np.random.default_rng([len(s), seed, 77])
    pick = rng.random(len(s)) < 0.5
    thr = np.float32(ps[2])
    low = np.where(rng.random(len(s)) < 0.5, thr, np.nextafter(thr, np.float32(-np.inf), dtype=np.float32))
    s[pick] = low[pick]
    return s


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def sparse_boxes(n, seed=0):
    """The control of the score-prefix tests: boxes on a lattice of pitch 200 with sides below 120 - no two overlap, so
    NMS selects the top scores unchanged - and distinct scores in (0.01, 1)."""
    rng = np.random.default_rng([n, seed, 4242])
    side = int(np.ceil(np.sqrt(n)))
    cell = rng.permutation(side * side)[:n]
    c = np.stack([cell // side, cell % side], 1) * 200.0 + rng.uniform(-20, 20, (n, 2))
    wh = rng.uniform(4, 120, (n, 2))
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    s = (0.01 + 0.99 * (rng.permutation(n) + 0.5) / n).astype(np.float32)
    return b, s
