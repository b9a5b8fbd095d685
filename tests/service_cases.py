"""Shared inputs of the evaluation-service edge tests (no GPU, no library import): seeded cases that put the scoring, matching
and thresholding kernels on their wave (64), block (128 / 256), tile (2048) and cap (4096 rows, 8192 classes, 16384 ground-truth
rows) boundaries.  test_service_cases_host.py checks the cases and their expected values on the CPU, test_gpu_service_edges.py
runs them through the device.

Every case is a function of (name, seed) and returns the inputs of one handle-free entry point as a dict; all values are finite.
`expected_*` applies the suite's numpy mirror (validate_ref, score_ref, pseudo_ref, coco_ref, thr_ref) once per case and keeps
the result, so the host and the device tests of one session share it.

  assign   utils_extra.assign_gt_boxes      M in ASSIGN_M at G = 9, G in ASSIGN_G at M = 65, `ident` (a block of identical boxes
                                            across ranks 63/64 and 127/128), `mse_tie` (two boxes 8 away on either side)
  score    active_learning.score_detections M, C, mcclass width from SCORE_SHAPES, max and mean; per case up to five images:
                                            everything kept with the largest value in wave 0 / wave 3 / the second stride, kept
                                            rows in wave 3 only, kept rows in the second stride only
  pseudo   pseudo_labels.select_detections  258 images of 2 rows; one image of 4096 rows under max_rows 99 and 4096
  coco     coco_metric.match_np             single-class images of 127 .. 300 rows, tied scores, exact area ends, crowds at
                                            orders 0 / 31 / 32 / 255, equal IoUs, odd class values, C = 8192, M = 4096
  thr      thresholding.roc_objective       N = 2047 / 2048 / 2049, 512 / 513 distinct scores, U = 4, G = 8192
"""
import functools
import zlib

import numpy as np

F32 = np.float32


def checksum(*arrays):
    """CRC-32 over dtype, shape and bytes of every array: what the fixture stores of a case's inputs."""
    crc = 0
    for a in arrays:
        a = np.ascontiguousarray(a)
        crc = zlib.crc32(("%s%s" % (a.dtype.str, a.shape)).encode(), crc)
        crc = zlib.crc32(a.tobytes(), crc)
    return np.uint32(crc)


def _rng(kind, name, seed):
    return np.random.default_rng([zlib.crc32(("%s/%s" % (kind, name)).encode()), seed])


# ------------------------------------------------------------------------------------------------ assign
ASSIGN_M = (0, 1, 63, 64, 65, 129, 4095, 4096)          # at G = 9
ASSIGN_G = (1, 4, 5, 257, 16384)                        # at M = 65
ASSIGN_CASES = tuple("m%d" % m for m in ASSIGN_M) + tuple("g%d" % g for g in ASSIGN_G) + ("ident", "mse_tie")
ASSIGN_METHODS = ("IoU", "MSE", "rank")
ASSIGN_KEEPS = ("validate", "calibrate")
GT_KINDS = ("last", "mid", "row0", "far", "degenerate", "k64", "jitter", "copy", "jitter")     # by ground-truth row % 9
IDENT_BLOCKS = ((60, 132), (70, 141))                   # rows [lo, hi) of image 0 / 1 that carry one box
MSE_TIES = (((67, 131), (100, 101)), ((30, 158), (63, 64)))     # per image, per ground-truth row: (rank of gt - 8, rank of gt + 8)
TIE_GT = np.array([[100, 200, 300, 400], [400, 100, 500, 300]], F32)


def _dets(rng, M, valid, lo=60.0):
    """[M, 4] float32 y1 x1 y2 x2 inside [0, 1500]; rows >= valid carry row 0's box, as the post-process pads."""
    c = rng.uniform(lo, 1440, (M, 2))
    hw = rng.uniform(6, 400 if lo < 100 else 200, (M, 2))
    b = np.clip(np.column_stack([c[:, 0] - hw[:, 0] / 2, c[:, 1] - hw[:, 1] / 2, c[:, 0] + hw[:, 0] / 2, c[:, 1] + hw[:, 1] / 2]),
                0, 1500).astype(F32)
    if M and valid < M:
        b[valid:] = b[0]
    return b


def _gt_row(rng, dets, valid, kind):
    if kind == "far" or valid == 0:
        y, x = rng.uniform(1700, 1900, 2)
        return np.array([y, x, y + rng.uniform(5, 100), x + rng.uniform(5, 100)], F32)
    if kind == "degenerate":                            # zero area: a line or a point
        y, x = rng.uniform(100, 1400, 2)
        return np.array([y, x, y, x + (rng.uniform(5, 80) if rng.random() < 0.5 else 0)], F32)
    if kind == "row0":
        return dets[0].copy()
    k = {"last": valid - 1, "mid": valid // 2, "k64": min(64, valid - 1)}.get(kind)
    if k is None:
        k = int(rng.integers(0, valid))
    if kind == "copy":
        return dets[k].copy()
    return (dets[k] + rng.normal(0, 2, 4)).astype(F32)


def _real_rows(rng, G):
    """The ground-truth rows that carry a box: all of them up to G = 257, about 260 of 16384 (the ends among them)."""
    if G <= 257:
        return np.arange(G)
    return np.unique(np.r_[np.arange(9), G - 2, G - 1, rng.integers(0, G, 250)])


def assign_case(name, seed=0):
    """-> dict(dets [2, M, 4], gt_boxes [2, G, 4], gt_classes [2, G]) float32.  Image 0 has M valid rows, image 1 two thirds of
    them (the rest padded with row 0's box).  Row i % 9 == 6 has class 0 (kept by calibrate only), i % 9 == 8 is padding."""
    rng = _rng("assign", name, seed)
    n = 2
    if name in ("ident", "mse_tie"):
        M, G = 200, 6 if name == "ident" else 4
    else:
        M, G = (int(name[1:]), 9) if name[0] == "m" else (65, int(name[1:]))
    valid = [M, max(1, 2 * M // 3) if M else 0]
    dets = np.stack([_dets(rng, M, v, 700.0 if name == "mse_tie" else 60.0) for v in valid]) if M else np.zeros((n, 0, 4), F32)
    gb = np.full((n, G, 4), -1, F32)
    gc = np.full((n, G), -1, F32)
    if name == "ident":
        for im, (lo, hi) in enumerate(IDENT_BLOCKS):
            valid[im] = M
            dets[im] = _dets(rng, M, M)
            dets[im, lo:hi] = dets[im, lo]
            box = dets[im, lo]
            gb[im, :5] = [box, box + rng.normal(0, 0.5, 4).astype(F32), _gt_row(rng, dets[im], M, "far"), dets[im, 0], box]
            gc[im, :5] = [3, 1, 2, 5, 0]
        return dict(dets=dets, gt_boxes=gb, gt_classes=gc)
    if name == "mse_tie":
        for im in range(n):
            dets[im] = _dets(rng, M, M, 700.0)
            for row, (minus, plus) in enumerate(MSE_TIES[im]):
                off = np.zeros(4, F32)
                off[(im + row) % 4] = 8
                dets[im, minus], dets[im, plus] = TIE_GT[row] - off, TIE_GT[row] + off
            gb[im, :2], gc[im, :2] = TIE_GT, [2, 4]
            gb[im, 2], gc[im, 2] = _gt_row(rng, dets[im], M, "jitter"), 1
        return dict(dets=dets, gt_boxes=gb, gt_classes=gc)
    for im in range(n):
        for i in _real_rows(rng, G):
            if i % 9 == 8:
                continue
            gb[im, i] = _gt_row(rng, dets[im], valid[im], GT_KINDS[i % 9])
            gc[im, i] = 0.0 if i % 9 == 6 else float(rng.integers(1, 8))
    return dict(dets=dets, gt_boxes=gb, gt_classes=gc)


@functools.lru_cache(maxsize=None)
def expected_assign(name, method, keep):
    """(idx, iou, count) of validate_ref.assign, or None where it raises ValueError (a kept row without a detection)."""
    import validate_ref as V
    c = assign_case(name)
    try:
        out = V.assign(method, c["gt_boxes"], c["gt_classes"], c["dets"], keep)
    except ValueError:
        return None
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ score
SCORE_SHAPES = ((1, 1, 1), (64, 8, 7), (65, 129, 8), (255, 8192, 9), (256, 8, 128), (257, 129, 7), (513, 8192, 9), (4096, 8, 128))
SCORE_CASES = tuple("%s_m%d" % (red, s[0]) for red in ("max", "mean") for s in SCORE_SHAPES)
SCORE_MIN = float(F32(0.25))
MAX_COMPONENTS = [[("mcbox", "rel_mean", 1.0)], [("albox", "rel_mean", 1.0)], [("mcclass", "mean", 1.0)]]
MEAN_COMPONENTS = [[("entropy", "scalar", 1.0)], [("albox", "mean", 1.0)], [("mcclass", "mean", 1.0)]]
TOP_ROWS = {"top_wave0": 5, "top_wave3": 200, "top_stride2": 300}
TOP_VALUES = (125.0, 125.0, 100.0)                       # the three components of a planted row: 1000 / 8, 1000 / 8, 100


def score_layout(M):
    """The images of a score case at M rows: (kind, kept rows lo, hi)."""
    out = [("top_wave0", 0, M)]
    if M > 200:
        out.append(("top_wave3", 0, M))
    if M > 300:
        out.append(("top_stride2", 0, M))
    if M > 192:
        out.append(("kept_wave3", 192, min(M, 256)))
    if M > 256:
        out.append(("kept_stride2", 256, min(M, 512)))
    return out


def score_case(name, seed=0):
    """-> dict(cols: float32 columns [n, M, ...], components, reduce_mean, min_score, num_classes, layout).  The float64 run
    takes the same values cast up.  Mean cases spread entropy and albox over 2^40 (all positive: any summation order stays
    within M * 2^-53 of the exact sum)."""
    red, M = name.split("_m")
    M = int(M)
    _, C, mcw = [s for s in SCORE_SHAPES if s[0] == M][0]
    rng = _rng("score", name, seed)
    layout = score_layout(M)
    n = len(layout)
    y1, x1 = rng.uniform(0, 500, (n, M)), rng.uniform(0, 500, (n, M))
    boxes = np.stack([y1, x1, y1 + rng.uniform(8, 120, (n, M)), x1 + rng.uniform(8, 120, (n, M))], -1).astype(F32)
    scores = rng.uniform(0.01, 0.2, (n, M)).astype(F32)
    classes = rng.integers(1, C + 1, (n, M)).astype(F32)
    scale = np.exp2(rng.integers(0, 41, (n, M))) if red == "mean" else np.ones((n, M))
    entropy = (rng.uniform(0.01, 2.0, (n, M)) * scale).astype(F32)
    albox = (rng.gamma(2.0, 1.0, (n, M, 4)) * scale[..., None]).astype(F32)
    mcbox = rng.gamma(2.0, 1.0, (n, M, 4)).astype(F32)
    mcclass = rng.gamma(2.0, 0.2, (n, M, mcw)).astype(F32)
    for i, (kind, lo, hi) in enumerate(layout):
        scores[i, lo:hi] = rng.uniform(0.3, 0.9, hi - lo).astype(F32)
        if kind == "top_wave0" and M > 8:                # a few rows under the threshold inside the list
            scores[i, rng.integers(1, M, max(1, M // 16))] = F32(0.1)
            scores[i, [min(5, M - 1), M - 1]] = F32(0.5)
        kept = np.nonzero(scores[i] > F32(SCORE_MIN))[0]
        classes[i, kept[0]], classes[i, kept[-1]] = 1, C
        if red == "max" and kind in TOP_ROWS:
            r = min(TOP_ROWS[kind], M - 1)
            boxes[i, r] = (64, 32, 72, 40)                # sides of exactly 8
            albox[i, r], mcbox[i, r], mcclass[i, r] = 1000, 1000, 100
    cols = dict(boxes=boxes, scores=scores, classes=classes, entropy=entropy, albox=albox, mcbox=mcbox, mcclass=mcclass)
    return dict(cols=cols, components=MAX_COMPONENTS if red == "max" else MEAN_COMPONENTS, reduce_mean=red == "mean",
                min_score=SCORE_MIN, num_classes=C, layout=layout)


def as64(cols):
    return {k: np.asarray(v, np.float64) for k, v in cols.items()}


@functools.lru_cache(maxsize=None)
def expected_score(name):
    import score_ref as S
    c = score_case(name)
    out = S.score_columns(as64(c["cols"]), c["components"], c["reduce_mean"], c["min_score"], c["num_classes"])
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ pseudo
PSEUDO_CASES = ("n258", "m4096_r99", "m4096_r4096")
PSEUDO_STRATEGY, PSEUDO_TAU, PSEUDO_MIN = "pseudoscore_alluncert", 0.5, 0.1


def pseudo_case(name, seed=0):
    """-> dict(cols float32, num_classes, max_rows, names).  n258: 258 images of M = 2 whose rows are candidates (score 0.8),
    kept only (0.3) or dropped (0.05) - every image has 0, 1 or 2 candidates, the images around 255 / 256 have some."""
    big = name != "n258"
    rng = _rng("pseudo", "m4096" if big else name, seed)
    n, M, C = (1, 4096, 4) if big else (258, 2, 4)
    if big:
        u = rng.random((n, M))
        scores = np.where(u < 0.5, rng.uniform(0.55, 0.99, (n, M)), np.where(u < 0.9, rng.uniform(0.11, 0.45, (n, M)), 0.05))
    else:
        level = rng.integers(0, 3, (n, M))
        level[[0, 255, 256, 257]] = [[2, 2], [0, 2], [2, 2], [2, 1]]
        level[[1, 254]] = [[0, 1], [1, 0]]
        scores = np.choose(level, [0.05, 0.3, 0.8]) + rng.uniform(0, 0.01, (n, M))
    y1, x1 = rng.uniform(0, 300, (n, M)), rng.uniform(0, 900, (n, M))
    cols = dict(boxes=np.stack([y1, x1, y1 + rng.uniform(2, 60, (n, M)), x1 + rng.uniform(2, 60, (n, M))], -1), scores=scores,
                classes=rng.integers(1, C + 1, (n, M)), entropy=rng.uniform(0.01, 2.0, (n, M)), albox=rng.gamma(2.0, 0.5, (n, M, 4)),
                mcbox=rng.gamma(2.0, 0.5, (n, M, 4)), mcclass=rng.gamma(2.0, 0.2, (n, M, C)))
    cols = {k: np.asarray(v, F32) for k, v in cols.items()}
    return dict(cols=cols, num_classes=C, max_rows={"n258": 99, "m4096_r99": 99, "m4096_r4096": 4096}[name],
                names=["im%03d.png" % i for i in range(n)])


@functools.lru_cache(maxsize=None)
def expected_pseudo(name):
    """(rows(...) of pseudo_ref, select(...) of pseudo_ref) on the float64 view of the case."""
    import pseudo_ref as R
    c = pseudo_case(name)
    cols = as64(c["cols"])
    comps, invert, gate, _ = R.components_of(PSEUDO_STRATEGY)
    rows = R.rows(cols, comps, invert, gate, PSEUDO_MIN, PSEUDO_TAU, c["max_rows"])
    return rows, R.select(cols, c["names"], PSEUDO_STRATEGY, PSEUDO_TAU, PSEUDO_MIN, max_rows=c["max_rows"])


# ------------------------------------------------------------------------------------------------ coco
# name: (M, G, T, detections per image) of the single-class cases; the crafted ones below.  The mirror walks detections x ground
# truth x thresholds x 4 areas in Python, so 256 ground-truth rows meet 32 thresholds with 28 detections only.
COCO_SINGLE = {"m127_g0_t1": (127, 0, 1, (127, 107)), "m128_g1_t32": (128, 1, 32, (128, 108)), "m129_g33_t32": (129, 33, 32, (129, 109)),
               "m300_g256_t1": (300, 256, 1, (300, 280)), "m300_g33_t1": (300, 33, 1, (300, 280)), "m32_g256_t32": (32, 256, 32, (28,))}
COCO_CASES = tuple(COCO_SINGLE) + ("area", "crowd", "equal_iou", "classes", "c8192", "m4096")
COCO_GOLDEN_CASES = tuple(c for c in COCO_CASES if c != "m4096")          # M <= 300: the reference runs them
STD_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
STD_PICK = (0, 5, 9)                                     # the standard thresholds the mirror is held to the fixture at
AREA_ENDS = (1024.0, 9216.0)
CROWD_ORDERS = (0, 31, 32, 255)
ODD_CLASSES = (2.5, 0.0, -0.5, 4.0)                      # at C = 3: inside class 2's range, unused by every class, C + 1


def coco_thrs(T):
    return {1: np.array([0.5]), 2: np.array([0.5, 0.75])}.get(T, np.linspace(0.2, 0.975, T))


def _gt(x, y, w, h, cls, crowd=0):
    return [y, x, y + h, x + w, crowd, -7.0, cls]        # the area column is not read


def _pad(rows, count, fill_cls=-1.0):
    out = np.zeros((count, 7), F32)
    out[:, 6] = fill_cls
    if len(rows):
        out[:len(rows)] = np.asarray(rows, F32)
    return out


def _random_image(rng, M, G, n_det, classes=(1,), far_gt=None):
    """G ground-truth rows (all real) on an integer grid and n_det detections, 70 % of them near a ground-truth box; scores on a
    grid of 0.01.  far_gt: the ground-truth row moved 3000 away, with detection row 0 an exact copy of it."""
    gts = []
    for _ in range(G):
        w, h = rng.integers(6, 140, 2)
        x, y = rng.integers(0, 500, 2)
        gts.append(_gt(x, y, w, h, int(rng.choice(classes))))
    if far_gt is not None:
        gts[far_gt][0] += 3000
        gts[far_gt][2] += 3000
    dets = []
    for k in range(n_det):
        if gts and rng.random() < 0.7:
            g = gts[int(rng.integers(0, len(gts)))]
            x, y = g[1] + rng.integers(-6, 7), g[0] + rng.integers(-6, 7)
            w, h = g[3] - g[1] + rng.integers(-4, 5), g[2] - g[0] + rng.integers(-4, 5)
            cls = g[6]
        else:
            w, h = rng.integers(4, 150, 2)
            x, y = rng.integers(0, 500, 2)
            cls = int(rng.choice(classes))
        if rng.random() < 0.3:
            x, y = x + rng.random(), y + rng.random()
        dets.append([-1, x, y, max(w, 1), max(h, 1), np.round(rng.random(), 2), cls])
    if far_gt is not None and dets:
        g = gts[far_gt]
        dets[0] = [-1, g[1], g[0], g[3] - g[1], g[2] - g[0], 1.0, g[6]]
    return _pad(gts, G), _pad(dets, M)


def _tie_scores(det, n_det):
    """Plants the ties of the single-class cases: the score of rank 99 is given to rows 127 and 128 and to two early rows (so
    that the tie crosses rank 99 / 100 and row 127 / 128), the top score to the last two rows (rows >= 128 of rank < 100)."""
    s = det[:n_det, 5]
    if n_det > 128:
        s[n_det - 2:] = 0.99
    if n_det > 100:
        cut = np.sort(s)[::-1][99]
        planted = [r for r in (3, 40, 127, 128) if r < n_det]
        s[planted] = cut
        for r in range(10, n_det):                       # (a planted row may have held a better score: refill the tie)
            if (s >= cut).sum() > 100:
                break
            if s[r] < cut and r not in planted:
                s[r] = cut


def coco_case(name, seed=0):
    """-> dict(det [n, M, 7] legacy rows, gt [n, G, 7], num_classes, thrs, plant: what the host test looks up)."""
    rng = _rng("coco", name, seed)
    plant = {}
    if name in COCO_SINGLE:
        M, G, T, per_image = COCO_SINGLE[name]
        far = 32 if G > 32 else (0 if G else None)       # detection row 0 copies this ground-truth row, which lies apart
        gts, dets = [], []
        for n_det in per_image:                          # (the last image ends in unused rows)
            gt, det = _random_image(rng, M, G, n_det, far_gt=far)
            _tie_scores(det, n_det)
            gts.append(gt), dets.append(det)
        plant["far_det_row"] = 0 if far is not None else None
        return dict(det=np.stack(dets), gt=np.stack(gts), num_classes=1, thrs=coco_thrs(T), plant=plant)
    if name == "area":
        # six ground-truth boxes whose float32 area is 1024, 9216 and one ulp either side of each; a detection on each of them
        # (matched: it takes the box's flag) and a detection of the same size far from everything (unmatched: its own area)
        gts, dets, areas = [], [], []
        for k, (side, step) in enumerate(((32, -1), (32, 0), (32, 1), (96, -1), (96, 0), (96, 1))):
            h = F32(side) if step == 0 else np.nextafter(F32(side), F32(side + step))
            areas.append(float(F32(side) * h))
            gts.append(_gt(200.0 * k, 0.0, side, h, 1))
            dets.append([-1, 200.0 * k, 0.0, side, h, 0.9 - 0.01 * k, 1])
            dets.append([-1, 200.0 * k, 2000.0, side, h, 0.5 - 0.01 * k, 1])
        plant["areas"] = areas
        return dict(det=_pad(dets, 16)[None], gt=_pad(gts, 8)[None], num_classes=1, thrs=coco_thrs(2), plant=plant)
    if name == "crowd":
        M, G = 64, 256
        gt, det = _random_image(rng, M, G, M)
        rows = []
        for k, g in enumerate(CROWD_ORDERS):
            x, y = 3000.0 + 300 * k, 3000.0
            gt[g] = _gt(x, y, 100, 100, 1, crowd=1)
            rows += [[-1, x + 5, y + 5, 30, 30, 0.95 - 0.01 * k, 1], [-1, x + 50, y + 50, 40, 40, 0.85 - 0.01 * k, 1]]
        det[:len(rows)] = np.asarray(rows, F32)
        plant["crowd_det_rows"] = list(range(len(rows)))
        return dict(det=det[None], gt=gt[None], num_classes=1, thrs=coco_thrs(2), plant=plant)
    if name == "equal_iou":
        # one box, two detections shifted 2 to either side (equal IoU 0.8182: the better score takes it, the other one misses);
        # one detection between two boxes at equal IoU 1/3 (the later row wins)
        gts = [_gt(100, 100, 40, 40, 1), _gt(300, 100, 10, 10, 1), _gt(310, 100, 10, 10, 1)]
        dets = [[-1, 102, 100, 40, 40, 0.8, 1], [-1, 98, 100, 40, 40, 0.7, 1], [-1, 305, 100, 10, 10, 0.6, 1]]
        return dict(det=_pad(dets, 8)[None], gt=_pad(gts, 4)[None], num_classes=1, thrs=np.array([0.3, 0.5, 0.8]), plant=plant)
    if name == "classes":
        gt, det = _random_image(rng, 24, 9, 16, classes=(1, 2, 3))
        det[16:16 + 4] = det[:4]
        det[16:20, 6] = ODD_CLASSES
        det[[1, 5], 6] = 2                               # (class 2 has rows of its own beside the 2.5)
        gt[:3, 6] = (1, 2, 3)
        return dict(det=det[None], gt=gt[None], num_classes=3, thrs=coco_thrs(2), plant=plant)
    if name == "c8192":
        gt, det = _random_image(rng, 12, 6, 12, classes=(1, 4096, 8192))
        gt[:3, 6] = (1, 4096, 8192)
        det[:3, 6] = (8192, 1, 4096)
        return dict(det=det[None], gt=gt[None], num_classes=8192, thrs=coco_thrs(2), plant=plant)
    if name == "m4096":
        gt, det = _random_image(rng, 4096, 256, 4000, classes=(1, 2))
        return dict(det=det[None], gt=gt[None], num_classes=2, thrs=coco_thrs(2), plant=plant)
    raise ValueError("unknown coco case %r" % (name,))


@functools.lru_cache(maxsize=None)
def expected_coco(name, std_thrs=False):
    """coco_ref.match at the case's thresholds, or at STD_THRS[STD_PICK] (a threshold's matching does not depend on the others)."""
    import coco_ref as R
    c = coco_case(name)
    out = R.match(c["det"], c["gt"], c["num_classes"], STD_THRS[list(STD_PICK)] if std_thrs else c["thrs"])
    for a in out:
        a.setflags(write=False)
    return out


def evaluated_rows(det, gt, num_classes):
    """Rows the reference evaluates: used rows of a class that has ground truth somewhere among the images with a used row."""
    used = det[:, :, 6] > -1
    imgs = used.any(1)
    cats = set(int(c) for c in gt[imgs][:, :, 6][gt[imgs][:, :, 6] > -1])
    cls = np.where(used, det[:, :, 6].astype(np.int32), -1)
    return used & imgs[:, None] & np.isin(cls, sorted(cats))


# ------------------------------------------------------------------------------------------------ thr
THR_CASES = ("n2047", "n2048", "n2049", "runs512", "runs513", "u4", "g8192")
THR_IOUS = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75]


def thr_case(name, seed=0):
    """-> dict(uncerts [U, N], ious, tp_class, iou_thrs, params [P, U (* G)], fix_cd, budget, group)."""
    rng = _rng("thr", name, seed)
    U, P, group = 2, 3, None
    N = {"n2047": 2047, "n2048": 2048, "n2049": 2049, "runs512": 1500, "runs513": 1500, "u4": 300, "g8192": 2049}[name]
    if name == "u4":
        U = 4
    tp = rng.random(N) < 0.85
    ious = np.round(rng.uniform(0.05, 0.999, N), 3)
    wrong = ~(tp & (ious >= 0.5))
    unc = np.stack([np.round(rng.uniform(0, 1.2, N) * np.where(wrong, 1.0, 0.6), 3)] +
                   [np.round(rng.gamma(2.0, 0.05, N), 3) for _ in range(U - 1)])
    params = rng.uniform(0, 1, (P, U))
    params[0] = np.round(params[0], 1)
    if name.startswith("runs"):
        runs = int(name[4:])
        v = np.r_[np.arange(runs), rng.integers(0, runs, N - runs)]
        unc = (rng.permutation(v) / 1024.0)[None]         # exactly `runs` distinct values; halving them keeps them distinct
        params = np.array([[1.0], [0.5]])
    if name == "g8192":
        group = rng.integers(0, 8192, N).astype(np.int32)
        group[[0, N - 1]] = (0, 8191)
        params = rng.uniform(0, 1, (2, U * 8192))
    return dict(uncerts=unc, ious=ious, tp_class=tp, iou_thrs=THR_IOUS, params=params, fix_cd=1, budget=0.95, group=group)


@functools.lru_cache(maxsize=None)
def expected_thr(name, fix_cd=1):
    import thr_ref as R
    c = thr_case(name)
    return R.roc_objective(c["uncerts"], c["ious"], c["tp_class"], c["iou_thrs"], c["params"], fix_cd, c["budget"], c["group"])
