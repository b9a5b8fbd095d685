"""Loop-level restatement of the COCO metric the package computes (reference src/coco_metric.py:219-283 for the containers,
src/custom_cocoeval.py:265-545 for evaluateImg / accumulate / summarize, pycocotools' bbIou and loadRes for IoU and detection
area).  Plain Python loops, one detection and one ground-truth row at a time: slow, easy to read against the reference, and
itself pinned to tests/golden/coco_eval_golden.npz (test_coco_host.py), which the reference's own functions produced.

Records have the layout of the match kernel: per detection row score, cls, rank, matched[4], ignored[4] (bit t per area range)."""
import numpy as np

RECORD_DTYPE = np.dtype([("score", "<f4"), ("cls", "<i4"), ("rank", "<i4"), ("matched", "<u4", (4,)), ("ignored", "<u4", (4,))])
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = [1, 10, 100]
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
STD_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
ALL_THRS = np.linspace(0.05, 0.95, int(np.round((0.95 - 0.05) / 0.05)) + 1, endpoint=True)


def bb_iou(d, g, crowd):
    """pycocotools bbIou on [x, y, w, h]: float64 arithmetic on the float32 values."""
    dx, dy, dw, dh = (float(v) for v in d)
    gx, gy, gw, gh = (float(v) for v in g)
    w = min(dw + dx, gw + gx) - max(dx, gx)
    if w <= 0:
        return 0.0
    h = min(dh + dy, gh + gy) - max(dy, gy)
    if h <= 0:
        return 0.0
    i = w * h
    da, ga = dw * dh, gw * gh
    u = da if crowd else da + ga - i
    return i / u


def image_ground_truth(gt_rows):
    """coco_metric.py:256-275 for one image: rows with class > -1, box [x1, y1, w, h] and area in float32."""
    out = []
    for row in gt_rows[np.where(gt_rows[:, -1] > -1)[0]]:
        box = row[0:4]
        if row[6] < 0:
            break
        out.append(dict(cat=int(row[6]), bbox=[box[1], box[0], box[3] - box[1], box[2] - box[0]],
                        area=(box[3] - box[1]) * (box[2] - box[0]), crowd=int(row[4])))
    return out


def match(det, gt, num_classes, iou_thrs):
    """det [n, M, 7] float32 rows id, x, y, w, h, score, class; gt [n, G, 7] float32 -> (records [n, M], npig [n, C, 4], used [n])."""
    det = np.asarray(det, np.float32)
    gt = np.asarray(gt, np.float32)
    n, M = det.shape[:2]
    T = len(iou_thrs)
    rec = np.zeros((n, M), RECORD_DTYPE)
    npig = np.zeros((n, num_classes, 4), np.int32)
    used = np.zeros((n,), np.int32)
    for i in range(n):
        rec[i]["score"] = det[i, :, 5]
        rec[i]["rank"] = -1
        groups = {}
        for r in range(M):
            cls = det[i, r, 6]
            if not cls > -1:
                rec[i, r]["cls"] = -1
                continue
            used[i] += 1
            rec[i, r]["cls"] = int(cls)
            if 1 <= int(cls) <= num_classes:
                groups.setdefault(int(cls), []).append(r)
        gts = image_ground_truth(gt[i])
        for c in range(1, num_classes + 1):
            rows = groups.get(c, [])
            order = np.argsort([-det[i, r, 5] for r in rows], kind="mergesort") if rows else []
            rows = [rows[j] for j in order]
            for rank, r in enumerate(rows):
                rec[i, r]["rank"] = rank
            rows = rows[:MAX_DETS[-1]]
            g_c = [g for g in gts if g["cat"] == c]
            for a, (lo, hi) in enumerate(AREA_RNG):
                ig_all = [1 if (g["crowd"] or g["area"] < lo or g["area"] > hi) else 0 for g in g_c]
                gtind = np.argsort(ig_all, kind="mergesort") if g_c else []
                g_s = [g_c[j] for j in gtind]
                g_ig = [ig_all[j] for j in gtind]
                npig[i, c - 1, a] = sum(1 for v in g_ig if v == 0)
                for t, thr in enumerate(iou_thrs):
                    taken = [False] * len(g_s)
                    for r in rows:
                        d = det[i, r, 1:5]
                        iou = min([thr, 1 - 1e-10])
                        m = -1
                        for gind, g in enumerate(g_s):
                            if taken[gind] and not g["crowd"]:
                                continue
                            if m > -1 and g_ig[m] == 0 and g_ig[gind] == 1:
                                break
                            v = bb_iou(d, g["bbox"], g["crowd"])
                            if v < iou:
                                continue
                            iou = v
                            m = gind
                        if m == -1:
                            area = d[2] * d[3]                      # float32 product (loadRes on the float32 rows)
                            if area < lo or area > hi:
                                rec[i, r]["ignored"][a] |= np.uint32(1 << t)
                            continue
                        taken[m] = True
                        rec[i, r]["matched"][a] |= np.uint32(1 << t)
                        if g_ig[m]:
                            rec[i, r]["ignored"][a] |= np.uint32(1 << t)
    return rec, npig, used


def accumulate(image_ids, rec, npig, used, gt_count, thr_index, n_thrs=None):
    """custom_cocoeval.py:351-465 over the evaluated images (used > 0) in ascending image id.  gt_count [n, C]: ground-truth
    rows per class (categories = classes that occur in the evaluated images' ground truth, sorted)."""
    ev_imgs = sorted((int(image_ids[i]), i) for i in range(len(used)) if used[i] > 0)
    C = npig.shape[1]
    cats = [c for c in range(1, C + 1) if any(gt_count[i, c - 1] > 0 for _, i in ev_imgs)]
    T, R, K, A, Mx = len(thr_index), len(REC_THRS), len(cats), 4, len(MAX_DETS)
    precision = -np.ones((T, R, K, A, Mx))
    recall = -np.ones((T, K, A, Mx))
    scores = -np.ones((T, R, K, A, Mx))
    for k, c in enumerate(cats):
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                sc, dtm, dtig = [], [], []
                n_pig = 0
                for _, i in ev_imgs:
                    rows = [r for r in range(rec.shape[1]) if rec[i, r]["cls"] == c and 0 <= rec[i, r]["rank"] < max_det]
                    rows.sort(key=lambda r: rec[i, r]["rank"])
                    for r in rows:
                        sc.append(rec[i, r]["score"])
                        dtm.append([(int(rec[i, r]["matched"][a]) >> int(t)) & 1 for t in thr_index])
                        dtig.append([(int(rec[i, r]["ignored"][a]) >> int(t)) & 1 for t in thr_index])
                    n_pig += int(npig[i, c - 1, a])
                if n_pig == 0:
                    continue
                sc = np.asarray(sc, np.float32)
                inds = np.argsort(-sc, kind="mergesort")
                sc_sorted = sc[inds]
                dtm = np.asarray(dtm, bool).reshape(len(sc), T).T[:, inds]
                dtig = np.asarray(dtig, bool).reshape(len(sc), T).T[:, inds]
                for t in range(T):
                    tp_c = fp_c = 0
                    tp, fp = [], []
                    for j in range(len(sc)):
                        tp_c += 1 if (dtm[t, j] and not dtig[t, j]) else 0
                        fp_c += 1 if (not dtm[t, j] and not dtig[t, j]) else 0
                        tp.append(float(tp_c))
                        fp.append(float(fp_c))
                    tp, fp = np.asarray(tp), np.asarray(fp)
                    nd = len(tp)
                    rc = tp / n_pig
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for j in range(nd - 1, 0, -1):
                        if pr[j] > pr[j - 1]:
                            pr[j - 1] = pr[j]
                    q, ss = np.zeros((R,)), np.zeros((R,))
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                        ss[ri] = sc_sorted[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return dict(precision=precision, recall=recall, scores=scores, category_ids=np.asarray(cats, np.int64))


def summarize(ev, iou_thrs):
    """custom_cocoeval.py:473-522."""
    labels = ["all", "small", "medium", "large"]

    def one(ap=1, iou_thr=None, area="all", max_dets=100):
        aind = [i for i, lbl in enumerate(labels) if lbl == area]
        mind = [i for i, md in enumerate(MAX_DETS) if md == max_dets]
        s = ev["precision"] if ap == 1 else ev["recall"]
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    return np.array([one(1), one(1, iou_thr=0.5), one(1, iou_thr=0.75), one(1, area="small"), one(1, area="medium"),
                     one(1, area="large"), one(0, max_dets=1), one(0, max_dets=10), one(0, max_dets=100), one(0, area="small"),
                     one(0, area="medium"), one(0, area="large")], dtype=np.float64)


def per_class_ap(ev, n_labels):
    precision = ev["precision"][:, :, :, 0, -1]
    ap = [0] * max(precision.shape[-1], n_labels)
    for c in range(precision.shape[-1]):
        p = precision[:, :, c]
        p = p[p > -1]
        ap[int(ev["category_ids"][c]) - 1] = np.mean(p) if p.size else -1.0
    return ap


def gt_class_counts(gt, num_classes):
    out = np.zeros((gt.shape[0], num_classes), np.int32)
    for i in range(gt.shape[0]):
        for g in image_ground_truth(np.asarray(gt[i], np.float32)):
            out[i, g["cat"] - 1] += 1
    return out


def image_ids_of(det, start=1):
    """coco_metric.py:233-244, :277: the id of an image is that of its first used row, -1 meaning the running counter."""
    ids, counter = np.zeros((det.shape[0],), np.int64), start
    for i in range(det.shape[0]):
        rows = np.where(det[i, :, -1] > -1)[0]
        if rows.size == 0:
            continue
        ids[i] = counter if det[i, rows[0], 0] == -1 else int(det[i, rows[0], 0])
        counter += 1
    return ids
