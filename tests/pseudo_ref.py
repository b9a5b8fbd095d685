"""numpy restatement of the reference's pseudo-labelling selection (src/SSL_stac.py:302-642, `STAC.score_image`) on COLUMNS
instead of parsed file lines.  The numpy calls are the reference's own (np.mean of python lists, 1 / np.mean([...], axis=0), the
running min / max of find_global_min_max), so the results are the reference's to the last bit for equal inputs;
tests/golden/pseudo_golden.npz holds what the reference itself returned.

One deviation, which the product documents: every branch caps an image at `max_rows` rows, where the reference's
multi-column branches slice the list of columns and fail on an image with 100 written rows.

Columns: as tests/score_ref.py takes them."""
import numpy as np

from score_ref import _term


def components_of(strategy, opt_params=None):
    """(components, invert, gate, rule) of an UNCALIBRATED strategy for a model that emits every column (:387-528)."""
    s = strategy
    rel = lambda src: [(src, "rel_mean", 1.0)]      # noqa: E731
    if "combo" in s:
        return [[("entropy", "scalar", opt_params[0]), ("albox", "rel_mean", opt_params[1])]], 0, 0, "combo"
    if "alluncert" in s:
        return [rel("mcbox"), rel("albox"), [("mcclass", "mean", 1.0)]], 1, 0, "alluncert"
    if "epuncert" in s:
        return [rel("mcbox"), [("mcclass", "mean", 1.0)]], 1, 0, "sigmoid"
    if "ental" in s:
        return [rel("albox"), [("entropy", "scalar", 1.0)]], 1, 0, "sigmoid"
    key = ("uncalib_" if ("box" in s or "class" in s) else "") + s.split("_")[-1]
    table = {"entropy": "entropy", "uncalib_albox": "albox", "uncalib_mcbox": "mcbox", "uncalib_mcclass": "mcclass"}
    if key in table:
        src = table[key]
        tr = "scalar" if src == "entropy" else ("rel_mean" if ("box" in s and "norm" in s) else "mean")
        return [[(src, tr, 1.0)]], 0, 1, "tau"
    return [[("det_score", "scalar", 1.0)]], 0, 1, "tau"


def _component(cols, i, r, comp):
    v = comp[0][2] * _term(cols, i, r, comp[0][0], comp[0][1])
    if len(comp) > 1:
        v = v + comp[1][2] * _term(cols, i, r, comp[1][0], comp[1][1])
    return v


def rows(cols, components, invert, gate, min_score, tau, max_rows=99):
    """The first half: per image the rows that take part, their value v and the candidate flag.
    -> dict(image, row, cls, v: the candidates in (image, rank) order), minmax [n, 2], kept [n], cand [n], and `all_v`: per
    image the values of every participating row (what the reference normalises)."""
    scores = np.asarray(cols["scores"])
    n = scores.shape[0]
    out = {"image": [], "row": [], "cls": [], "v": []}
    minmax = np.zeros((n, 2))
    kept = np.zeros((n,), np.int32)
    cand = np.zeros((n,), np.int32)
    all_v = []
    with np.errstate(all="ignore"):
        for i in range(n):
            written = np.where(scores[i] > min_score)[0]
            kept[i] = len(written)
            part = written[:max_rows]
            if invert:
                columns = [[_component(cols, i, r, comp) for r in part] for comp in components]
                v = list(1 / np.mean(columns, axis=0)) if len(part) else []
            else:
                v = [_component(cols, i, r, components[0]) for r in part]
            gmin, gmax = float("inf"), float("-inf")
            for item in v:
                gmin, gmax = min(gmin, item), max(gmax, item)
            minmax[i] = gmin, gmax
            all_v.append(v)
            for r, item in zip(part, v):
                if (item > tau) if gate else (float(scores[i][r]) > tau):
                    out["image"].append(i)
                    out["row"].append(int(r))
                    out["cls"].append(int(cols["classes"][i][r]))
                    out["v"].append(float(item))
                    cand[i] += 1
    res = {k: np.asarray(val, np.float64 if k == "v" else np.int64) for k, val in out.items()}
    return res, minmax, kept, cand, all_v


def select(cols, names, strategy, tau, min_score, opt_params=None, opt_thrs=None, max_rows=99):
    """Both halves: what `STAC.score_image` returns - (names, classes, boxes, pseudo_score) - written the reference's way
    (lists per image, the det_score filter as a multiplication, the dataset-wide min / max over every participating row)."""
    components, invert, gate, rule = components_of(strategy, opt_params)
    scores = np.asarray(cols["scores"])
    _, _, kept, _, all_v = rows(cols, components, invert, gate, min_score, tau, max_rows)
    img = [i for i in range(len(kept)) if kept[i]]                         # images that reach the file
    part = {i: np.where(scores[i] > min_score)[0][:max_rows] for i in img}
    with np.errstate(all="ignore"):
        if rule == "tau":
            per_image_score = [np.asarray(all_v[i]) for i in img]
            flt = [pis > tau for pis in per_image_score]
        else:
            gmin, gmax = float("inf"), float("-inf")
            for i in img:
                for item in all_v[i]:
                    gmin, gmax = min(gmin, item), max(gmax, item)
            norm = [[(x - gmin) / (gmax - gmin) if gmax - gmin > 0 else 0 for x in all_v[i]] for i in img]
            sigmoid = [np.asarray([float(scores[i][r]) for r in part[i]]) > tau for i in img]
            per_image_score = [np.asarray(norm[u]) * sigmoid[u] for u in range(len(img))]
            if rule == "combo":
                flt = [(np.asarray(pis) <= np.mean(opt_thrs)) * (np.asarray(pis) > 0) for pis in per_image_score]
            elif rule == "alluncert":
                flt = [pis > tau for pis in per_image_score]
            else:
                flt = sigmoid
    keep = [u for u in range(len(img)) if sum(flt[u]) > 0]
    out_names = np.asarray([names[img[u]] for u in keep])
    classes = [np.asarray([float(cols["classes"][img[u]][r]) for r in part[img[u]]])[flt[u]] for u in keep]
    boxes = [np.asarray([[float(x) for x in cols["boxes"][img[u]][r][:4]] for r in part[img[u]]])[flt[u]] for u in keep]
    pseudo = [np.asarray(per_image_score[u])[flt[u]] for u in keep]
    return out_names, classes, boxes, pseudo


# ------------------------------------------------------------------ the fixture (tests/golden/pseudo_golden.npz)
COLUMN_KEYS = ("boxes", "scores", "classes", "entropy", "albox", "mcbox", "mcclass")


class Golden:
    """What tests/golden/make_pseudo_golden.py stored: the datasets' columns and, per case, the reference's returns."""

    def __init__(self):
        import os
        self.path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pseudo_golden.npz")
        self.z = z = np.load(self.path)
        self.min_score, self.max_rows = float(z["min_score"][0]), int(z["max_rows"][0])
        self.opt, self.opt_thrs = tuple(float(v) for v in z["opt_params"]), [float(v) for v in z["opt_thrs"]]
        self.names = [str(v) for v in z["names"]]
        self.cases = [(str(d), str(s), float(t)) for d, s, t in zip(z["case_dataset"], z["case_strategy"], z["case_tau"])]
        self.ids = ["%s-%s-%g" % c for c in self.cases]

    def columns(self, ds, n=None):
        return {k: self.z["%s_%s" % (ds, k)][:n] for k in COLUMN_KEYS}, int(self.z["%s_num_classes" % ds][0])

    def case(self, ci):
        """-> (columns of the case's images, num_classes, names, dict of the case's stored arrays)."""
        ds = self.cases[ci][0]
        n = int(self.z["k%d_n" % ci][0])
        cols, C = self.columns(ds, n)
        pre = "k%d_" % ci
        return cols, C, self.names[:n], {k[len(pre):]: self.z[k] for k in self.z.files if k.startswith(pre)}

    def returned(self, ci):
        """What score_image returned for the case, in its shapes: (names, classes, boxes, pseudo_score)."""
        g = self.case(ci)[3]
        if not len(g["count"]):
            return g["names"], [], [], []
        cut = np.cumsum(g["count"])[:-1]
        return g["names"], np.split(g["classes"], cut), np.split(g["boxes"], cut), np.split(g["pseudo"], cut)


def same_selection(got, want, pseudo_rtol=1e-12):
    """Two (names, classes, boxes, pseudo_score) tuples: everything exact but the scores, which agree to pseudo_rtol with
    inf / NaN in equal places."""
    assert [str(v) for v in got[0]] == [str(v) for v in want[0]]
    assert len(got[1]) == len(want[1]) == len(got[2]) == len(want[2])
    for a, b in zip(got[1], want[1]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(got[2], want[2]):
        np.testing.assert_array_equal(np.asarray(a).reshape(-1, 4), np.asarray(b).reshape(-1, 4))
    for a, b in zip(got[3], want[3]):
        np.testing.assert_allclose(a, b, rtol=pseudo_rtol, atol=0)


def as_records(res, cols, dtype):
    """The candidates of `rows` as the device's record array (float32 box and det_score, as stored)."""
    rec = np.zeros((len(res["v"]),), dtype)
    rec["image"], rec["row"], rec["cls"], rec["v"] = res["image"], res["row"], res["cls"], res["v"]
    for k, (i, r) in enumerate(zip(res["image"], res["row"])):
        rec["box"][k] = np.asarray(cols["boxes"][i][r][:4], np.float32)
        rec["det_score"][k] = np.float32(cols["scores"][i][r])
    return rec
