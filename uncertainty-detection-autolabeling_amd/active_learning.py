"""The scoring step of the reference's active-learning loop (src/active_learning_loop.py:528-840) without the text file
in between.

The reference serves the unlabeled pool, writes one dict per detection to prediction_data.txt (infer_model.py:836-960),
parses every line back (`ActiveLearning.score_image`, :528-765), turns each detection into one to three uncertainty numbers,
reduces them per image with mean or max, combines the columns over the dataset and ranks the images (`select_images`,
:767-840).  Here the per-detection numbers and the per-image reduction run on the device, on the detections resident in a
handle (`ServingDriver.score_images` / `serve_score`, C entry point uda_score_images) or on host arrays
(`score_detections`, uda_score_images_np); the host keeps n x 3 doubles per batch (`ImageScores`) and does the dataset-wide
part (`ImageScores.scores`, `select_images`).

  resolve_strategy   the reference's substring grammar -> `Strategy` (the descriptor the kernel takes)
  ImageScores        accumulator over batches + the combination of :733-764
  select_images      class balancing (`perc`), `nee`, `bottomk`, top-k of :767-840
  score_detections   the same kernel on host columns (calibrated strategies, gathered multi-GPU batches)
  default_min_score  the writer's threshold (infer_model.py:568-573)

Two deviations from the file route: the device scores the unrounded float32 columns where the file holds them
rounded to 4 decimals, and names are paired with scores in served order where the reference pairs them with np.unique(names).
"""
import ctypes as C

import numpy as np

from . import capi

SOURCES = {"entropy": capi.SCORE_ENTROPY, "det_score": capi.SCORE_DET_SCORE, "albox": capi.SCORE_ALBOX,
           "mcbox": capi.SCORE_MCBOX, "mcclass": capi.SCORE_MCCLASS}
TRANSFORMS = {"scalar": capi.SCORE_SCALAR, "mean": capi.SCORE_MEAN, "rel_mean": capi.SCORE_REL_MEAN}
BOX_CALIB_MODE, CLASS_CALIB_MODE = "iso_perclscoo_", "iso_percls_"          # active_learning_loop.py:556-557
# keys of a prediction_data.txt line (writers.prediction_records) that the grammar can select and that hold no uncertainty
# this path scores.  ("bbox" and "class" cannot be selected: a strategy that ends in them contains "box" / "class", which turns
# the key into "uncalib_bbox" / "uncalib_class", and those are in no line - the reference scores det_score then.)
_UNSCORED = ("logits", "probab", CLASS_CALIB_MODE + "probab")


class Strategy:
    """A resolved scoring strategy.

    components: per component one or two terms (source, transform, weight) with the names of SOURCES / TRANSFORMS;
    reduce_mean: mean (True) or max over the kept detections of an image;
    columns: source name -> key of the column in the dict `score_detections` takes ("albox", or "iso_perclscoo_albox" under
    a `calib` strategy); calibrated: the strategy reads calibrated columns, which only the host-array path serves;
    combine: None (one component) | "highep_lowal" | "sota" | "sum" - the dataset-wide combination of :733-764."""

    def __init__(self, name, components, reduce_mean, columns, calibrated, combine):
        self.name, self.components, self.reduce_mean = name, components, bool(reduce_mean)
        self.columns, self.calibrated, self.combine = columns, bool(calibrated), combine

    @property
    def n_comp(self):
        return len(self.components)

    def sources(self):
        return sorted({t[0] for comp in self.components for t in comp})

    def desc(self):
        d = capi.ScoreDesc()
        d.n_comp, d.reduce_mean = len(self.components), int(self.reduce_mean)
        for k, comp in enumerate(self.components):
            d.n_terms[k] = len(comp)
            for t, (src, tr, w) in enumerate(comp):
                d.term[k][t].source, d.term[k][t].transform, d.term[k][t].weight = SOURCES[src], TRANSFORMS[tr], float(w)
        return d

    def __repr__(self):
        return "Strategy(%r, %r, %s)" % (self.name, self.components, "mean" if self.reduce_mean else "max")


def emitted_sources(params):
    """The uncertainty columns a configuration emits (the split of `postprocess.unpack_detections`)."""
    mc = bool(params.get("mc_dropout"))
    out = {"det_score"}
    if params.get("enable_softmax"):
        out.add("entropy")
    if params.get("loss_attenuation"):
        out.add("albox")
    if mc and (params.get("mc_boxheadrate") or params.get("mc_dropoutrate")):
        out.add("mcbox")
    if mc and (params.get("mc_classheadrate") or params.get("mc_dropoutrate")):
        out.add("mcclass")
    return out


def _emitted(params):
    """The source names a model emits: params are the model parameters, or a dict of source names -> anything."""
    return (set(params) | {"det_score"}) if set(params) <= set(SOURCES) else emitted_sources(params)


class _Terms:
    """Builds (source, transform, weight) terms for a strategy string and notes the column key of every source read: the part
    of the grammar the active-learning loop and the pseudo-labelling teacher (pseudo_labels.resolve_selection) share."""

    def __init__(self, s, has):
        self.s, self.has, self.calib = s, has, "calib" in s
        self.box_mode = BOX_CALIB_MODE if self.calib else ""
        self.cls_mode = CLASS_CALIB_MODE if self.calib else ""
        self.columns = {}

    def term(self, src, tr, w=1.0):
        if src not in self.has:
            raise ValueError("strategy %r reads %s, which this model does not emit" % (self.s, src))
        if src != "det_score":
            self.columns[src] = (self.box_mode if src in ("albox", "mcbox") else self.cls_mode) + src
        return (src, tr, float(w))

    def combo(self, opt_params):
        if opt_params is None or len(opt_params) < 2:
            raise ValueError("strategy %r needs opt_params = (entropy weight, aleatoric weight)" % self.s)
        return [[self.term("entropy", "scalar", opt_params[0]), self.term("albox", "rel_mean", opt_params[1])]]

    def alluncert(self):
        return [[self.term("mcbox", "rel_mean")], [self.term("albox", "rel_mean")], [self.term("mcclass", "mean")]]

    def epuncert(self):
        return [[self.term("mcbox", "rel_mean")], [self.term("mcclass", "mean")]]

    def ental(self):
        return [[self.term("albox", "rel_mean")], [self.term("entropy", "scalar")]]

    def single(self):
        """The last branch of both loops: the key add_mode + strategy.split("_")[-1] of a file line, det_score when the line
        would not hold it."""
        s, has = self.s, self.has
        if self.calib:
            add_mode = BOX_CALIB_MODE if "box" in s else CLASS_CALIB_MODE
        else:
            add_mode = "uncalib_" if ("box" in s or "class" in s) else ""
        key = add_mode + s.split("_")[-1]
        in_file = {"det_score": ("det_score", "")}
        if "entropy" in has:
            in_file["entropy"] = ("entropy", "")
            in_file[CLASS_CALIB_MODE + "entropy"] = ("entropy", CLASS_CALIB_MODE)
        for src in ("albox", "mcbox", "mcclass"):
            if src in has:
                mode = CLASS_CALIB_MODE if src == "mcclass" else BOX_CALIB_MODE
                in_file["uncalib_" + src] = (src, "")
                in_file[mode + src] = (src, mode)
        if key in in_file:
            src, mode = in_file[key]
            if src in ("entropy", "det_score"):
                tr = "scalar"                                  # a python float in the line (:703-704)
            else:
                tr = "rel_mean" if ("box" in s and "norm" in s) else "mean"
            if tr == "rel_mean" and src == "mcclass":
                raise ValueError("strategy %r relativizes %s, which has no box shape" % (s, key))
            if src != "det_score":
                self.columns[src] = mode + src
            return [[(src, tr, 1.0)]]
        if "entropy" in has and key in _UNSCORED:
            # a key the writer emits (or would, given calibrators) that this path does not turn into a score
            raise ValueError("strategy %r selects the key %r of a prediction line, which this path does not score" % (s, key))
        return [[("det_score", "scalar", 1.0)]]               # the reference's fallback (:707-708)

    def calibrated(self):
        return any(v.startswith((BOX_CALIB_MODE, CLASS_CALIB_MODE)) for v in self.columns.values())


def resolve_strategy(strategy, params, opt_params=None):
    """`ActiveLearning.scoring_strategy` -> `Strategy`, branch for branch in the order of score_image (:544-708): `combo`;
    `alluncert` | `sota`; `epuncert`; `ental`; otherwise the key add_mode + strategy.split("_")[-1] of a file line.  All tests
    are substring tests, as in the reference.  params: the model parameters, which decide what a line would contain (a dict
    of emitted source names -> anything is taken as that set itself).  A branch that reads a column the model does not emit
    raises ValueError (the reference: KeyError); in the last branch a key the line would not contain falls back to det_score
    (:707-708), and a key it would contain but that holds no uncertainty number (logits, probab) raises ValueError."""
    s = str(strategy)
    t = _Terms(s, _emitted(params))
    multi = [k for k in ("alluncert", "sota", "epuncert", "ental") if k in s]
    if "combo" in s:
        if multi:
            raise ValueError("strategy %r: `combo` beside %s has no meaning in the reference (its per-image accumulator "
                             "is sized for the latter and filled by the former)" % (s, multi[0]))
        comps = t.combo(opt_params)
    elif "alluncert" in s or "sota" in s:
        comps = t.alluncert()
    elif "epuncert" in s:
        comps = t.epuncert()
    elif "ental" in s:
        comps = t.ental()
    else:
        comps = t.single()
    combine = None
    if len(comps) > 1:
        if "highep_lowal" in s:
            if len(comps) != 3:
                raise ValueError("strategy %r: highep_lowal needs the three columns of alluncert / sota" % s)
            combine = "highep_lowal"
        elif "sota" in s:
            combine = "sota"
        else:
            combine = "sum"
    return Strategy(s, comps, "mean" in s, t.columns, t.calibrated(), combine)


def default_min_score(params, average_score=0, ssl=False):
    """The threshold `Infer.iterate_infer` writes detections above (infer_model.py:568-573)."""
    return 0.1 if ssl else (params["nms_configs"]["score_thresh"] or average_score or 0.4)


def min_max_scaler(data):
    """ActiveLearning.min_max_scaler (:319-321)."""
    return [(x - min(data)) / (max(data) - min(data)) for x in data]


def z_score_normalization(data):
    """ActiveLearning.z_score_normalization (:324-326)."""
    return (data - np.mean(data)) / np.std(data)


def combine_components(components, combine):
    """The dataset-wide combination of the per-image columns (:733-764).  components [K, n_comp] float64 -> [K]."""
    comp = np.asarray(components, np.float64)
    if combine is None:
        return comp[:, 0].copy()
    cols = range(comp.shape[1])
    if combine == "highep_lowal":
        scaled = np.asarray([min_max_scaler(comp[:, i]) for i in cols])
        ep = np.sum([scaled[i] for i in [0, 2]], axis=0)
        return ep - scaled[1]
    if combine == "sota":
        return np.max([z_score_normalization(comp[:, i]) for i in cols], axis=0)
    return np.sum([min_max_scaler(comp[:, i]) for i in cols], axis=0)


class ImageScores:
    """Per-image results accumulated over the batches of a pool: name, components, kept detections, kept detections per
    class.  Images with no kept detection are dropped - they never reach the reference's file."""

    def __init__(self, strategy):
        self.strategy = strategy
        self.names, self._comp, self._count, self._cls = [], [], [], []

    def add(self, names, result):
        """names: the batch's image names; result: (components [n, n_comp], count [n], class_counts [n, C])."""
        comp, count, cls = result
        names = list(names)
        if len(names) != len(count):
            raise ValueError("%d names for %d scored images" % (len(names), len(count)))
        keep = np.nonzero(np.asarray(count) > 0)[0]
        self.names += [names[i] for i in keep]
        self._comp.append(np.asarray(comp, np.float64)[keep])
        self._count.append(np.asarray(count, np.int32)[keep])
        self._cls.append(np.asarray(cls, np.int32)[keep])
        return len(keep)

    def __len__(self):
        return len(self.names)

    @property
    def components(self):
        return np.concatenate(self._comp) if self._comp else np.zeros((0, self.strategy.n_comp))

    @property
    def count(self):
        return np.concatenate(self._count) if self._count else np.zeros((0,), np.int32)

    @property
    def class_counts(self):
        return np.concatenate(self._cls) if self._cls else np.zeros((0, 0), np.int32)

    def scores(self):
        """One score per image: the single component, or the combination of :733-764 over everything added so far."""
        if not self.names:
            raise ValueError("ImageScores: nothing scored")
        return combine_components(self.components, self.strategy.combine)

    def select(self, num_per_iter, im_names):
        return select_images(self.scores(), self.names, self.class_counts, self.strategy.name, num_per_iter, im_names)


def select_images(scores, names, class_counts, strategy, num_per_iter, im_names):
    """`ActiveLearning.select_images` (:767-840) on per-image scores: `perc` multiplies each score with the image's mean
    class weight (total kept detections / kept detections of the class; np.insert puts 0 for classes below the highest that
    nobody predicted, exactly as the reference calls it), `nee` takes the top of four score quantile bins and the bottom of
    the fifth, `bottomk` the lowest, otherwise the highest num_per_iter.  names[i] belongs to scores[i] (served order).
    Returns the indices into im_names whose stem was selected."""
    s = str(strategy)
    per_image = np.asarray(scores, np.float64)
    names = np.asarray(list(names))
    if "perc" in s:
        cc = np.asarray(class_counts)
        total = cc.sum(0)
        class_names = np.nonzero(total > 0)[0] + 1                     # np.unique of every predicted class
        n_ideal_classes = np.arange(np.max(class_names)) + 1
        class_distribution = [int(total[c - 1]) for c in class_names]
        weights = np.asarray([sum(class_distribution) / class_distribution[i] for i in range(len(class_names))])
        weights = np.insert(weights, [int(i - 1) for i in n_ideal_classes if i not in class_names], 0)
        per_image_cls = [np.mean([weights[int(c)] for c in np.nonzero(row > 0)[0]]) for row in cc]
        per_image = np.multiply(per_image_cls, per_image)
    if "nee" in s:
        n = 5
        batch_size, remainder = num_per_iter // n, num_per_iter % n
        selected = []
        bins = np.array_split(np.argsort(per_image), n)
        for i in range(n - 1):
            selected.extend(bins[i][-batch_size:])
        selected.extend(bins[-1][: batch_size + remainder])
        chosen = [x.split(".")[0] for x in names[selected]]
    else:
        ordered = [x.split(".")[0] for _, x in sorted(zip(per_image, names), key=lambda pair: pair[0])]
        chosen = ordered[:num_per_iter] if "bottomk" in s else ordered[-num_per_iter:]
    return [i for i, item in enumerate(im_names) if item.split(".")[0] in chosen]


def _column(a, shape, what, dtype, finite=True):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != shape:
        raise ValueError("%s must be %s, got %s" % (what, shape, a.shape))
    if finite and not np.isfinite(a).all():
        raise ValueError("%s must be finite" % what)
    return a


def detection_columns(columns, strategy, resolver, params, opt_params, num_classes, as_float32):
    """What `score_detections` and `pseudo_labels.select_detections` do before they call the library: the strategy resolved by
    `resolver` (a string: against params, or against the columns present when params is None), every column it reads checked
    and cast.  -> (strategy, the seven arrays boxes, scores, classes, entropy, albox, mcbox, mcclass - None where the strategy
    reads none -, n, M, mcclass columns, num_classes)."""
    dt = np.float32 if as_float32 else np.float64
    cols = {k: v for k, v in columns.items() if v is not None}
    if not isinstance(strategy, Strategy):
        if params is None:
            present = {src for src in ("entropy", "albox", "mcbox", "mcclass") if any(k == src or k.endswith("_" + src) for k in cols)}
            params = dict.fromkeys(present)
        strategy = resolver(strategy, params, opt_params)
    scores = np.asarray(cols["scores"])
    if scores.ndim != 2:
        raise ValueError("scores must be [n, M], got %s" % (scores.shape,))
    n, M = scores.shape
    scores = _column(scores, (n, M), "scores", dt)
    boxes = _column(np.asarray(cols["boxes"])[..., :4], (n, M, 4), "boxes", dt)
    classes = _column(cols["classes"], (n, M), "classes", dt)
    if num_classes is None:
        num_classes = int((params or {}).get("num_classes") or max(int(classes.max()) if classes.size else 1, 1))
    arrays = {"entropy": None, "albox": None, "mcbox": None, "mcclass": None}
    mcw = 0
    for src in strategy.sources():
        if src == "det_score":
            continue
        key = strategy.columns[src]
        if key not in cols:
            raise ValueError("strategy %r reads the column %r, which is not given" % (strategy.name, key))
        a = np.asarray(cols[key])
        finite = not as_float32 or src == "entropy"
        if src == "mcclass":
            if a.ndim == 2:
                a = a[..., None]
            mcw = a.shape[-1]
            arrays[src] = _column(a, (n, M, mcw), key, dt, finite)
        else:
            arrays[src] = _column(a, (n, M) if src == "entropy" else (n, M, 4), key, dt, finite)
    return strategy, [boxes, scores, classes] + list(arrays.values()), n, M, int(mcw), int(num_classes)


def raise_from_rc(rc, lib, what):
    """A handle-free entry point returned rc: a class id the caller's num_classes does not cover is a ValueError."""
    if rc != 0:
        msg = lib.uda_last_error(None).decode()
        raise (ValueError if "class id outside" in msg else capi.UdaError)("%s failed: %s" % (what, msg))


def score_detections(columns, strategy, min_score, params=None, opt_params=None, num_classes=None, device=0, as_float32=False):
    """`score_image`'s per-image part on host arrays, through the same kernel in float64 (uda_score_images_np): for the
    calibrated strategies - the columns `BoxCalibrator` / `ClassCalibrator` return already are on the host - and for callers
    that hold detections of their own (a gathered multi-GPU batch).

    columns: dict with boxes [n, M, 4], scores [n, M], classes [n, M] and the uncertainty columns the strategy names
    (`Strategy.columns`: "entropy" [n, M], "albox" / "mcbox" [n, M, 4], "mcclass" [n, M, C'] - the keys of
    `ServingDriver.serve_unpacked` - or "iso_percls_entropy", "iso_perclscoo_albox", ... under a `calib` strategy).
    strategy: a string (resolved against params, or against the columns present when params is None) or a `Strategy`.
    Values must be finite (ValueError).  as_float32=True runs the float32 instantiation the handle runs
    (uda_score_images_np_f32) on the columns cast to float32: the raw device columns, whose albox / mcbox / mcclass may then
    hold NaN / inf - the kernel applies np.nan_to_num to them, as the reference's caller does (infer_model.py:607-631).
    Returns (components [n, n_comp] float64, count [n], class_counts [n, num_classes])."""
    strategy, arrays, n, M, mcw, num_classes = detection_columns(columns, strategy, resolve_strategy, params, opt_params, num_classes,
                                                                 as_float32)
    comp = np.zeros((n, strategy.n_comp), np.float64)
    count = np.zeros((n,), np.int32)
    cls = np.zeros((n, num_classes), np.int32)
    lib = capi.load()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    desc = strategy.desc()
    fn, what = (lib.uda_score_images_np_f32, "uda_score_images_np_f32") if as_float32 else (lib.uda_score_images_np, "uda_score_images_np")
    raise_from_rc(fn(int(device), C.byref(desc), float(min_score), *[p(a) for a in arrays], n, M, num_classes, mcw, p(comp), p(count),
                     p(cls)), lib, what)
    return comp, count, cls
