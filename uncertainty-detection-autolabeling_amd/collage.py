"""Rare-class collages (RCC): the reference's `Parent_SSL.crop_collage` (ssl_utils/parent.py:317-686, driven by ssl_utils/rcc.py).

Every box of a target class is cut out of its image with a random margin, scaled to the full image height with Pillow's
Lanczos filter and packed side by side into collages; the labels of every box that falls into a crop are carried along.

`plan_collage` restates the procedure as decisions - which crop, at which size, where - from the image sizes alone: the crops,
the temporaries and a list of resample jobs in levels.  `crop_collage` cuts the crops on the host (a crop is a copy) and hands
all the jobs to ONE device call, `uda_resample_np` (csrc/kernels_collage.hip), whose pixels are Pillow's bit for bit.  With
`manual_augmentations` (parent.py:261-315, 534-537) every resized crop gets one of five random augmentations - flip, brightness,
contrast, Gaussian blur, noise - before it is pasted: the planner draws them on the reference's stream and the call becomes
`uda_collage_np` (csrc/kernels_augment.hip), again Pillow's pixels bit for bit.  The writers produce the reference's files.
What the reference also offers and `rcc.py` as shipped switches off is not built and raises NotImplementedError naming the
option: rand_augment_wholeimage, full_im, plot_final, the TFRecord creators and `generate_commands_and_create_dirs` (tfrecords /
commands), weight_images_cls_dist (cb_weight)."""
import ctypes as C
import json
import os

import numpy as np

from . import capi

MAX_BOXES_PER_COLLAGE = 100
# the ops of a uda_collage_np job (include/uda_hip.h); the reference's five augmentations in the order of its list
OP_RESIZE, OP_FLIP, OP_BRIGHTNESS, OP_CONTRAST, OP_BLUR, OP_NOISE = range(6)
AUGMENT_KINDS = ("flip", "brightness", "contrast", "blur", "noise")
NOT_BUILT = ("rand_augment_wholeimage", "full_im", "plot_final", "tfrecords", "commands", "cb_weight")


def _refuse(options):
    for name in NOT_BUILT:
        if options.get(name):
            raise NotImplementedError("crop_collage: option %r of the reference is not built (rcc.py as shipped sets it off)" % name)
    unknown = sorted(set(options) - set(NOT_BUILT))
    if unknown:
        raise TypeError("crop_collage: unknown options %s" % unknown)


class CollagePlan:
    """What `plan_collage` decided.

    crops      [(image index, x0, y0, x1, y1)] in packing order (after the seeded shuffle): Image.crop's integer box; source
               plane k of the device call is crop k
    tmp_wh     [(w, h)] of the temporaries (plane ids S + t)
    jobs       [K, 7] int32 (level, source plane, destination plane, x, y, w, h), sorted by level; the outputs are the plane
               ids S + T + n.  A plan made with manual_augmentations has [K, 9] jobs (.., op, arg) for uda_collage_np
    params     [P] float64: the factors and radii the jobs' arg indexes;  noise: uint8, the noise of the op-5 jobs one after
               another in job-list order;  augment: per crop (kind, parameter) - the kind's name and its factor or radius, None
               for flip and noise.  Empty without manual_augmentations
    n, height, width   the collages
    labels     per collage [[class, [x1, y1, x2, y2]], ...] in the reference's float arithmetic
    crop_boxes, crop_classes   per crop what it carries, in crop coordinates (the two lists of a crop may differ in length)"""

    def __init__(self, crops, tmp_wh, jobs, n, height, width, labels, crop_boxes=None, crop_classes=None, params=(), noise=(), augment=None):
        self.crops, self.tmp_wh, self.n, self.height, self.width, self.labels = crops, tmp_wh, n, height, width, labels
        self.crop_boxes, self.crop_classes = crop_boxes, crop_classes
        jobs = np.asarray(jobs, np.int32).reshape(-1, 7 if augment is None else 9)
        self.jobs = np.ascontiguousarray(jobs[np.argsort(jobs[:, 0], kind="stable")])
        self.params, self.augment = np.asarray(params, np.float64).reshape(-1), [] if augment is None else augment
        if len(noise):                                               # per noise job, indexed by its arg -> job-list order
            noise = [noise[a] for a in self.jobs[self.jobs[:, 7] == OP_NOISE, 8]]
            self.jobs[self.jobs[:, 7] == OP_NOISE, 8] = np.arange(len(noise))
            self.noise = np.concatenate([z.reshape(-1) for z in noise])
        else:
            self.noise = np.zeros(0, np.uint8)

    def images_used(self):
        return sorted({c[0] for c in self.crops})


def _size(image):
    if hasattr(image, "shape"):
        return int(image.shape[1]), int(image.shape[0])
    w, h = image
    return int(w), int(h)


def plan_collage(images, classes, boxes, target_class, dataset="KITTI", scale=False, low_scale=0.5, high_scale=1.0, rng=None,
                 manual_augmentations=False):
    """parent.py:380-598 without pixels.  images: per image an array [h, w, 3] or (width, height); classes / boxes: per image the
    class names and the boxes - [x1, y1, x2, y2] for KITTI, [y1, x1, y2, x2] otherwise (swapped here, as the reference does).
    rng: None seeds numpy's global legacy stream with 42 and draws from it, as the reference does; a np.random.RandomState is
    drawn from as it is.  manual_augmentations: per packed crop, after its resizes, `choice(5)` and the kind's own draw on the same
    stream (parent.py:261-315); the augment job reads the resized crop from a temporary one level later.  A flip rewrites the
    crop's boxes in place as the reference does - with the RESIZED width on boxes still in crop coordinates.  Returns a
    CollagePlan."""
    if rng is None:
        np.random.seed(42)
        rng = np.random
    if len(images) == 0:
        raise ValueError("plan_collage: no images")
    crops, crop_boxes, crop_classes = [], [], []
    for index in range(len(images)):
        width, height = _size(images[index])
        cls_im, boxes_im = np.array(classes[index]), np.array(boxes[index])
        if len(boxes_im) == 0:
            continue
        if dataset != "KITTI":
            boxes_im = np.stack([boxes_im[:, 1], boxes_im[:, 0], boxes_im[:, 3], boxes_im[:, 2]], axis=-1)
        for cls, box in zip(cls_im, boxes_im):
            if cls not in target_class:
                continue
            padding = rng.uniform(low_scale, high_scale)
            wtransform = (box[2] - box[0]) * padding
            htransform = (box[3] - box[1]) * padding
            new_box = [max(0, box[0] - wtransform), max(0, box[1] - htransform), min(width, box[2] + wtransform),
                       min(height, box[3] + htransform)]
            overlapping_boxes, overlapping_classes = [], []
            for other_cls, other_box in zip(cls_im, boxes_im):
                if ((other_box[0] < new_box[2] and other_box[0] > new_box[0]) or (other_box[2] < new_box[2] and other_box[2] > new_box[0])) and (
                        (other_box[1] < new_box[3] and other_box[1] > new_box[1]) or (other_box[3] < new_box[3] and other_box[3] > new_box[1])):
                    overlapping_classes.append(other_cls)
                    adjusted_box = [max(other_box[0], new_box[0]) - new_box[0], max(other_box[1], new_box[1]) - new_box[1],
                                    min(new_box[2], other_box[2]) - new_box[0], min(new_box[3], other_box[3]) - new_box[1]]
                    if (adjusted_box[2] - adjusted_box[0]) > 2 and (adjusted_box[3] - adjusted_box[1]) > 2:
                        overlapping_boxes.append(adjusted_box)       # (the class stays: the two lists may differ, zip truncates)
            if len(overlapping_boxes) < 100:
                x0, y0, x1, y1 = (int(round(v)) for v in new_box)    # Image.crop
                if x1 < x0:
                    raise ValueError("Coordinate 'right' is less than 'left'")
                if y1 < y0:
                    raise ValueError("Coordinate 'lower' is less than 'upper'")
                crops.append((index, x0, y0, x1, y1))
                crop_boxes.append(overlapping_boxes)
                crop_classes.append(overlapping_classes)
    indices = np.arange(len(crops))
    rng.shuffle(indices)
    crops = [crops[i] for i in indices]
    crop_boxes = [crop_boxes[i] for i in indices]
    crop_classes = [crop_classes[i] for i in indices]
    collage_width, collage_height = _size(images[-1])                # the last image opened, even one without boxes
    S = len(crops)
    tmp_wh, jobs, labels_all = [], [], []
    OUT = -1                                                          # destination ids below OUT - n are outputs until S + T is known

    def tmp(w, h):
        tmp_wh.append((int(w), int(h)))
        return ("t", len(tmp_wh) - 1)

    params, noise, augment = [], [], [] if manual_augmentations else None

    def job(level, src, dst, x, y, w, h, dst_w, dst_h, op=OP_RESIZE, arg=0):
        if x < dst_w and y < dst_h:                                   # (a paste wholly outside pastes nothing)
            jobs.append((level, src, dst, int(x), int(y), int(w), int(h), op, arg))

    k, n = 0, 0
    while k < S:
        x_offset, labels, box_count = 0, [], 0
        while x_offset < collage_width and k < S and box_count < MAX_BOXES_PER_COLLAGE:
            _, cx0, cy0, cx1, cy1 = crops[k]
            original_boxes, original_classes = crop_boxes[k], crop_classes[k]
            original_width, original_height = cx1 - cx0, cy1 - cy0
            src, last = ("s", k), k == S - 1
            k += 1
            new_width = collage_width - x_offset if last else int(original_width * collage_height / original_height)
            if new_width < 1 or collage_height < 1 or original_width < 1 or original_height < 1:
                raise ValueError("height and width must be > 0")
            level, img_w, img_h = 0, new_width, collage_height
            second = x_offset + new_width > collage_width
            if second or scale or manual_augmentations:               # the resized crop is read again: a temporary
                t = tmp(new_width, collage_height)
                job(level, src, t, 0, 0, new_width, collage_height, new_width, collage_height)
                src, level = t, level + 1
            if second:
                img_w = collage_width - x_offset
                if scale or manual_augmentations:
                    t = tmp(img_w, img_h)
                    job(level, src, t, 0, 0, img_w, img_h, img_w, img_h)
                    src, level = t, level + 1
            op, arg = OP_RESIZE, 0
            if manual_augmentations:                                  # apply_manual_augmentation: np.random.choice of five, then its draw
                kind = int(rng.choice(5))
                op, value = kind + 1, None
                if op == OP_FLIP:
                    for box in original_boxes:                        # (the resized width, boxes in crop coordinates: the reference's own)
                        box[0], box[2] = img_w - box[2], img_w - box[0]
                elif op in (OP_BRIGHTNESS, OP_CONTRAST):
                    value = float(rng.uniform(0.7, 1.3))
                elif op == OP_BLUR:
                    value = float(rng.uniform(1, 3))
                else:
                    noise.append(rng.randint(5, 20, (img_h, img_w, 3), dtype="uint8"))
                    arg = len(noise) - 1
                if value is not None:
                    params.append(value)
                    arg = len(params) - 1
                augment.append((AUGMENT_KINDS[kind], value))
                if scale:                                             # the quadrants read the augmented crop: one more temporary
                    t = tmp(img_w, img_h)
                    job(level, src, t, 0, 0, img_w, img_h, img_w, img_h, op, arg)
                    src, level, op, arg = t, level + 1, OP_RESIZE, 0
            if scale:
                quadrant_sizes = [(np.ceil(img_w * 0.75), np.ceil(img_h * 0.75)), (np.ceil(img_w * 0.25), np.ceil(img_h * 0.75)),
                                  (np.ceil(img_w * 0.75), np.ceil(img_h * 0.25)), (np.ceil(img_w * 0.25), np.ceil(img_h * 0.25))]
                quadrant_sizes = np.asarray(quadrant_sizes).astype(int)
                part = tmp(img_w, img_h)
                y_offset_part, x_offset_part, positions = 0, 0, []
                for j in range(4):
                    if j == 2:
                        y_offset_part, x_offset_part = quadrant_sizes[0][1], 0
                    job(level, src, part, x_offset_part, y_offset_part, quadrant_sizes[j][0], quadrant_sizes[j][1], img_w, img_h)
                    positions.append((x_offset + x_offset_part, y_offset_part))
                    x_offset_part += quadrant_sizes[j][0]
                    if j == 1:
                        x_offset_part = 0
                for idx, pos in enumerate(positions):
                    scale_x = quadrant_sizes[idx][0] / original_width
                    scale_y = quadrant_sizes[idx][1] / original_height
                    for cls, original_box in zip(original_classes, original_boxes):
                        labels.append([cls, [pos[0] + scale_x * original_box[0], pos[1] + scale_y * original_box[1],
                                             pos[0] + scale_x * original_box[2], pos[1] + scale_y * original_box[3]]])
                        box_count += 1
                        if box_count >= MAX_BOXES_PER_COLLAGE:
                            break                                     # (leaves the inner loop only, as in the reference)
                job(level + 1, part, OUT - n, x_offset, 0, img_w, img_h, collage_width, collage_height)
            else:
                job(level, src, OUT - n, x_offset, 0, img_w, img_h, collage_width, collage_height, op, arg)
                scale_x = img_w / original_width
                scale_y = img_h / original_height
                for cls, original_box in zip(original_classes, original_boxes):
                    labels.append([cls, [x_offset + scale_x * original_box[0], scale_y * original_box[1],
                                         x_offset + scale_x * original_box[2], scale_y * original_box[3]]])
                    box_count += 1
                    if box_count >= MAX_BOXES_PER_COLLAGE:
                        break
            x_offset += img_w
        labels_all.append(labels)
        n += 1
    T = len(tmp_wh)

    def plane(p):
        if isinstance(p, tuple):
            return p[1] if p[0] == "s" else S + p[1]
        return S + T + (OUT - p)

    jobs = [(lv, plane(s), plane(d)) + tuple(rest if manual_augmentations else rest[:4]) for lv, s, d, *rest in jobs]
    return CollagePlan(crops, tmp_wh, jobs, n, collage_height, collage_width, labels_all, crop_boxes, crop_classes, params, noise, augment)


def _call_arrays(who, src_planes, tmp_wh, n, height, width, jobs, columns):
    planes = [np.ascontiguousarray(p, np.uint8) for p in src_planes]
    for i, p in enumerate(planes):
        if p.ndim != 3 or p.shape[2] != 3:
            raise ValueError("%s: source plane %d has shape %s, [h, w, 3] is taken" % (who, i, p.shape))
    src_wh = np.asarray([(p.shape[1], p.shape[0]) for p in planes], np.int32).reshape(-1, 2)
    pix = np.concatenate([p.reshape(-1) for p in planes]) if planes else np.zeros(0, np.uint8)
    tmp = np.ascontiguousarray(np.asarray(tmp_wh, np.int32).reshape(-1, 2))
    jobs = np.ascontiguousarray(np.asarray(jobs, np.int32).reshape(-1, columns))
    if n < 1 or height < 1 or width < 1:
        raise ValueError("%s: %d output planes of %d x %d" % (who, n, width, height))
    out = np.empty((int(n), int(height), int(width), 3), np.uint8)          # (the call writes all of it, or fails)
    return planes, src_wh, pix, tmp, jobs, out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def resample_np(src_planes, tmp_wh, n, height, width, jobs, device=0):
    """uda_resample_np: src_planes a list of uint8 arrays [h, w, 3]; tmp_wh [(w, h)]; jobs [K, 7] int32 (include/uda_hip.h).
    Returns the n output planes [n, height, width, 3] uint8."""
    planes, src_wh, pix, tmp, jobs, out = _call_arrays("resample_np", src_planes, tmp_wh, n, height, width, jobs, 7)
    lib = capi.load()
    rc = lib.uda_resample_np(int(device), len(planes), _ptr(src_wh), _ptr(pix), len(tmp), _ptr(tmp), int(n), int(height), int(width),
                             len(jobs), _ptr(jobs), out.ctypes.data_as(C.c_void_p))
    capi.check(lib, None, rc, "uda_resample_np")
    return out


def collage_np(src_planes, tmp_wh, n, height, width, jobs, params=(), noise=None, device=0):
    """uda_collage_np: as `resample_np` with jobs [K, 9] int32 (.., op, arg), params the doubles the ops 2-4 index and noise the
    uint8 bytes of the op-5 jobs in job-list order (include/uda_hip.h).  Returns the n output planes [n, height, width, 3] uint8."""
    planes, src_wh, pix, tmp, jobs, out = _call_arrays("collage_np", src_planes, tmp_wh, n, height, width, jobs, 9)
    params = np.ascontiguousarray(np.asarray(params, np.float64).reshape(-1))
    noise = np.zeros(0, np.uint8) if noise is None else np.ascontiguousarray(np.asarray(noise, np.uint8).reshape(-1))
    lib = capi.load()
    rc = lib.uda_collage_np(int(device), len(planes), _ptr(src_wh), _ptr(pix), len(tmp), _ptr(tmp), int(n), int(height), int(width),
                            len(jobs), _ptr(jobs), len(params), _ptr(params), noise.size, _ptr(noise), out.ctypes.data_as(C.c_void_p))
    capi.check(lib, None, rc, "uda_collage_np")
    return out


def gauss_box(radius):
    """uda_gauss_box_np (host only): Pillow's box blur behind GaussianBlur(radius) -> (fr float32, ww, fw)."""
    lib = capi.load()
    fr, ww, fw = C.c_float(), C.c_uint32(), C.c_uint32()
    capi.check(lib, None, lib.uda_gauss_box_np(float(radius), C.byref(fr), C.byref(ww), C.byref(fw)), "uda_gauss_box_np")
    return np.float32(fr.value), ww.value, fw.value


def augment_np(plane, kind, value=None, noise=None, device=0):
    """One augmentation of one plane [h, w, 3] uint8 on the device: kind one of AUGMENT_KINDS; value the factor (brightness,
    contrast) or the radius (blur); noise a uint8 array of the plane's shape (noise).  Returns the augmented plane."""
    plane = np.ascontiguousarray(plane, np.uint8)
    if kind not in AUGMENT_KINDS:
        raise ValueError("augment_np: kind %r, one of %s is taken" % (kind, AUGMENT_KINDS))
    op = AUGMENT_KINDS.index(kind) + 1
    if op in (OP_BRIGHTNESS, OP_CONTRAST, OP_BLUR) and value is None:
        raise ValueError("augment_np: %s takes a value" % kind)
    if op == OP_NOISE and (noise is None or np.shape(noise) != plane.shape):
        raise ValueError("augment_np: noise takes a uint8 array of the plane's shape")
    h, w = plane.shape[:2]
    return collage_np([plane], [], 1, h, w, [(0, 0, 1, 0, 0, w, h, op, 0)], [value] if value is not None else [],
                      noise if op == OP_NOISE else None, device=device)[0]


def apply_manual_augmentation(image, boxes, rng=None, device=0):
    """The reference's Parent_SSL.apply_manual_augmentation (parent.py:261-315) on an array [h, w, 3] uint8: one of the five
    augmentations drawn from `rng` (None: numpy's global legacy stream, as the reference), run on the device.  A flip rewrites
    `boxes` ([[x1, y1, x2, y2], ...]) in place, as the reference does.  Returns (image, boxes)."""
    rng = np.random if rng is None else rng
    image = np.ascontiguousarray(image, np.uint8)
    h, w = image.shape[:2]
    kind = AUGMENT_KINDS[int(rng.choice(5))]
    value = noise = None
    if kind == "flip":
        for box in boxes:
            box[0], box[2] = w - box[2], w - box[0]
    elif kind in ("brightness", "contrast"):
        value = float(rng.uniform(0.7, 1.3))
    elif kind == "blur":
        value = float(rng.uniform(1, 3))
    else:
        noise = rng.randint(5, 20, (h, w, 3), dtype="uint8")
    return augment_np(image, kind, value, noise, device=device), boxes


def resample_coeffs(in_size, out_size):
    """uda_resample_coeffs_np (host only): Pillow's 8-bit Lanczos table of one axis -> (ksize, bounds [out, 2], coeffs [out, ksize])."""
    lib = capi.load()
    ks = C.c_int32()
    capi.check(lib, None, lib.uda_resample_coeffs_np(int(in_size), int(out_size), C.byref(ks), None, None, 0), "uda_resample_coeffs_np")
    bounds = np.zeros((int(out_size), 2), np.int32)
    coeffs = np.zeros((int(out_size), ks.value), np.int32)
    capi.check(lib, None, lib.uda_resample_coeffs_np(int(in_size), int(out_size), C.byref(ks), bounds.ctypes.data_as(C.c_void_p),
                                                     coeffs.ctypes.data_as(C.c_void_p), coeffs.size), "uda_resample_coeffs_np")
    return ks.value, bounds, coeffs


class Collage:
    """images [N, H, W, 3] uint8; labels: per collage [[class, [x1, y1, x2, y2]], ...]; plan: the CollagePlan behind them."""

    def __init__(self, images, labels, plan=None):
        self.images, self.labels, self.plan = images, labels, plan

    def __len__(self):
        return len(self.labels)


def crop_collage(images, classes, boxes, target_class, dataset="KITTI", scale=False, low_scale=0.5, high_scale=1.0, rng=None, sizes=None,
                 resample=None, device=0, manual_augmentations=False, **not_built):
    """The reference's crop_collage up to the collages and their labels.

    images: per image a uint8 array [h, w, 3] or a path; with paths only the images that contribute a crop are decoded
    (infer_lib.read_images), and `sizes` [(width, height)] may spare opening the others for their size.  classes / boxes /
    target_class / dataset / scale / low_scale / high_scale / rng: as `plan_collage`.  resample: another implementation of
    `resample_np` (same arguments; the tests pass a numpy mirror) - with manual_augmentations of `collage_np`, which is then
    called with the plan's [K, 9] jobs, params and noise.  Returns a Collage."""
    _refuse(not_built)
    images = list(images)
    if sizes is None:
        sizes = []
        for im in images:
            if isinstance(im, (str, os.PathLike)):
                from PIL import Image
                with Image.open(im) as f:
                    sizes.append(f.size)
            else:
                sizes.append(_size(np.asarray(im)))
    plan = plan_collage(sizes, classes, boxes, target_class, dataset, scale, low_scale, high_scale, rng, manual_augmentations)
    used = plan.images_used()
    paths = [i for i in used if isinstance(images[i], (str, os.PathLike))]
    decoded = {}
    if paths:
        from . import infer_lib
        decoded = dict(zip(paths, infer_lib.read_images([images[i] for i in paths])))
    pixels = {i: decoded[i] if i in decoded else np.asarray(images[i], np.uint8) for i in used}
    planes = [pixels[i][y0:y1, x0:x1] for i, x0, y0, x1, y1 in plan.crops]
    if plan.n == 0:
        return Collage(np.zeros((0, plan.height, plan.width, 3), np.uint8), [], plan)
    args = (planes, plan.tmp_wh, plan.n, plan.height, plan.width, plan.jobs) + ((plan.params, plan.noise) if manual_augmentations else ())
    run = resample or (collage_np if manual_augmentations else resample_np)
    out = run(*args, **({} if resample else {"device": device}))
    return Collage(out, plan.labels, plan)


def gt_inputs(names, dataset, used_classes, labels_folder=None, items=None):
    """gt=True (parent.py:358-373): the annotations of the labelled images through the readers of pseudo_audit.py ->
    (classes, boxes) per image.  KITTI: labels_folder holds <name> for every name; BDD100K: items is the loaded label json."""
    from . import pseudo_audit
    classes, boxes = [], []
    for name in names:
        if dataset == "KITTI":
            objs = pseudo_audit.read_kitti_annotations(os.path.join(labels_folder, name), used_classes)
        else:
            objs = pseudo_audit.read_bdd_annotations(items, name, used_classes)
        classes.append(np.asarray([o["class"] for o in objs]))
        boxes.append(np.asarray([o["bbox"] for o in objs]))
    return classes, boxes


def pseudo_inputs(selected, class_names, filter_ims=None):
    """gt=False (parent.py:375-379): selected = (names, classes, boxes[, scores]) as `PseudoLabelSet.finalize` or the prediction
    readers give them (class ids, boxes y1 x1 y2 x2 - pass dataset="BDD100K"-style order on, or reorder for KITTI);
    class_names {id: name}.  filter_ims keeps image i where filter_ims[i] is true - it filters the NAMES only, as the reference
    does: classes and boxes stay indexed by position.  Returns (names, classes, boxes)."""
    names = list(selected[0])
    if filter_ims is not None:
        names = [nm for nm, keep in zip(names, filter_ims) if keep]
    classes = [np.asarray([class_names[int(c)] for c in c_im]) for c_im in selected[1]]
    return names, classes, [np.asarray(b, np.float64) for b in selected[2]]


def kitti_label_text(labels):
    return "".join("%s 0.0 0 0 %s %s %s %s 0 0 0 0 0 0 0\n" % (cls, box[0], box[1], box[2], box[3]) for cls, box in labels)


def bdd_label_items(labels_per_collage):
    """The list the reference dumps: one item per collage and, after every collage but the first, its stray ",\\n" string."""
    data = []
    for i, labels in enumerate(labels_per_collage):
        items = [{"id": str(i) + str(d_i), "attributes": {"occluded": False, "truncated": False}, "category": cls,
                  "box2d": {"x1": box[0], "x2": box[2], "y1": box[1], "y2": box[3]}} for d_i, (cls, box) in enumerate(labels)]
        data.append({"name": "collage_%d.jpg" % i, "attributes": {"weather": "clear", "timeofday": "daytime", "scene": "city street"},
                     "timestamp": 10000, "labels": items})
        if i:
            data.append(",\n")
    return data


def bdd_label_text(labels_per_collage):
    return json.dumps(bdd_label_items(labels_per_collage), indent=4)


def write_kitti_collage(save_path, collage, **not_built):
    """parent.py:600-608: {10000 + i:06}.png and .txt per collage.  Returns the number of collages."""
    _refuse(not_built)
    from PIL import Image
    os.makedirs(save_path, exist_ok=True)
    for i, labels in enumerate(collage.labels):
        stem = os.path.join(save_path, "%06d" % (10000 + i))
        Image.fromarray(collage.images[i]).save(stem + ".png")
        with open(stem + ".txt", "w") as f:
            f.write(kitti_label_text(labels))
    return len(collage.labels)


def write_bdd_collage(save_path, collage, **not_built):
    """parent.py:609-667: collage_{i}.jpg per collage and bdd100k_labels_images_train.json.  Returns the number of collages."""
    _refuse(not_built)
    from PIL import Image
    os.makedirs(save_path, exist_ok=True)
    for i in range(len(collage.labels)):
        Image.fromarray(collage.images[i]).save(os.path.join(save_path, "collage_%d.jpg" % i))
    with open(os.path.join(save_path, "bdd100k_labels_images_train.json"), "w") as f:
        f.write(bdd_label_text([[[str(cls), [float(v) for v in box]] for cls, box in labels] for labels in collage.labels]))
    return len(collage.labels)
