"""Generates tests/golden/collage_golden.npz by running the REAL reference method `Parent_SSL.crop_collage`
(src/ssl_utils/parent.py:317-686) on tiny synthetic images written to a temporary directory.  Run once where a checkout of the
reference exists; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_collage_golden.py <src directory of the reference's checkout>

How the method is reached: as make_audit_golden.py reaches Parent_SSL - the heavy imports (tensorflow and friends, cv2, seaborn,
ijson, skimage, sklearn, aug, the TFRecord creators) are stubbed, `ssl_utils.parent` is imported and the object is made with
`__new__` and given the attributes the constructor would have set.  `kitti_custom_to_tfrecords`, `bdd_custom_to_tfrecords` and
`generate_commands_and_create_dirs` are stubbed in the module's namespace.  KITTI collages are read back from the PNGs the method
writes; BDD100K collages are captured before JPEG encoding by wrapping `Image.Image.save`.

Runs: KITTI and BDD100K, each with scale False and True, from pseudo-label style lists (gt=False), and KITTI scale False once
more with gt=True from label files holding the same boxes.  What is planted is asserted in main(): a crop that overshoots (the
second resize), the last crop taking the remaining width, more than one collage, a box dropped by the `> 2` filter whose class
stays (the lists differ in length), and a last image without target boxes whose size differs from the others'.

Recorded: the decoded input images, classes and boxes, the target classes, per run the collage pixels and the label texts,
Pillow's and numpy's versions.  All coordinates are multiples of 1/8."""
import json
import os
import sys
import tempfile
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_collage_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
for name in ("tensorflow", "tensorflow_probability", "uncertainty_toolbox", "uncertainty_toolbox.viz", "cv2", "seaborn", "ijson", "skimage", "aug",
             "aug.autoaugment", "datasets", "datasets.BDD100K", "datasets.BDD100K.bdd_tf_creator", "datasets.KITTI",
             "datasets.KITTI.kitti_tf_creator", "sklearn", "sklearn.metrics"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
import numpy as np                       # noqa: E402
import PIL                               # noqa: E402
from PIL import Image                    # noqa: E402
import ssl_utils.parent as P             # noqa: E402  (the reference module)

P.kitti_custom_to_tfrecords = lambda *a, **k: None
P.bdd_custom_to_tfrecords = lambda *a, **k: None
P.generate_commands_and_create_dirs = lambda *a, **k: None

KITTI = ["Car", "Van", "Truck", "Pedestrian", "Person_sitting", "Cyclist", "Tram"]
BDD = ["pedestrian", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle", "traffic light", "traffic sign"]
TARGET = {"KITTI": ["Person_sitting", "Tram"], "BDD100K": ["train", "rider", "motorcycle", "bicycle"]}
# class slots of the design below -> names: t0 / t1 are target classes, o0 / o1 are not
SLOT = {"KITTI": {"t0": "Tram", "t1": "Person_sitting", "o0": "Car", "o1": "Pedestrian"},
        "BDD100K": {"t0": "train", "t1": "rider", "o0": "car", "o1": "traffic light"}}
SIZES = [(96, 64), (96, 64), (90, 70), (96, 64), (100, 60)]      # (width, height); the last image has no target box


def design():
    """per image [(slot, [x1, y1, x2, y2])]"""
    return [
        # 0: a wide target near the top (its crop is clamped to y = 0 whatever the margin), a car inside its crop, and FIRST in the
        #    list a pedestrian 1.5 px high at the top: its class is carried, its box is dropped by the `> 2` filter, so the classes
        #    [Pedestrian, Tram, Car] are zipped with the boxes [tram, car]
        [("o1", [40.0, 0.0, 50.0, 1.5]), ("t0", [30.0, 4.0, 60.0, 16.0]), ("o0", [36.0, 6.0, 50.0, 14.0]), ("o0", [70.0, 40.0, 90.0, 60.0])],
        # 1: two targets whose crops hold each other; one at the image's corner (clamped)
        [("t1", [0.0, 0.0, 12.0, 20.0]), ("t0", [8.0, 10.0, 30.0, 40.0]), ("o0", [80.0, 50.0, 95.0, 63.0])],
        # 2: a tall narrow target, a box larger than its crop on both sides (not "overlapping" by the reference's test)
        [("t1", [40.125, 20.0, 46.5, 50.25]), ("o0", [10.0, 5.0, 85.0, 68.0]), ("t0", [60.0, 30.0, 80.0, 45.0])],
        # 3: fractional boxes; crops whose int(round()) box rounds half to even
        [("t0", [10.5, 10.5, 30.5, 25.5]), ("o1", [14.0, 12.0, 20.0, 22.0]), ("t1", [50.0, 8.0, 58.0, 30.0]), ("o0", [52.0, 10.0, 57.0, 29.0])],
        # 4: no target class
        [("o0", [5.0, 5.0, 40.0, 40.0]), ("o1", [50.0, 10.0, 56.0, 30.0])],
    ]


def make_image(rng, w, h):
    """Smooth colour ramps, a 0 / 255 checkerboard patch, single bright pixels and a little noise."""
    y, x = np.mgrid[0:h, 0:w]
    im = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 255 // (w + h - 2))], -1).astype(np.int64)
    im += rng.integers(-6, 7, im.shape)
    im = np.clip(im, 0, 255).astype(np.uint8)
    im[h // 4:h // 2, w // 3:w // 2] = (((y + x) % 2) * 255)[h // 4:h // 2, w // 3:w // 2, None]
    for _ in range(12):
        im[rng.integers(0, h), rng.integers(0, w)] = 255 if rng.random() < 0.5 else 0
    return im


class SaveTap:
    """Wraps Image.Image.save: keeps the pixels of every collage_*.jpg before the JPEG encoder sees them."""

    def __init__(self):
        self.taken = {}
        self.orig = Image.Image.save

    def __enter__(self):
        tap = self

        def save(im, fp, *a, **k):
            if isinstance(fp, str) and os.path.basename(fp).startswith("collage_"):
                tap.taken[os.path.basename(fp)] = np.array(im)
            return tap.orig(im, fp, *a, **k)
        Image.Image.save = save
        return self

    def __exit__(self, *exc):
        Image.Image.save = self.orig


def run(o, dataset, list_classes, list_boxes, save_path, scale, gt):
    with SaveTap() as tap:
        o.crop_collage(list_classes, list_boxes, target_class=TARGET[dataset], save_path=save_path, gt=gt, scale=scale)
    files = sorted(os.listdir(save_path))
    if dataset == "KITTI":
        pngs = [f for f in files if f.endswith(".png")]
        pixels = np.stack([np.array(Image.open(save_path + f).convert("RGB")) for f in pngs])
        texts = [open(save_path + f[:-4] + ".txt").read() for f in pngs]
        assert pngs == ["%06d.png" % (10000 + i) for i in range(len(pngs))]
    else:
        n = len(tap.taken)
        pixels = np.stack([tap.taken["collage_%d.jpg" % i] for i in range(n)])
        texts = [open(save_path + "bdd100k_labels_images_train.json").read()]
    return pixels, texts


def main():
    rng = np.random.default_rng(20241021)
    out = {"numpy_version": np.array([np.__version__]), "pillow_version": np.array([PIL.__version__]),
           "kitti_classes": np.array(KITTI), "bdd_classes": np.array(BDD), "sizes": np.asarray(SIZES)}
    n = len(SIZES)
    stems = ["%06d" % (7 * i + 3) for i in range(n)]
    base = [make_image(rng, w, h) for w, h in SIZES]
    with tempfile.TemporaryDirectory(prefix="collage_") as td:
        general = os.path.join(td, "general")
        for dataset in ("KITTI", "BDD100K"):
            key = "kitti_" if dataset == "KITTI" else "bdd_"
            fmt = "png" if dataset == "KITTI" else "jpg"
            img_dir = os.path.join(general, "datasets", dataset, "images")
            os.makedirs(img_dir)
            images = []
            for stem, im in zip(stems, base):
                path = os.path.join(img_dir, stem + "." + fmt)
                Image.fromarray(im).save(path, **({} if fmt == "png" else {"quality": 90}))
                images.append(np.array(Image.open(path).convert("RGB")))
                out[key + "image_" + stem] = images[-1]
            assert (dataset != "KITTI") or all(np.array_equal(a, b) for a, b in zip(images, base))
            classes = [np.asarray([SLOT[dataset][s] for s, _ in im]) for im in design()]
            xyxy = [np.asarray([b for _, b in im], np.float64) for im in design()]
            for b in xyxy:
                assert (b * 8 == np.round(b * 8)).all()
            boxes = xyxy if dataset == "KITTI" else [b[:, [1, 0, 3, 2]] for b in xyxy]      # BDD lists hold y1 x1 y2 x2
            out[key + "classes"] = np.concatenate(classes)
            out[key + "boxes"] = np.concatenate(boxes)
            out[key + "counts"] = np.asarray([len(c) for c in classes])
            out[key + "target"] = np.array(TARGET[dataset])
            out[key + "stems"] = np.array(stems)
            o = P.Parent_SSL.__new__(P.Parent_SSL)
            o.dataset, o.used_classes, o.general_path = dataset, KITTI if dataset == "KITTI" else BDD, general
            o.gt_images_folder, o.images_data = img_dir, [s + "." + fmt for s in stems]
            o.labeled_indices, o.added_name = list(range(n)), "num_labeled_10"
            if dataset == "KITTI":
                with open(os.path.join(general, "datasets", "KITTI", "vaL_index_list.txt"), "w") as f:
                    f.write("1\n2\n")
            for scale in (False, True):
                save_path = os.path.join(general, "datasets", dataset, "collage_crops", "num_labeled_10", "rcc_%d" % scale) + "/"
                pixels, texts = run(o, dataset, [c.copy() for c in classes], [b.copy() for b in boxes], save_path, scale, False)
                tag = key + ("scale_" if scale else "plain_")
                out[tag + "pixels"], out[tag + "texts"] = pixels, np.array(texts)
                print(dataset, "scale", scale, pixels.shape)
                assert pixels.shape[1:] == (SIZES[-1][1], SIZES[-1][0], 3) and len(pixels) > 1      # the last image's size; several collages
            if dataset == "KITTI":
                # gt=True: the same boxes from label files
                lab_dir = os.path.join(general, "datasets", "KITTI", "training", "label_2")
                os.makedirs(lab_dir)
                label_texts = []
                for stem, c_im, b_im in zip(stems, classes, boxes):
                    text = "".join("%s 0.0 0 -1.5 %r %r %r %r 1 1 3 1 1 20 -1\n" % (c, float(b[0]), float(b[1]), float(b[2]), float(b[3]))
                                   for c, b in zip(c_im, b_im)) + "DontCare -1 -1 -10 5.00 6.00 7.00 8.00 -1 -1 -1 -1000 -1000 -1000 -10\n"
                    label_texts.append(text)
                    with open(os.path.join(lab_dir, stem + ".txt"), "w") as f:
                        f.write(text)
                out["kitti_label_files"] = np.array(label_texts)
                o.gt_labels_folder, o.labeled_imnames = lab_dir, ["x/y/" + s + ".txt" for s in stems]
                save_path = os.path.join(general, "datasets", "KITTI", "collage_crops", "num_labeled_10", "rcc_gt") + "/"
                pixels, texts = run(o, "KITTI", [], [], save_path, False, True)
                assert np.array_equal(pixels, out["kitti_plain_pixels"]) and texts == list(out["kitti_plain_texts"])
    # what is planted
    text0 = "".join(str(t) for t in out["kitti_plain_texts"])
    assert "Pedestrian" in text0                                    # the class of the box the `> 2` filter dropped is carried
    assert json.loads(str(out["bdd_plain_texts"][0]))[2] == ",\n"   # the stray list item after the second collage
    dst = os.path.join(HERE, "collage_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) <= 534274                           # no larger than the largest golden committed before it


if __name__ == "__main__":
    main()
