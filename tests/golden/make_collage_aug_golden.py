"""Generates tests/golden/collage_aug_golden.npz by running the REAL reference method `Parent_SSL.crop_collage` with
manual_augmentations=True (src/ssl_utils/parent.py:317-686; the augmentations: 261-315, applied at 534-537) on tiny synthetic
images.  Run once where a checkout of the reference exists; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_collage_aug_golden.py <src directory of the reference's checkout>

The method is reached the way make_collage_golden.py reaches it, whose stubs, images, design and runner are imported from there:
the heavy imports stubbed, the object made with `__new__`, KITTI collages read back from the PNGs, BDD100K collages captured
before JPEG encoding.  The images are that golden's five (the same generator in the same order) plus EXTRA ones placed before
the last, which stays the image without a target box that gives the collages their size.  The extra images are there so that
the reference's own draws (seed 42, np.random.choice of the five augmentations per packed crop) show every kind: main() asserts,
from a tap on np.random.choice and on apply_manual_augmentation, that flip, brightness, contrast, blur and noise each occur in
every run, and that a flipped crop carries a box.

Runs: KITTI and BDD100K, each with scale False and True, from pseudo-label style lists (gt=False).

Recorded: the decoded input images, classes and boxes, the target classes, per run the collage pixels and the label texts, the
kinds drawn, Pillow's and numpy's versions."""
import os
import sys
import tempfile

sys.dont_write_bytecode = True          # never write into the reference's checkout
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_collage_golden as M          # noqa: E402  (checks the command line, stubs the heavy imports, imports the reference module)
import numpy as np                       # noqa: E402
import PIL                               # noqa: E402
from PIL import Image                    # noqa: E402

P = M.P
KINDS = ("flip", "brightness", "contrast", "blur", "noise")
EXTRA_SIZES = [(80, 64), (96, 72)]
SIZES = M.SIZES[:-1] + EXTRA_SIZES + M.SIZES[-1:]


def design():
    """per image [(slot, [x1, y1, x2, y2])]: the first golden's design with the extra images before its last one"""
    extra = [
        # a target with a car inside its crop, a second small target
        [("t0", [20.0, 20.0, 50.0, 44.0]), ("o0", [24.0, 24.0, 40.0, 40.0]), ("t1", [60.0, 6.0, 70.0, 30.0])],
        # two targets side by side with a pedestrian between them, a target in the corner
        [("t1", [10.0, 30.0, 28.0, 60.0]), ("o1", [26.0, 34.0, 32.0, 50.0]), ("t0", [30.0, 28.0, 66.0, 52.0]), ("t0", [80.0, 56.0, 96.0, 72.0])],
    ]
    d = M.design()
    return d[:-1] + extra + d[-1:]


class ChoiceTap:
    """Wraps np.random.choice: records which of the five augmentations the reference drew (the index of the function in its
    list), and what apply_manual_augmentation was given and returned (boxes before and after)."""

    def __init__(self):
        self.kinds, self.boxes = [], []
        self.orig_choice = np.random.choice
        self.orig_apply = P.Parent_SSL.apply_manual_augmentation

    def __enter__(self):
        tap = self

        def choice(a, *args, **kw):
            got = tap.orig_choice(a, *args, **kw)
            if isinstance(a, list) and len(a) == 5 and callable(a[0]):
                tap.kinds.append(KINDS[[f is got for f in a].index(True)])
            return got

        def apply(image, boxes):
            before = [[float(v) for v in b] for b in boxes]
            image, boxes = tap.orig_apply(image, boxes)
            tap.boxes.append((before, [[float(v) for v in b] for b in boxes], image.width))
            return image, boxes
        np.random.choice = choice
        P.Parent_SSL.apply_manual_augmentation = staticmethod(apply)
        return self

    def __exit__(self, *exc):
        np.random.choice = self.orig_choice
        P.Parent_SSL.apply_manual_augmentation = staticmethod(self.orig_apply)


def run(o, dataset, list_classes, list_boxes, save_path, scale):
    with M.SaveTap() as tap:
        o.crop_collage(list_classes, list_boxes, target_class=M.TARGET[dataset], save_path=save_path, gt=False, scale=scale,
                       manual_augmentations=True)
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
           "kitti_classes": np.array(M.KITTI), "bdd_classes": np.array(M.BDD), "sizes": np.asarray(SIZES)}
    n = len(SIZES)
    stems = ["%06d" % (7 * i + 3) for i in range(n)]
    made = [M.make_image(rng, w, h) for w, h in M.SIZES] + [M.make_image(rng, w, h) for w, h in EXTRA_SIZES]      # the first golden's five first
    base = made[:len(M.SIZES) - 1] + made[len(M.SIZES):] + [made[len(M.SIZES) - 1]]
    assert [(im.shape[1], im.shape[0]) for im in base] == SIZES
    with tempfile.TemporaryDirectory(prefix="collage_aug_") as td:
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
            classes = [np.asarray([M.SLOT[dataset][s] for s, _ in im]) for im in design()]
            xyxy = [np.asarray([b for _, b in im], np.float64) for im in design()]
            boxes = xyxy if dataset == "KITTI" else [b[:, [1, 0, 3, 2]] for b in xyxy]      # BDD lists hold y1 x1 y2 x2
            out[key + "classes"] = np.concatenate(classes)
            out[key + "boxes"] = np.concatenate(boxes)
            out[key + "counts"] = np.asarray([len(c) for c in classes])
            out[key + "target"] = np.array(M.TARGET[dataset])
            out[key + "stems"] = np.array(stems)
            o = P.Parent_SSL.__new__(P.Parent_SSL)
            o.dataset, o.used_classes, o.general_path = dataset, M.KITTI if dataset == "KITTI" else M.BDD, general
            o.gt_images_folder, o.images_data = img_dir, [s + "." + fmt for s in stems]
            o.labeled_indices, o.added_name = list(range(n)), "num_labeled_10"
            if dataset == "KITTI":
                with open(os.path.join(general, "datasets", "KITTI", "vaL_index_list.txt"), "w") as f:
                    f.write("1\n2\n")
            for scale in (False, True):
                save_path = os.path.join(general, "datasets", dataset, "collage_crops", "num_labeled_10", "rcc_aug_%d" % scale) + "/"
                with ChoiceTap() as tap:
                    pixels, texts = run(o, dataset, [c.copy() for c in classes], [b.copy() for b in boxes], save_path, scale)
                tag = key + ("scale_" if scale else "plain_")
                out[tag + "pixels"], out[tag + "texts"], out[tag + "kinds"] = pixels, np.array(texts), np.array(tap.kinds)
                print(dataset, "scale", scale, pixels.shape, tap.kinds)
                assert pixels.shape[1:] == (SIZES[-1][1], SIZES[-1][0], 3) and len(pixels) > 1
                # what the reference's own draws must show
                assert set(tap.kinds) == set(KINDS), "a kind is missing: add images to the design"
                assert len(tap.kinds) == len(tap.boxes)
                flipped = [(b, a, w) for k, (b, a, w) in zip(tap.kinds, tap.boxes) if k == "flip" and len(b)]
                assert flipped, "no flipped crop carries a box: add images to the design"
                for before, after, width in flipped:                  # the flip rewrote the boxes with the resized width
                    assert all(a[0] == width - b[2] and a[2] == width - b[0] and a[1] == b[1] for b, a in zip(before, after))
    dst = os.path.join(HERE, "collage_aug_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) <= 700000                           # noise and blur compress badly; far below the 1 MiB a committed file may have


if __name__ == "__main__":
    main()
