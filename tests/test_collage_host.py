"""The collage service without a GPU: the numpy mirror (tests/collage_ref.py) against live Pillow, the library's host-only
coefficient tables against the mirror's, the planner against the golden of the REAL `Parent_SSL.crop_collage`
(tests/golden/make_collage_golden.py), the argument errors of both entry points, the no-device message and the options that are
not built.  Pixels are compared for equality: Pillow's 8-bit resize is integer arithmetic on coefficient tables."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import collage_ref as R
from common import ROOT
from uda_amd import capi, collage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collage_golden.npz")
RUNS = [("kitti_", "KITTI", False), ("kitti_", "KITTI", True), ("bdd_", "BDD100K", False), ("bdd_", "BDD100K", True)]
# (source w, h) -> (w, h): enlarging, shrinking, a pass skipped in turn, a copy, ksize far above a tile, 1 x N sources,
# the vertical-first rule
EDGES = [((3, 3), (7, 5)), ((9, 6), (9, 13)), ((9, 6), (4, 6)), ((9, 6), (9, 6)), ((70, 1), (1, 1)), ((1, 70), (1, 1)), ((70, 70), (1, 3)),
         ((70, 70), (3, 1)), ((1, 9), (5, 9)), ((1, 9), (4, 20)), ((9, 1), (20, 4)), ((1, 1), (6, 6)), ((33, 31), (32, 33)), ((200, 3), (7, 3)),
         # Image.resize's own rule: more than 100 times as tall as wide and getting shorter -> along y first (either side of the rule)
         ((4, 401), (3, 300)), ((4, 400), (3, 300)), ((4, 401), (6, 300)), ((4, 401), (3, 802)), ((4, 401), (3, 400)), ((2, 201), (1, 1)),
         ((7, 720), (6, 540)), ((7, 720), (2, 180))]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.load()


def pattern(kind, w, h, seed=0):
    rng = np.random.default_rng([seed, w, h])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "checker":                      # 0 / 255: negative accumulators and overshoot above 255
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) % 2) * 255).astype(np.uint8)[:, :, None], 3, 2)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    im = np.zeros((h, w, 3), np.uint8)         # single bright pixels
    for _ in range(max(1, w * h // 16)):
        im[rng.integers(0, h), rng.integers(0, w), rng.integers(0, 3)] = 255
    return im


KINDS = ("noise", "checker", "binary", "dots")


def golden_case(g, key):
    """-> (images, classes, boxes, target) of a dataset of the golden."""
    stems = [str(s) for s in g[key + "stems"]]
    off = np.concatenate([[0], np.cumsum(g[key + "counts"])])
    images = [g[key + "image_" + s] for s in stems]
    classes = [g[key + "classes"][a:b] for a, b in zip(off[:-1], off[1:])]
    boxes = [g[key + "boxes"][a:b] for a, b in zip(off[:-1], off[1:])]
    return images, classes, boxes, [str(t) for t in g[key + "target"]]


def golden_texts(got, g, key, scale):
    tag = key + ("scale_" if scale else "plain_")
    want = [str(t) for t in g[tag + "texts"]]
    if key == "kitti_":
        assert [collage.kitti_label_text(l) for l in got.labels] == want
    else:
        assert [collage.bdd_label_text(got.labels)] == want


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_mirror_equals_live_pillow_sweep():
    rng = np.random.default_rng(7)
    for i in range(60):
        w, h, W, H = (int(v) for v in rng.integers(1, 48, 4))
        if i % 5 == 0:
            W = w
        if i % 7 == 0:
            H = h
        img = pattern(KINDS[i % 4], w, h, i)
        assert np.array_equal(R.resize(img, W, H), R.pillow_resize(img, W, H)), (i, w, h, W, H)


@pytest.mark.parametrize("src,dst", EDGES)
def test_mirror_equals_live_pillow_edges(src, dst):
    for kind in KINDS:
        img = pattern(kind, *src)
        assert np.array_equal(R.resize(img, *dst), R.pillow_resize(img, *dst)), kind


@pytest.mark.parametrize("n_in,n_out", [(3, 7), (7, 3), (70, 1), (1, 9), (5, 5), (100, 37), (37, 100), (64, 375), (300, 720), (1280, 31)])
def test_library_coefficients_equal_the_mirror(lib, n_in, n_out):
    ksize, bounds, kk = collage.resample_coeffs(n_in, n_out)
    r_ksize, r_bounds, r_kk = R.coeffs(n_in, n_out)
    assert ksize == r_ksize and kk.shape == (n_out, ksize)
    assert np.array_equal(bounds, r_bounds)
    assert np.array_equal(kk, r_kk)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (np.diff(bounds[:, 0]) >= 0).all()


def test_coefficient_argument_errors(lib):
    ks = C.c_int32()
    b, k = np.zeros((4, 2), np.int32), np.zeros((4, 7), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    for args, word in (((0, 4, C.byref(ks), None, None, 0), "1.."), ((4, 0, C.byref(ks), None, None, 0), "1.."),
                       ((4, capi.RESAMPLE_MAX_SIDE + 1, C.byref(ks), None, None, 0), "1.."), ((4, 4, None, None, None, 0), "NULL ksize"),
                       ((3, 4, C.byref(ks), p(b), None, 0), "go together"), ((3, 4, C.byref(ks), p(b), p(k), 27), "are needed")):
        assert lib.uda_resample_coeffs_np(*args) == 1
        msg = lib.uda_last_error(None).decode()
        assert msg.startswith("uda_resample_coeffs_np: ") and word in msg, msg
    assert not b.any() and not k.any()


def _call(lib, src, tmp_wh, n, h, w, jobs, out=None):
    src_wh = np.asarray([(s.shape[1], s.shape[0]) for s in src], np.int32).reshape(-1, 2)
    pix = np.concatenate([s.reshape(-1) for s in src]) if src else np.zeros(1, np.uint8)
    tmp = np.asarray(tmp_wh, np.int32).reshape(-1, 2)
    jobs = np.asarray(jobs, np.int32).reshape(-1, 7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    return lib.uda_resample_np(0, len(src), p(src_wh), p(pix), len(tmp), p(tmp) if len(tmp) else None, n, h, w, len(jobs), p(jobs),
                               None if out is None else p(out))


def test_resample_argument_errors(lib):
    """Every refusal comes before the device is touched, names the entry point, and leaves `out` as it was."""
    a, b = pattern("noise", 5, 4), pattern("noise", 3, 3)
    out = np.full((2, 8, 10, 3), 77, np.uint8)
    bad = [
        (([a], [], 0, 8, 10, [(0, 0, 1, 0, 0, 5, 4)]), "output planes"),
        (([a], [], 2, 0, 10, [(0, 0, 1, 0, 0, 5, 4)]), "sides of 1.."),
        (([a], [(0, 4)], 2, 8, 10, [(0, 0, 2, 0, 0, 5, 4)]), "empty plane"),
        (([a], [], 2, 8, 10, [(0, 3, 1, 0, 0, 5, 4)]), "reads plane 3"),
        (([a], [], 2, 8, 10, [(0, -1, 1, 0, 0, 5, 4)]), "reads plane -1"),
        (([a], [], 2, 8, 10, [(0, 0, 0, 0, 0, 5, 4)]), "writes plane 0"),
        (([a], [], 2, 8, 10, [(0, 0, 3, 0, 0, 5, 4)]), "writes plane 3"),
        (([a], [], 2, 8, 10, [(0, 0, 1, 0, 0, 0, 4)]), "resizes to 0 x 4"),
        (([a], [], 2, 8, 10, [(0, 0, 1, 0, 0, 5, -2)]), "resizes to 5 x -2"),
        (([a], [], 2, 8, 10, [(0, 0, 1, 10, 0, 5, 4)]), "outside its destination"),
        (([a], [], 2, 8, 10, [(0, 0, 1, 0, -1, 5, 4)]), "outside its destination"),
        (([a], [(6, 6)], 2, 8, 10, [(0, 0, 1, 0, 0, 6, 6), (0, 1, 2, 0, 0, 5, 4)]), "of its own level"),
        (([a], [(6, 6)], 2, 8, 10, [(0, 1, 1, 0, 0, 6, 6)]), "of its own level"),
        (([a], [], 2, 8, 10, [(1, 0, 1, 0, 0, 5, 4), (0, 0, 2, 0, 0, 5, 4)]), "levels ascend"),
        (([a, b], [], 2, 8, 10, [(0, 0, 2, 0, 0, 5, 4), (0, 1, 2, 4, 3, 3, 3)]), "write the same pixels"),
        (([a], [(capi.RESAMPLE_MAX_SIDE, capi.RESAMPLE_MAX_SIDE)] * 2, 2, 8, 10, []), "bytes of scratch"),
    ]
    for args, word in bad:
        assert _call(lib, *args, out=out) == 1, word
        msg = lib.uda_last_error(None).decode()
        assert msg.startswith("uda_resample_np: ") and word in msg, (word, msg)
    assert _call(lib, [a], [], 2, 8, 10, [(0, 0, 1, 0, 0, 5, 4)], out=None) == 1 and "NULL" in lib.uda_last_error(None).decode()
    assert (out == 77).all()
    with pytest.raises(ValueError):
        collage.resample_np([a[:, :, :2]], [], 1, 8, 10, [])


def test_resample_fails_loudly_without_gpu(lib):
    """No CPU fallback: without a HIP device uda_resample_np returns 1, names itself and carries HIP's own words."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from uda_amd import capi, collage\n"
            "try:\n"
            "    collage.resample_np([np.ones((3, 4, 3), np.uint8)], [], 1, 6, 8, [(0, 0, 1, 0, 0, 8, 6)])\n"
            "    print('no error')\n"
            "except capi.UdaError as e:\n"
            "    print('UdaError|%%s' %% e)\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "UdaError|" in out.stdout and "uda_resample_np: " in out.stdout and "no ROCm-capable device is detected" in out.stdout, out.stdout


@pytest.mark.parametrize("key,dataset,scale", RUNS)
def test_planner_and_mirror_equal_the_golden(golden, key, dataset, scale):
    """plan_collage + the numpy mirror reproduce the real crop_collage: pixels, labels, file texts."""
    images, classes, boxes, target = golden_case(golden, key)
    got = collage.crop_collage(images, classes, boxes, target, dataset=dataset, scale=scale, resample=R.run_jobs)
    want = golden[key + ("scale_" if scale else "plain_") + "pixels"]
    assert got.images.shape == want.shape and got.images.dtype == np.uint8
    assert want.shape[1:3] == tuple(images[-1].shape[:2]) != tuple(images[0].shape[:2])      # the LAST image's size, and it has no crop
    golden_texts(got, golden, key, scale)
    assert np.array_equal(got.images, want)
    assert len(got) == len(want) > 1


@pytest.mark.parametrize("key,dataset,scale", RUNS)
def test_job_list_equals_the_reference_loop(golden, key, dataset, scale):
    """The planner's jobs against `collage_ref.pack`, the reference's packing loop on the crop sizes: the same resizes at the same
    places, in levels that respect what reads what."""
    images, classes, boxes, target = golden_case(golden, key)
    plan = collage.plan_collage(images, classes, boxes, target, dataset=dataset, scale=scale)
    sizes = [(x1 - x0, y1 - y0) for _, x0, y0, x1, y1 in plan.crops]
    S, T = len(plan.crops), len(plan.tmp_wh)
    assert 4 not in plan.images_used() and S == 7
    collages = R.pack(sizes, [[[0, 0, 1, 1]]] * S, [["c"]] * S, plan.width, plan.height, scale)
    assert len(collages) == plan.n
    assert any(len(sz) == 2 for placed, _ in collages for _, _, sz, _ in placed)             # a crop that overshoots: resized twice
    assert collages[-1][0][-1][1] + collages[-1][0][-1][2][-1][0] == plan.width              # the last crop takes the remaining width
    jobs = plan.jobs.tolist()
    assert [j[0] for j in jobs] == sorted(j[0] for j in jobs)
    by_src = {}
    for j in jobs:
        by_src.setdefault(j[1], []).append(j)
    written = {}
    for j in jobs:                                                                            # a plane is read only after the levels that write it
        assert j[1] < S or written[j[1]] < j[0]
        written[j[2]] = max(written.get(j[2], -1), j[0])
    for n, (placed, _) in enumerate(collages):
        for k, x_offset, sz, quads in placed:
            src = k
            for w, h in (sz if scale else sz[:-1]):                                           # the resizes that are read again: temporaries
                (j,) = by_src[src]
                assert j[3:7] == [0, 0, w, h] and S <= j[2] < S + T and plan.tmp_wh[j[2] - S] == (w, h)
                src = j[2]
            if scale:
                quad_jobs = by_src[src]
                part = quad_jobs[0][2]
                live = [q for q in quads if q[0] < sz[-1][0] and q[1] < sz[-1][1]]
                assert sorted(j[3:7] for j in quad_jobs) == sorted(list(q) for q in live)
                (j,) = by_src[part]
                assert j[2:7] == [S + T + n, x_offset, 0, sz[-1][0], sz[-1][1]]
            else:
                (j,) = [j for j in by_src[src] if j[2] >= S + T]
                assert j[2:7] == [S + T + n, x_offset, 0, sz[-1][0], sz[-1][1]]
    assert np.array_equal(R.render([images[i][y0:y1, x0:x1] for i, x0, y0, x1, y1 in plan.crops], collages, plan.width, plan.height),
                          golden[key + ("scale_" if scale else "plain_") + "pixels"])


def test_planner_quirks(golden):
    """The `> 2` filter drops a box but not its class (the lists differ, zip truncates), a box larger than its crop on both sides
    is not carried, a RandomState is drawn from as it is, and the reference's errors are raised."""
    images, classes, boxes, target = golden_case(golden, "kitti_")
    plan = collage.plan_collage(images, classes, boxes, target)
    labelled = [str(c) for labels in plan.labels for c, _ in labels]
    assert "Pedestrian" in labelled                                   # carried with the box of the entry after it
    kept = [b for labels in plan.labels for c, b in labels if str(c) == "Pedestrian"]
    assert all(b[3] - b[1] > 2 for b in kept)
    again = collage.plan_collage(images, classes, boxes, target, rng=np.random.RandomState(42))
    assert np.array_equal(again.jobs, plan.jobs) and again.crops == plan.crops
    other = collage.plan_collage(images, classes, boxes, target, rng=np.random.RandomState(43))
    assert other.crops != plan.crops
    sizes = [(im.shape[1], im.shape[0]) for im in images]
    assert np.array_equal(collage.plan_collage(sizes, classes, boxes, target).jobs, plan.jobs)      # sizes alone decide
    with pytest.raises(ZeroDivisionError):                            # a crop of zero height that is not the last one (of two, one is not)
        collage.plan_collage([(50, 40)], [["Tram"] * 3], [[[10.0, 5.0, 20.0, 5.0], [30.0, 20.0, 40.0, 30.0], [12.0, 9.0, 20.0, 9.0]]], ["Tram"],
                             rng=np.random.RandomState(3))
    with pytest.raises(ValueError):                                   # a target width of zero
        collage.plan_collage([(50, 40)], [["Tram"] * 3], [[[10.0, 5.0, 10.0, 9.0], [30.0, 20.0, 40.0, 30.0], [12.0, 5.0, 12.0, 9.0]]], ["Tram"],
                             rng=np.random.RandomState(3))


def test_box_cap_per_collage():
    """100 boxes a collage: the outer loop stops opening crops and the `break` cuts a crop's labels - with scale=True it leaves the
    inner loop only, so the other quadrants add one label each.  The labels equal the reference loop's (collage_ref.pack)."""
    n = 120
    boxes = [[float(3 * i), 10.0, float(3 * i + 3.5), 30.0] for i in range(n)]
    counts = {}
    for scale in (False, True):
        plan = collage.plan_collage([(800, 40)], [["Tram"] * n], [boxes], ["Tram"], scale=scale)
        assert len(plan.crops) == n
        sizes = [(x1 - x0, y1 - y0) for _, x0, y0, x1, y1 in plan.crops]
        want = R.pack(sizes, plan.crop_boxes, plan.crop_classes, 800, 40, scale)
        assert [labels for _, labels in want] == plan.labels
        counts[scale] = max(len(labels) for labels in plan.labels)
    assert counts[False] == collage.MAX_BOXES_PER_COLLAGE and counts[True] > collage.MAX_BOXES_PER_COLLAGE


def test_writers_write_the_reference_files(golden, tmp_path):
    from PIL import Image
    for key, dataset, scale in RUNS:
        images, classes, boxes, target = golden_case(golden, key)
        got = collage.crop_collage(images, classes, boxes, target, dataset=dataset, scale=scale, resample=R.run_jobs)
        tag = key + ("scale_" if scale else "plain_")
        d = str(tmp_path / tag)
        if dataset == "KITTI":
            assert collage.write_kitti_collage(d, got) == len(got)
            for i in range(len(got)):
                assert open(os.path.join(d, "%06d.txt" % (10000 + i))).read() == str(golden[tag + "texts"][i])
                assert np.array_equal(np.asarray(Image.open(os.path.join(d, "%06d.png" % (10000 + i)))), golden[tag + "pixels"][i])
            assert sorted(os.listdir(d)) == sorted("%06d.%s" % (10000 + i, e) for i in range(len(got)) for e in ("png", "txt"))
        else:
            assert collage.write_bdd_collage(d, got) == len(got)
            text = open(os.path.join(d, "bdd100k_labels_images_train.json")).read()
            assert text == str(golden[tag + "texts"][0])
            assert json.loads(text)[2] == ",\n"                      # the stray list item
            assert Image.open(os.path.join(d, "collage_%d.jpg" % (len(got) - 1))).size == (got.images.shape[2], got.images.shape[1])


def test_gt_inputs_read_the_label_files(golden, tmp_path):
    images, classes, boxes, _ = golden_case(golden, "kitti_")
    names = [str(s) + ".txt" for s in golden["kitti_stems"]]
    for name, text in zip(names, golden["kitti_label_files"]):
        (tmp_path / name).write_text(str(text))
    c, b = collage.gt_inputs(names, "KITTI", [str(k) for k in golden["kitti_classes"]], labels_folder=str(tmp_path))
    assert all(np.array_equal(x, y) for x, y in zip(c, classes)) and all(np.array_equal(x, y) for x, y in zip(b, boxes))


def test_paths_decode_only_the_images_that_give_a_crop(golden, tmp_path):
    from PIL import Image
    images, classes, boxes, target = golden_case(golden, "kitti_")
    paths = []
    for i, im in enumerate(images):
        paths.append(str(tmp_path / ("%d.png" % i)))
        if i != 4:                                                    # image 4 has no target box: with `sizes` its file is never opened
            Image.fromarray(im).save(paths[-1])
    sizes = [(im.shape[1], im.shape[0]) for im in images]
    got = collage.crop_collage(paths, classes, boxes, target, sizes=sizes, resample=R.run_jobs)
    assert np.array_equal(got.images, golden["kitti_plain_pixels"])
    Image.fromarray(images[4]).save(paths[4])
    got = collage.crop_collage(paths, classes, boxes, target, resample=R.run_jobs)       # sizes from the files' headers
    assert np.array_equal(got.images, golden["kitti_plain_pixels"])


def test_pseudo_inputs_name_the_classes_and_filter_the_names():
    selected = (np.asarray(["a.png", "b.png", "c.png"]), [np.asarray([7.0, 1.0]), np.asarray([5.0]), np.zeros(0)],
                [np.asarray([[1.0, 2.0, 30.0, 40.0], [5.0, 6.0, 70.0, 80.0]]), np.asarray([[0.0, 0.0, 9.0, 9.0]]), np.zeros((0, 4))])
    names, classes, boxes = collage.pseudo_inputs(selected, {1: "Car", 5: "Person_sitting", 7: "Tram"}, filter_ims=[True, False, True])
    assert names == ["a.png", "c.png"]                                # the names only, as in the reference (parent.py:377-378)
    assert [c.tolist() for c in classes] == [["Tram", "Car"], ["Person_sitting"], []]
    assert boxes[0].dtype == np.float64 and boxes[0].shape == (2, 4) and len(boxes) == 3


@pytest.mark.parametrize("option", collage.NOT_BUILT)
def test_unbuilt_options_raise_and_name_themselves(option):
    with pytest.raises(NotImplementedError, match=option):
        collage.crop_collage([np.zeros((8, 8, 3), np.uint8)], [[]], [[]], ["Tram"], **{option: True})
    with pytest.raises(NotImplementedError, match=option):
        collage.write_kitti_collage("unused", collage.Collage(np.zeros((0, 8, 8, 3), np.uint8), []), **{option: True})
