"""RCC's manual augmentations without a GPU: the numpy mirror (tests/collage_aug_ref.py) against live Pillow, the library's
host-only box-blur weights against the mirror's, the planner with manual_augmentations against the golden of the REAL
`Parent_SSL.crop_collage(manual_augmentations=True)` (tests/golden/make_collage_aug_golden.py), the draw sequence, the argument
errors of uda_collage_np, the no-device message and the symbols.  Pixels are compared for equality: Pillow's augmentations are
integer and float32 arithmetic."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import collage_aug_ref as A
import collage_ref as R
import test_collage_host as H
from common import ROOT
from uda_amd import capi, collage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collage_aug_golden.npz")
RUNS = H.RUNS
RADII = (0.05, 0.3, 0.58, 1, 1.5, 2.999, 3, 8)
BLUR_PLANES = ((1, 1), (7, 1), (1, 7), (2, 2), (40, 5), (5, 40), (31, 33))       # (w, h)
FACTORS = (0, 0.7, 1, 1.3)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def pillow(golden):
    """Live Pillow, when it is the version that made the golden (whose arithmetic the mirror restates)."""
    import PIL
    if PIL.__version__ != str(golden["pillow_version"][0]):
        pytest.skip("Pillow %s is installed, the mirror was pinned to Pillow %s" % (PIL.__version__, golden["pillow_version"][0]))
    return PIL


def half_plane(k=100):
    """Two grey pixels k and k + 1: the mean luma is exactly k + 0.5, which int(mean + 0.5) rounds up."""
    return np.asarray([[[k, k, k], [k + 1, k + 1, k + 1]]], np.uint8)


def same(img, op, value=None, noise=None):
    got, want = A.augment(img, op, value, noise), A.pillow_augment(img, op, value, noise)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (op, value, img.shape, np.argwhere(got != want)[:3].tolist())
    return got


@pytest.mark.parametrize("radius", RADII)
def test_mirror_blur_equals_live_pillow(pillow, radius):
    r = int(A.gauss_box(radius)[0])
    for w, h in BLUR_PLANES:
        for kind in H.KINDS:
            same(H.pattern(kind, w, h, seed=3), A.BLUR, radius)
    assert r == 0 or any(min(w, h) < r + 1 for w, h in BLUR_PLANES)  # lines shorter than r + 1


def test_mirror_blend_equals_live_pillow(pillow):
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    ramp[..., 1] = ramp[::-1, ::-1, 1]
    for factor in FACTORS:
        for img in (ramp, H.pattern("noise", 33, 31, 1), H.pattern("binary", 7, 5, 2), H.pattern("noise", 1, 1, 3)):
            same(img, A.BRIGHTNESS, factor)
            same(img, A.CONTRAST, factor)
        got = same(half_plane(), A.CONTRAST, factor)
        assert A.contrast_mean(half_plane()) == 101
        if factor == 0:
            assert (got == 101).all()                                 # the degenerate image itself: the mean, rounded half up


def test_mirror_flip_and_noise_equal_live_pillow(pillow):
    for w in (1, 2, 7, 8):
        img = H.pattern("noise", w, 5, w)
        got = same(img, A.FLIP)
        assert np.array_equal(got[:, 0], img[:, w - 1])
    img = np.full((3, 4, 3), 250, np.uint8)
    noise = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)
    got = same(img, A.NOISE, noise=noise)
    assert got[0, 0, 0] == 250 and got[0, 2, 0] == 0 and got[2, 3, 2] == (250 + 35) % 256      # wraps modulo 256; np.clip after it changes nothing


def test_library_gauss_box_equals_the_mirror(lib):
    rng = np.random.default_rng(5)
    radii = np.concatenate([32 * (1 - rng.random(992)), RADII])      # (0, 32]
    assert len(radii) == 1000 and radii.min() > 0 and radii.max() <= 32
    for radius in radii:
        fr, ww, fw = collage.gauss_box(radius)
        m_fr, m_ww, m_fw = A.gauss_box(radius)
        assert fr.tobytes() == m_fr.tobytes() and (ww, fw) == (m_ww, m_fw), radius
    assert collage.gauss_box(0) == (0, 1 << 24, 0)
    assert int(collage.gauss_box(capi.BLUR_MAX_RADIUS)[0]) <= capi.BLUR_MAX_BOX
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(capi.UdaError, match="uda_gauss_box_np: "):
            collage.gauss_box(bad)


@pytest.mark.parametrize("key,dataset,scale", RUNS)
def test_planner_and_mirror_equal_the_golden(golden, key, dataset, scale):
    """plan_collage(manual_augmentations=True) + the numpy mirror reproduce the real crop_collage: kinds, pixels, labels."""
    images, classes, boxes, target = H.golden_case(golden, key)
    got = collage.crop_collage(images, classes, boxes, target, dataset=dataset, scale=scale, manual_augmentations=True, resample=A.run_jobs)
    tag = key + ("scale_" if scale else "plain_")
    want = golden[tag + "pixels"]
    kinds = [k for k, _ in got.plan.augment]
    assert kinds == [str(k) for k in golden[tag + "kinds"]] and set(kinds) == set(collage.AUGMENT_KINDS)
    assert got.plan.jobs.shape[1] == 9 and got.plan.jobs.dtype == np.int32
    H.golden_texts(got, golden, key, scale)
    assert got.images.shape == want.shape and np.array_equal(got.images, want)
    # the flipped crop carries a box, rewritten with the resized width
    flipped = [i for i, k in enumerate(kinds) if k == "flip" and len(got.plan.crop_boxes[i])]
    assert flipped


@pytest.mark.parametrize("key,dataset,scale", RUNS)
def test_planner_with_the_option_off_is_unchanged(golden, key, dataset, scale):
    """Off: the [K, 7] plan the resize-only planner made - checked against the reference's packing loop (collage_ref.pack /
    render) and, on the first golden's inputs, against that golden's pixels - and no draw more on the stream."""
    images, classes, boxes, target = H.golden_case(golden, key)
    rng = np.random.RandomState(42)
    plan = collage.plan_collage(images, classes, boxes, target, dataset=dataset, scale=scale, rng=rng, manual_augmentations=False)
    after = rng.uniform()
    default = collage.plan_collage(images, classes, boxes, target, dataset=dataset, scale=scale)
    assert plan.jobs.shape[1] == 7 and np.array_equal(plan.jobs, default.jobs) and plan.labels == default.labels
    assert len(plan.params) == 0 and len(plan.noise) == 0 and plan.augment == []
    replay = np.random.RandomState(42)
    replay.uniform(0.5, 1.0, len(plan.crops))
    replay.shuffle(np.arange(len(plan.crops)))
    assert replay.uniform() == after
    sizes = [(x1 - x0, y1 - y0) for _, x0, y0, x1, y1 in plan.crops]
    crops = [images[i][y0:y1, x0:x1] for i, x0, y0, x1, y1 in plan.crops]
    packed = R.pack(sizes, plan.crop_boxes, plan.crop_classes, plan.width, plan.height, scale)
    assert [labels for _, labels in packed] == plan.labels
    assert np.array_equal(R.run_jobs(crops, plan.tmp_wh, plan.n, plan.height, plan.width, plan.jobs), R.render(crops, packed, plan.width, plan.height))
    first = np.load(H.GOLDEN)
    images, classes, boxes, target = H.golden_case(first, key)
    got = collage.crop_collage(images, classes, boxes, target, dataset=dataset, scale=scale, manual_augmentations=False, resample=R.run_jobs)
    assert np.array_equal(got.images, first[key + ("scale_" if scale else "plain_") + "pixels"])


@pytest.mark.parametrize("scale", [False, True])
def test_draw_sequence_equals_a_hand_written_replay(golden, scale):
    images, classes, boxes, target = H.golden_case(golden, "kitti_")
    plan = collage.plan_collage(images, classes, boxes, target, scale=scale, rng=np.random.RandomState(42), manual_augmentations=True)
    rs = np.random.RandomState(42)
    S = len(plan.crops)
    for _ in range(S):
        rs.uniform(0.5, 1.0)                                          # a margin a crop
    rs.shuffle(np.arange(S))
    S0, T = S, len(plan.tmp_wh)
    augment, noise = [], []
    jobs = plan.jobs.tolist()
    aug_jobs = [j for j in jobs if j[7] != 0]
    by_crop = {}
    for k in range(S):                                                # crop k -> its resizes into temporaries -> its augment job
        cur = k
        while k not in by_crop:
            readers = [j for j in jobs if j[1] == cur]
            if readers[0][7] != 0:
                (by_crop[k],) = readers
            else:
                ((_, _, cur, *_),) = readers
    assert len(aug_jobs) == S and S0 + T > S
    for k in range(S):                                                # packing order is crop order
        w, h = by_crop[k][5], by_crop[k][6]
        kind = rs.choice(5)
        if kind == 0:
            augment.append(("flip", None))
        elif kind == 1:
            augment.append(("brightness", rs.uniform(0.7, 1.3)))
        elif kind == 2:
            augment.append(("contrast", rs.uniform(0.7, 1.3)))
        elif kind == 3:
            augment.append(("blur", rs.uniform(1, 3)))
        else:
            augment.append(("noise", None))
            noise.append((by_crop[k], rs.randint(5, 20, (h, w, 3), dtype="uint8")))
    assert plan.augment == augment
    assert plan.params.tolist() == [v for _, v in augment if v is not None]
    noise.sort(key=lambda jn: jobs.index(jn[0]))                     # job-list order
    assert np.array_equal(plan.noise, np.concatenate([z.reshape(-1) for _, z in noise]))
    for j in aug_jobs:                                                # one level after the resize that made its source
        made = [i for i in jobs if i[2] == j[1]]
        assert len(made) == 1 and made[0][0] == j[0] - 1 and made[0][7] == 0 and (made[0][5], made[0][6]) == (j[5], j[6])
        assert (j[2] >= S0 + T) != scale                              # straight into the collage, or into the quadrants' temporary


def test_flip_rewrites_the_boxes_with_the_resized_width():
    """box[0], box[2] = width - box[2], width - box[0] with the RESIZED width on boxes in crop coordinates: the reference's own."""
    for seed in range(200):
        rng = np.random.RandomState(seed)
        args = ([(100, 60)], [["Tram", "Car"]], [[[30.0, 10.0, 50.0, 30.0], [34.0, 14.0, 44.0, 26.0]]], ["Tram"])
        plan = collage.plan_collage(*args, rng=rng, manual_augmentations=True)
        if plan.augment[0][0] != "flip":
            continue
        plain = collage.plan_collage(*args, rng=np.random.RandomState(seed))
        width = plan.jobs[-1, 5]
        assert width == 100 and len(plain.crop_boxes[0]) == 2
        for a, b in zip(plan.crop_boxes[0], plain.crop_boxes[0]):
            assert a == [width - b[2], b[1], width - b[0], b[3]]
        return
    raise AssertionError("no seed below 200 draws a flip")


def _call(lib, src, tmp_wh, n, h, w, jobs, params=(), noise=None, noise_bytes=None, out=None):
    src_wh = np.asarray([(s.shape[1], s.shape[0]) for s in src], np.int32).reshape(-1, 2)
    pix = np.concatenate([s.reshape(-1) for s in src]) if src else np.zeros(1, np.uint8)
    tmp = np.asarray(tmp_wh, np.int32).reshape(-1, 2)
    jobs = np.asarray(jobs, np.int32).reshape(-1, 9)
    params = np.asarray(params, np.float64).reshape(-1)
    noise = np.zeros(0, np.uint8) if noise is None else np.asarray(noise, np.uint8).reshape(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None      # noqa: E731
    return lib.uda_collage_np(0, len(src), p(src_wh), p(pix), len(tmp), p(tmp), n, h, w, len(jobs), p(jobs), len(params), p(params),
                              noise.size if noise_bytes is None else noise_bytes, p(noise), None if out is None else p(out))


def test_collage_argument_errors(lib):
    """Every refusal comes before the device is touched, names the entry point, and leaves `out` as it was."""
    a = H.pattern("noise", 5, 4)
    out = np.full((2, 8, 10, 3), 77, np.uint8)
    nz = np.zeros(60, np.uint8)
    bad = [
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 6, 0)]), "op 6"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, -1, 0)]), "op -1"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 2, 1)], params=[1.0]), "arg 1"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 3, -1)], params=[1.0]), "arg -1"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 4, 0)]), "arg 0"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 2, 0)], params=[float("nan")]), "finite"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 3, 0)], params=[float("inf")]), "finite"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 4, 0)], params=[-0.5]), "finite and >= 0"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 4, 0)], params=[capi.BLUR_MAX_RADIUS + 0.001]), "radius"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 5, 0)], noise=nz[:59]), "noise bytes"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 5, 0)]), "noise bytes"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 4, 1, 0)], noise=nz), "noise bytes"),
        (dict(jobs=[(0, 0, 1, 0, 0, 6, 4, 1, 0)]), "keeps the size"),
        (dict(jobs=[(0, 0, 1, 0, 0, 5, 3, 5, 0)], noise=nz[:45]), "keeps the size"),
        # the refusals of uda_resample_np, under this entry point's name
        (dict(jobs=[(0, 3, 1, 0, 0, 5, 4, 1, 0)]), "reads plane 3"),
        (dict(jobs=[(0, 0, 0, 0, 0, 5, 4, 1, 0)]), "writes plane 0"),
        (dict(jobs=[(0, 0, 1, 10, 0, 5, 4, 1, 0)]), "outside its destination"),
        (dict(jobs=[(1, 0, 1, 0, 0, 5, 4, 1, 0), (0, 0, 2, 0, 0, 5, 4, 0, 0)]), "levels ascend"),
        (dict(jobs=[(0, 0, 2, 0, 0, 5, 4, 1, 0), (0, 0, 2, 4, 3, 5, 4, 0, 0)]), "write the same pixels"),
    ]
    for kw, word in bad:
        assert _call(lib, [a], [], 2, 8, 10, out=out, **kw) == 1, word
        msg = lib.uda_last_error(None).decode()
        assert msg.startswith("uda_collage_np: ") and word in msg, (word, msg)
    assert _call(lib, [a], [], 2, 8, 10, [(0, 0, 1, 0, 0, 5, 4, 1, 0)], out=None) == 1 and "NULL" in lib.uda_last_error(None).decode()
    assert (out == 77).all()
    with pytest.raises(ValueError):
        collage.collage_np([a[:, :, :2]], [], 1, 8, 10, [])
    with pytest.raises(ValueError):
        collage.augment_np(a, "sharpen")
    with pytest.raises(ValueError):
        collage.augment_np(a, "blur")
    with pytest.raises(ValueError):
        collage.augment_np(a, "noise", noise=np.zeros((4, 4, 3), np.uint8))


def test_collage_fails_loudly_without_gpu(lib):
    """No CPU fallback: without a HIP device uda_collage_np returns 1, names itself and carries HIP's own words."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from uda_amd import capi, collage\n"
            "try:\n"
            "    collage.augment_np(np.ones((3, 4, 3), np.uint8), 'flip')\n"
            "    print('no error')\n"
            "except capi.UdaError as e:\n"
            "    print('UdaError|%%s' %% e)\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "UdaError|" in out.stdout and "uda_collage_np: " in out.stdout and "no ROCm-capable device is detected" in out.stdout, out.stdout


def test_symbols_in_header_binding_and_library(lib):
    header = open(os.path.join(ROOT, "include", "uda_hip.h")).read()
    for name in ("uda_collage_np", "uda_gauss_box_np"):
        assert "int %s(" % name in header and name in capi._SIGNATURES and hasattr(lib, name)
    assert "#define UDA_AUGMENT_TILE %d\n" % capi.AUGMENT_TILE in header
    assert "#define UDA_BLUR_MAX_BOX %d\n" % capi.BLUR_MAX_BOX in header and "#define UDA_BLUR_MAX_RADIUS %.1f " % capi.BLUR_MAX_RADIUS in header
    assert "manual_augmentations" not in collage.NOT_BUILT


def test_manual_augmentations_is_built_and_the_writers_take_no_such_option():
    """The calls with which test_collage_host.py's parametrised test found the option refused while it was in NOT_BUILT: crop_collage
    now takes it (no target box: no crop, no collage, no device call), and the writers, which never had such an option, call
    it unknown."""
    assert "manual_augmentations" not in collage.NOT_BUILT
    got = collage.crop_collage([np.zeros((8, 8, 3), np.uint8)], [[]], [[]], ["Tram"], manual_augmentations=True)
    assert len(got) == 0 and got.images.shape == (0, 8, 8, 3) and got.plan.augment == [] and got.plan.jobs.shape == (0, 9)
    for write in (collage.write_kitti_collage, collage.write_bdd_collage):
        with pytest.raises(TypeError, match="manual_augmentations"):
            write("unused", collage.Collage(np.zeros((0, 8, 8, 3), np.uint8), []), manual_augmentations=True)
