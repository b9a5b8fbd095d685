"""uda_collage_np on the device against the numpy mirror (tests/collage_aug_ref.py), and `crop_collage(manual_augmentations=True)`
against the golden of the real `Parent_SSL.crop_collage`.  Every run goes through the C ABI (`collage.collage_np`).  EVERY PIXEL IS
EQUAL: the augmentations are integer and float32 arithmetic, the blend is built without FMA contraction.  No tolerance.

Sizes: a pointwise tile is capi.AUGMENT_TILE pixels x capi.AUGMENT_ROWS rows, a blur tile capi.AUGMENT_TILE positions x
capi.AUGMENT_TILE lines with a halo of 3 (r + 1) positions a side: planes one below, at and one above 8 and 32, and 1 and 2."""
import numpy as np
import pytest

import collage_aug_ref as A
import collage_ref as R
import test_collage_aug_host as HA
import test_collage_host as H
from uda_amd import capi, collage

pytestmark = pytest.mark.gpu
TILE, ROWS = capi.AUGMENT_TILE, capi.AUGMENT_ROWS
SIDES = sorted({1, 2, ROWS - 1, ROWS, ROWS + 1, TILE - 1, TILE, TILE + 1})
OPS = (A.FLIP, A.BRIGHTNESS, A.CONTRAST, A.BLUR, A.NOISE)


def both(src, tmp_wh, n, height, width, jobs, params=(), noise=None):
    """The device's output planes, after they were found equal to the mirror's."""
    got = collage.collage_np(src, tmp_wh, n, height, width, jobs, params, noise)
    want = A.run_jobs(src, tmp_wh, n, height, width, jobs, params, noise)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def one(img, op, value=None, noise=None, x=0, y=0, width=None, height=None):
    h, w = img.shape[:2]
    width, height = width or x + w, height or y + h
    return both([img], [], 1, height, width, [(0, 0, 1, x, y, w, h, op, 0)], [] if value is None else [value],
                noise if op == A.NOISE else None)


def noise_for(img, seed=0):
    return np.random.default_rng(seed).integers(0, 256, img.shape, dtype=np.uint8)


@pytest.mark.parametrize("w", SIDES)
def test_every_op_on_widths_around_the_tiles(w):
    for h in (1, 2, ROWS + 1):
        img = H.pattern("noise", w, h, w)
        for op, value in ((A.FLIP, None), (A.BRIGHTNESS, 1.21), (A.CONTRAST, 0.77), (A.BLUR, 2.0), (A.NOISE, None)):
            one(img, op, value, noise_for(img), x=1, y=2)


@pytest.mark.parametrize("h", SIDES)
def test_every_op_on_heights_around_the_tiles(h):
    for w in (1, 2, TILE + 1):
        img = H.pattern("binary", w, h, h)
        for op, value in ((A.FLIP, None), (A.BRIGHTNESS, 0.83), (A.CONTRAST, 1.29), (A.BLUR, 1.1), (A.NOISE, None)):
            one(img, op, value, noise_for(img), x=2, y=1)


@pytest.mark.parametrize("radius", [0.0, 0.3, 1.0, 1.5, 2.999, 3.0, 8.0])
def test_blur_line_lengths_around_the_box(radius):
    """r = 0 (radius 0.3), the copy (radius 0), and for every r lines of r, r + 1 and r + 2 positions on each axis: r + 1 greater
    than, equal to and less than the line length."""
    r = int(A.gauss_box(radius)[0])
    assert radius != 0.3 or r == 0
    for n in sorted({max(1, r), r + 1, r + 2}):
        one(H.pattern("noise", n, 37, 1), A.BLUR, radius)
        one(H.pattern("noise", 37, n, 2), A.BLUR, radius)
        one(H.pattern("checker", n, n, 3), A.BLUR, radius)


def test_blur_largest_radius_and_tiles_at_the_line_ends():
    """The largest accepted radius (box 15, halo 48) on planes narrower than the halo, on one whose single tile touches both ends
    of its lines (TILE positions), and on one with tiles at the start, in the middle (a full halo on both sides) and at the end."""
    radius = capi.BLUR_MAX_RADIUS
    r = int(A.gauss_box(radius)[0])
    assert r == capi.BLUR_MAX_BOX and 3 * (r + 1) > TILE
    one(H.pattern("noise", 20, 9, 1), A.BLUR, radius)
    one(H.pattern("noise", 9, 20, 2), A.BLUR, radius)
    one(H.pattern("binary", TILE, TILE, 3), A.BLUR, radius)
    one(H.pattern("noise", 5 * TILE + 3, 5, 4), A.BLUR, radius)
    one(H.pattern("noise", 5, 5 * TILE + 3, 5), A.BLUR, radius)
    one(H.pattern("dots", 3 * TILE + 1, 2 * TILE + 5, 6), A.BLUR, 3.0)
    with pytest.raises(capi.UdaError, match="uda_collage_np: .*radius"):
        collage.augment_np(H.pattern("noise", 4, 4), "blur", radius + 0.01)


def test_contrast_mean_over_several_blocks_and_the_half():
    """300 x 200 pixels are 15 blocks of the sum; the k + 0.5 plane's mean rounds up."""
    img = H.pattern("noise", 300, 200, 9)
    for factor in (0.7, 1.3, 0.0):
        one(img, A.CONTRAST, factor)
    out = one(HA.half_plane(), A.CONTRAST, 0.0)
    assert (out == 101).all()
    one(HA.half_plane(37), A.CONTRAST, 1.3)
    flat = np.full((200, 300, 3), 255, np.uint8)                     # the largest sum a plane of this size has
    assert (one(flat, A.CONTRAST, 0.0) == 255).all()


@pytest.mark.parametrize("factor", [0.0, 0.3, 0.7, 1.0, 1.0000001, 1.3, 1.9, 7.5])
def test_blend_on_all_256_values(factor):
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    ramp[..., 1] = ramp[::-1, ::-1, 1]
    ramp[..., 2] = ramp[:, ::-1, 2]
    one(ramp, A.BRIGHTNESS, factor)
    one(ramp, A.CONTRAST, factor)


@pytest.mark.parametrize("x", [0, 1, 2, 3, "clipped"])
def test_destination_offsets_and_clipped_paste(x):
    """3-byte pixels at any x; a paste that reaches past the right and the bottom edge is cut as Image.paste cuts it."""
    w, h, width, height = 21, 17, 50, 24
    clipped = x == "clipped"
    x, y = (width - w + 5, height - h + 4) if clipped else (x, 3)
    img = H.pattern("noise", w, h, 7)
    for op, value in ((A.FLIP, None), (A.BRIGHTNESS, 1.1), (A.CONTRAST, 0.9), (A.BLUR, 2.5), (A.NOISE, None)):
        out = one(img, op, value, noise_for(img, 3), x=x, y=y, width=width, height=height)
        assert not out[0, :y].any() and not out[0, :, :x].any()
        if not clipped:
            assert not out[0, y + h:].any() and not out[0, :, x + w:].any()


def test_chain_resize_augment_quadrants_paste():
    """One call, four levels: a crop resized into a temporary, augmented into a second, its four quadrant resizes into a part (the
    right ones clipped by the part's edge), the part pasted - for every kind, beside a plain resize of another crop."""
    a, b = H.pattern("noise", 10, 14, 1), H.pattern("dots", 17, 6, 2)
    w, h = 15, 30                                           # ceil(.75 * 15) + ceil(.25 * 15) = 16: the right quadrants are clipped
    nz = noise_for(np.zeros((h, w, 3)), 5)
    for op, value in ((A.FLIP, None), (A.BRIGHTNESS, 1.27), (A.CONTRAST, 0.71), (A.BLUR, 1.7), (A.NOISE, None)):
        jobs = [(0, 0, 2, 0, 0, w, h, 0, 0), (1, 2, 3, 0, 0, w, h, op, 0), (2, 3, 4, 0, 0, 12, 23, 0, 0), (2, 3, 4, 12, 0, 4, 23, 0, 0),
                (2, 3, 4, 0, 23, 12, 8, 0, 0), (2, 3, 4, 12, 23, 4, 8, 0, 0), (3, 4, 5, 25, 0, w, h, 0, 0), (3, 1, 6, 3, 2, 17, 6, 0, 0)]
        both([a, b], [(w, h)] * 3, 2, 30, 40, jobs, [] if value is None else [value], nz if op == A.NOISE else None)


def test_forty_mixed_jobs_in_one_call_and_one_by_one():
    rng = np.random.default_rng(11)
    src = [H.pattern(H.KINDS[i % 4], int(rng.integers(1, 60)), int(rng.integers(1, 40)), i) for i in range(40)]
    jobs, params, noise, x = [], [], [], [0, 0, 0]
    for i in range(40):                                     # side by side, plane after plane; the last of a plane may be clipped
        p, op = i % 3, i % 6
        h0, w0 = src[i].shape[:2]
        w, h = (int(v) for v in rng.integers(1, 40, 2)) if op == 0 else (w0, h0)
        arg = 0
        if op in (A.BRIGHTNESS, A.CONTRAST, A.BLUR):
            params.append(float(rng.uniform(0.7, 1.3)) if op != A.BLUR else float(rng.uniform(0.2, 4)))
            arg = len(params) - 1
        jobs.append((0, i, 40 + p, x[p], int(rng.integers(0, 4)), w, h, op, arg))
        x[p] += w
    width = max(x) - 3
    jobs = [j for j in jobs if j[3] < width]
    for j in jobs:
        if j[7] == A.NOISE:
            noise.append(rng.integers(0, 256, 3 * j[5] * j[6], dtype=np.uint8))
    assert {j[7] for j in jobs} == set(range(6)) and len(noise) > 1
    together = both(src, [], 3, 44, width, jobs, params, np.concatenate(noise))
    alone, at = np.zeros_like(together), 0
    for j in jobs:
        nz = None
        if j[7] == A.NOISE:
            nz, at = noise[at], at + 1
        got = collage.collage_np([src[j[1]]], [], 1, 44, width, [(0, 0, 1) + tuple(j[3:8]) + (0,)],
                                 [params[j[8]]] if j[7] in (A.BRIGHTNESS, A.CONTRAST, A.BLUR) else [], nz)
        alone[j[2] - 40] |= got[0]
    assert np.array_equal(together, alone)


def test_resize_only_jobs_equal_uda_resample_np():
    """op 0 only: uda_collage_np and uda_resample_np give the same bytes (and Pillow's, through the mirror)."""
    a, b = H.pattern("noise", 10, 14, 1), H.pattern("dots", 17, 6, 2)
    three = [(0, 0, 2, 0, 0, 41, 30), (1, 2, 3, 0, 0, 15, 30), (2, 3, 4, 0, 0, 12, 23), (2, 3, 4, 12, 0, 4, 23), (2, 3, 4, 0, 23, 12, 8),
             (2, 3, 4, 12, 23, 4, 8), (3, 4, 5, 25, 0, 15, 30), (3, 1, 6, 3, 2, 17, 6), (3, 0, 6, 20, 9, 10, 14), (3, 0, 6, 0, 9, 4, 300)]
    tmp = [(41, 30), (15, 30), (15, 30)]
    old = collage.resample_np([a, b], tmp, 2, 30, 40, three)
    new = collage.collage_np([a, b], tmp, 2, 30, 40, [j + (0, 0) for j in three])
    assert np.array_equal(old, new) and np.array_equal(old, R.run_jobs([a, b], tmp, 2, 30, 40, three))


def test_augment_np_and_apply_manual_augmentation():
    img = H.pattern("noise", 45, 20, 4)
    nz = noise_for(img, 8)
    for kind, value in (("flip", None), ("brightness", 1.3), ("contrast", 0.7), ("blur", 2.2), ("noise", None)):
        got = collage.augment_np(img, kind, value, nz if kind == "noise" else None)
        assert np.array_equal(got, A.augment(img, A.KINDS[kind], value, nz))
    seen = set()
    for seed in range(12):                                            # the reference's call shape: the same draws, the same pixels
        boxes = [[3.0, 2.0, 10.0, 9.0]]
        got, got_boxes = collage.apply_manual_augmentation(img, boxes, rng=np.random.RandomState(seed))
        rs = np.random.RandomState(seed)
        k = int(rs.choice(5))
        value = rs.uniform(0.7, 1.3) if k in (1, 2) else rs.uniform(1, 3) if k == 3 else None
        noise = rs.randint(5, 20, img.shape, dtype="uint8") if k == 4 else None
        assert np.array_equal(got, A.augment(img, k + 1, value, noise))
        assert got_boxes is boxes and boxes == ([[35.0, 2.0, 42.0, 9.0]] if k == 0 else [[3.0, 2.0, 10.0, 9.0]])
        seen.add(k)
    assert seen == set(range(5))


@pytest.fixture(scope="module")
def golden():
    return np.load(HA.GOLDEN)


@pytest.mark.parametrize("key,dataset,scale", H.RUNS)
def test_crop_collage_equals_the_golden(golden, key, dataset, scale):
    images, classes, boxes, target = H.golden_case(golden, key)
    want = golden[key + ("scale_" if scale else "plain_") + "pixels"]
    got = collage.crop_collage(images, classes, boxes, target, dataset=dataset, scale=scale, manual_augmentations=True)
    H.golden_texts(got, golden, key, scale)
    assert got.images.shape == want.shape and np.array_equal(got.images, want)
