"""uda_resample_np on the device against the numpy mirror (tests/collage_ref.py) and live Pillow, and `crop_collage` against the golden
of the real `Parent_SSL.crop_collage`.  Every run goes through the C ABI (`collage.resample_np`).  EVERY PIXEL IS EQUAL: Pillow's
8-bit resize is integer arithmetic on coefficient tables, the tables are built on the host in double with the C library's sin,
and the device adds the same int32 products.  No tolerance, no case left out.

Sizes: a horizontal tile holds capi.RESAMPLE_TILE output columns x 8 rows, a vertical one 8 output rows x 32 columns (fewer
positions and more lines when the output is narrow or the source span of a tile would not fit the LDS buffer): outputs one
below, at and one above 8 and 32; shrinking by 20, 60 and 100 so that the tile narrows down to one position; ksize up to 421,
far above the 16 coefficients a chunk holds."""
import numpy as np
import pytest

import collage_ref as R
import test_collage_host as H
from uda_amd import capi, collage

pytestmark = pytest.mark.gpu
TILE = capi.RESAMPLE_TILE


def both(src, tmp_wh, n, height, width, jobs):
    """The device's output planes, after they were found equal to the mirror's and to live Pillow's."""
    got = collage.resample_np(src, tmp_wh, n, height, width, jobs)
    want = R.run_jobs(src, tmp_wh, n, height, width, jobs)
    assert np.array_equal(want, R.run_jobs_pillow(src, tmp_wh, n, height, width, jobs)), "the mirror differs from live Pillow"
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def one(img, w, h, x=0, y=0, width=None, height=None):
    width, height = width or x + w, height or y + h
    return both([img], [], 1, height, width, [(0, 0, 1, x, y, w, h)])


@pytest.mark.parametrize("src,dst", H.EDGES)
@pytest.mark.parametrize("kind", H.KINDS)
def test_edges(kind, src, dst):
    """3 x 3 -> 7 x 5, each pass skipped in turn, the copy, 70 -> 1 (ksize 421), 1 x N sources, on noise, 0 / 255 checkerboards,
    0 / 255 noise and single bright pixels (negative accumulators, overshoot above 255)."""
    one(H.pattern(kind, *src), *dst, x=1, y=2)


@pytest.mark.parametrize("w", [7, 8, 9, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_output_widths_around_the_tile(w):
    one(H.pattern("noise", 23, 11, w), w, 11)               # along x only
    one(H.pattern("binary", 23, 11, w), w, 19)              # both passes: the columns are the vertical pass's lines
    one(H.pattern("noise", 90, 11, w), w, 7, x=2)           # shrinking both


@pytest.mark.parametrize("h", [7, 8, 9, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_output_heights_around_the_tile(h):
    one(H.pattern("noise", 11, 23, h), 11, h)               # along y only
    one(H.pattern("binary", 11, 23, h), 35, h)              # both passes: the source rows are the horizontal pass's lines
    one(H.pattern("noise", 11, 90, h), 7, h, y=1)


@pytest.mark.parametrize("n_in,n_out", [(600, 30), (1500, 25), (2000, 20), (4000, 3), (333, 32)])
def test_shrinking_narrows_the_tile(n_in, n_out):
    one(H.pattern("noise", n_in, 5, 1), n_out, 5)
    one(H.pattern("binary", 5, n_in, 2), 5, n_out)
    one(H.pattern("noise", n_in, 9, 3), n_out, 4)


def test_enlarging_to_collage_height():
    """The service's own shapes: a small crop to 375 rows, a larger one to 720, and the second resize of an overshoot (x only)."""
    one(H.pattern("noise", 25, 31, 4), 302, 375)
    one(H.pattern("dots", 140, 100, 5), 1008, 720)
    one(H.pattern("noise", 300, 720, 6)[:, :, :], 173, 720)


@pytest.mark.parametrize("x", [0, 1, 2, 3, "right"])
def test_destination_offsets(x):
    """3-byte pixels at any x: the stores are not dword aligned and touch nobody else's bytes."""
    w, width = 21, 50
    x = width - w if x == "right" else x
    out = one(H.pattern("noise", 13, 9, 7), w, 17, x=x, y=3, width=width, height=24)
    assert not out[0, :3].any() and not out[0, 20:].any() and not out[0, :, :x].any() and not out[0, :, x + w:].any()


def test_abutting_jobs_and_guard_columns():
    """Two jobs side by side in plane 0 and two with a gap of guard columns in plane 2; plane 1 in between gets nothing: all the
    guards stay zero."""
    a, b, c = H.pattern("noise", 9, 12, 1), H.pattern("checker", 14, 5, 2), H.pattern("binary", 6, 6, 3)
    jobs = [(0, 0, 3, 3, 0, 10, 20), (0, 1, 3, 13, 0, 9, 20), (0, 2, 5, 0, 1, 7, 18), (0, 0, 5, 10, 0, 30, 20)]
    out = both([a, b, c], [], 3, 20, 40, jobs)
    assert not out[1].any() and not out[0, :, :3].any() and not out[0, :, 22:].any() and not out[2, :, 7:10].any() and not out[2, 0, :7].any()


def test_clipped_paste():
    """x + w = W + 1 and y + h = H + 2: what reaches past the edge is dropped, as Image.paste drops it - with both passes, with
    each alone, for the copy, and for a source that Pillow resizes along y first."""
    for src, (w, h) in (((9, 7), (20, 15)), ((9, 15), (20, 15)), ((20, 7), (20, 15)), ((20, 15), (20, 15)), ((3, 400), (20, 15))):
        one(H.pattern("noise", *src, seed=w + h), w, h, x=11, y=0, width=30, height=15)
        one(H.pattern("noise", *src, seed=w * h), w, h, x=0, y=6, width=20, height=19)
        one(H.pattern("binary", *src, seed=1), w, h, x=11, y=6, width=30, height=19)


def test_job_chains():
    """Two levels (a crop resized, then resized again from its resized pixels) and three (then the four quadrants into a part, a
    quadrant clipped by the part's edge, and the part pasted)."""
    a, b = H.pattern("noise", 10, 14, 1), H.pattern("dots", 17, 6, 2)
    two = [(0, 0, 2, 0, 0, 41, 30), (0, 1, 4, 0, 0, 25, 30), (1, 2, 4, 25, 0, 15, 30)]
    both([a, b], [(41, 30)], 2, 30, 40, two)
    w, h = 15, 30                                           # ceil(.75 * 15) + ceil(.25 * 15) = 16: the right quadrants are clipped
    three = [(0, 0, 2, 0, 0, 41, 30), (1, 2, 3, 0, 0, w, h), (2, 3, 4, 0, 0, 12, 23), (2, 3, 4, 12, 0, 4, 23), (2, 3, 4, 0, 23, 12, 8),
             (2, 3, 4, 12, 23, 4, 8), (3, 4, 5, 25, 0, w, h), (3, 1, 6, 3, 2, 17, 6)]
    both([a, b], [(41, 30), (w, h), (w, h)], 2, 30, 40, three)


def test_forty_ragged_jobs_in_one_call_and_one_by_one():
    rng = np.random.default_rng(11)
    src = [H.pattern(H.KINDS[i % 4], int(rng.integers(1, 60)), int(rng.integers(1, 60)), i) for i in range(40)]
    jobs, x = [], [0, 0, 0]
    for i in range(40):                                     # side by side, plane after plane; the last of a plane may be clipped
        p = i % 3
        w, h = (int(v) for v in rng.integers(1, 40, 2))
        if i % 9 == 0:
            w, h = src[i].shape[1], src[i].shape[0]
        jobs.append((0, i, 40 + p, x[p], int(rng.integers(0, 8)), w, h))
        x[p] += w
    width = max(x) - 3
    jobs = [j for j in jobs if j[3] < width]
    together = both(src, [], 3, 44, width, jobs)
    alone = np.zeros_like(together)
    for j in jobs:
        got = collage.resample_np([src[j[1]]], [], 1, 44, width, [(0, 0, 1) + tuple(j[3:])])
        alone[j[2] - 40] |= got[0]
    assert np.array_equal(together, alone)


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN)


@pytest.mark.parametrize("key,dataset,scale", H.RUNS)
def test_crop_collage_equals_the_golden(golden, key, dataset, scale):
    images, classes, boxes, target = H.golden_case(golden, key)
    want = golden[key + ("scale_" if scale else "plain_") + "pixels"]
    # first, on the CPU: does the installed Pillow's own resize still give the golden's pixels?
    plan = collage.plan_collage(images, classes, boxes, target, dataset=dataset, scale=scale)
    crops = [images[i][y0:y1, x0:x1] for i, x0, y0, x1, y1 in plan.crops]
    pillow_now = R.run_jobs_pillow(crops, plan.tmp_wh, plan.n, plan.height, plan.width, plan.jobs)
    got = collage.crop_collage(images, classes, boxes, target, dataset=dataset, scale=scale)
    H.golden_texts(got, golden, key, scale)
    assert np.array_equal(got.images, pillow_now)
    if not np.array_equal(pillow_now, want):
        pytest.skip("Pillow %s resizes differently from Pillow %s, which made the golden: its pixels cannot be asked of the device"
                    % (__import__("PIL").__version__, golden["pillow_version"][0]))
    assert np.array_equal(got.images, want)
