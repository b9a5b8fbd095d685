"""Dataset pruning on the device (`dataset_pruning.hamming_neighbours` / `prune` / `prune_pool` -> `uda_hash_neighbors_np`;
reference active_learning_loop.py:198-316): the C entry point and the package against the numpy mirror (tests/prune_ref.py)
entry for entry at every size where the tiling changes (rows per block, columns per staged chunk, from include/uda_hip.h) with
pairs planted across those boundaries, the inclusive limit, the absolute limit, the capacity protocol, and the reference's own
outcomes (tests/golden/prune_golden.npz).  Everything is integer-exact: there is no tolerance anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prune_ref as R
from common import ROOT
from uda_amd import capi
from uda_amd import dataset_pruning as DP

pytestmark = pytest.mark.gpu

_DEFS = dict(re.findall(r"#define (UDA_PRUNE_[A-Z_]+) (\d+)", open(os.path.join(ROOT, "include", "uda_hip.h")).read()))
ROWS, COLS = int(_DEFS["UDA_PRUNE_ROWS"]), int(_DEFS["UDA_PRUNE_COLS"])
SIZES = [1, 2, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, COLS - 1, COLS, COLS + 1, 2 * COLS + 3]
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prune_golden.npz"))
GOLD_CASES = [str(c) for c in GOLD["cases"]]
SENTINEL = -7


def planted_pairs(L):
    """(row, column, bits apart): L is the limit the test will use - L is in, L + 1 is out."""
    return [(63, 64, L),                          # across the wave boundary
            (ROWS - 1, COLS, L),                  # last row of block 0 x first column of chunk 1
            (ROWS, COLS - 1, L + 1),              # first row of block 1 x last column of chunk 0
            (ROWS + 1, 2 * COLS, L),              # x first column of chunk 2
            (COLS + 1, 2 * COLS + 1, L + 1),
            (3 * ROWS - 1, 3 * ROWS, 0),          # an exact copy across a row-block boundary
            (1, 2, L + 1)]


def pool(N, W, L, seed=0):
    """Seeded random hashes with the planted pairs that fit (the copy differs from its original in the LAST word only) and, from
    N = 8, a complementary pair (max_dist = 64 W) whose second member is the highest free index: block and chunk of the maximum
    lie far from the diagonal, on the side the symmetric maximum pass skips."""
    rng = np.random.default_rng([N, W, seed])
    words = rng.integers(0, 2 ** 64, (N, W), dtype=np.uint64)
    pairs = [(a, b, d) for a, b, d in planted_pairs(L) if a < N and b < N]
    for a, b, d in pairs:
        words[b] = words[a]
        words[b, W - 1] ^= np.uint64((1 << d) - 1)
    if N >= 8:
        used = {i for a, b, _ in pairs for i in (a, b)} | {5}
        far = max(i for i in range(N) if i not in used)
        words[far] = ~words[5]
    return words, pairs


def raw(words, prune_thr=0.0, max_distance=-1, cap=None, want_idx=True, device=0):
    """One call of the C entry point: (rc, max_dist, row_off, idx buffer, total).  cap=None: room for every pair."""
    lib = capi.load()
    n, w = words.shape
    cap = n * n if cap is None else cap
    idx = np.full(max(cap, 1), SENTINEL, np.int32)
    off = np.full(n + 1, SENTINEL, np.int64)
    md, tot = C.c_int32(SENTINEL), C.c_int64(SENTINEL)
    rc = lib.uda_hash_neighbors_np(device, words.ctypes.data, n, w, prune_thr, max_distance, cap, C.byref(md), off.ctypes.data,
                                   idx.ctypes.data if want_idx else None, C.byref(tot))
    assert rc == 0, lib.uda_last_error(None).decode()
    return md.value, off, idx, tot.value


def assert_equals_mirror(got, want):
    md, off, idx, tot = got
    wmd, woff, widx = want
    print("max_dist %d / %d, total %d / %d" % (md, wmd, tot, woff[-1]))
    assert md == wmd and tot == woff[-1]
    assert np.array_equal(off, woff)
    assert np.array_equal(idx[:tot], widx) and (idx[tot:] == SENTINEL).all()


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("N", SIZES)
def test_entry_point_equals_the_mirror(N, W):
    """prune_thr 0.125: from N = 8 the limit is 64 W / 8 bits exactly, the distance of the planted pairs; their twins one bit
    further out stay outside.  A second call gives the same arrays; the package's wrapper returns them too."""
    L = 8 * W
    words, pairs = pool(N, W, L)
    want = R.neighbours(words, 0.125)
    got = raw(words, 0.125)
    assert_equals_mirror(got, want)
    if N >= 8:
        assert got[0] == 64 * W
        for a, b, d in pairs:
            row = got[2][got[1][a]:got[1][a + 1]]
            assert (b in row) == (d <= L) and a in row and (np.diff(row) > 0).all(), (a, b, d, row)
    again = raw(words, 0.125)
    assert again[0] == got[0] and again[3] == got[3] and np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2])
    md, off, idx = DP.hamming_neighbours(words, prune_thr=0.125)
    assert md == want[0] and np.array_equal(off, want[1]) and np.array_equal(idx, want[2]) and idx.dtype == np.int32


def test_spans_of_several_chunks_equal_the_mirror():
    """N = 12301: 49 row blocks and 25 column chunks, more blocks than the grid takes, so a block walks a span of two chunks
    (the last span has one).  Pairs planted across span ends; W = 1."""
    N, L = 12301, 8
    words, _ = pool(N, 1, L, seed=1)
    extra = [(ROWS - 1, 2 * COLS, L), (2 * COLS - 1, 24 * COLS, L), (24 * COLS - 1, 24 * COLS + 7, L + 1), (N - 3, 4 * COLS - 1, L)]
    for a, b, d in extra:
        words[b] = words[a] ^ np.uint64((1 << d) - 1)
    want = R.neighbours_blocked(words, 0.125)
    assert want[0] == 64
    got = raw(words, 0.125, cap=4 * N)
    assert_equals_mirror(got, want)
    for a, b, d in extra:
        assert (b in got[2][got[1][a]:got[1][a + 1]]) == (d <= L) and (a in got[2][got[1][b]:got[1][b + 1]]) == (d <= L)


@pytest.mark.parametrize("W", [1, 4])
def test_threshold_zero_keeps_exact_copies_only(W):
    N = 2 * COLS + 3
    words, pairs = pool(N, W, 8 * W)
    got = raw(words, 0.0)
    assert_equals_mirror(got, R.neighbours(words, 0.0))
    assert got[3] == N + 2                                  # the diagonal and the one exact copy, seen from both sides
    assert got[2][got[1][3 * ROWS - 1]:got[1][3 * ROWS]].tolist() == [3 * ROWS - 1, 3 * ROWS]


def test_all_equal_pool():
    words = np.full((65, 1), 0x0123456789ABCDEF, np.uint64)
    md, off, idx, tot = raw(words, 0.1)
    assert md == 0 and tot == 65 * 65 and np.array_equal(off, np.arange(66) * 65)
    assert np.array_equal(idx[:tot].reshape(65, 65), np.tile(np.arange(65, dtype=np.int32), (65, 1)))


@pytest.mark.parametrize("W", [1, 4])
def test_absolute_limit(W):
    """max_distance >= 0: that many bits, inclusive; prune_thr is not read (a NaN there is not even refused)."""
    N, L = COLS + 1, 8 * W
    words, pairs = pool(N, W, L)
    for lim in (L, L + 1, 0, 64 * W):
        if lim == 64 * W:
            words = words[:65]
        got = raw(words, float("nan"), max_distance=lim)
        assert_equals_mirror(got, R.neighbours(words, max_distance=lim))
        if lim == 64 * W:
            assert got[3] == 65 * 65
    md, off, idx = DP.hamming_neighbours(words, max_distance=L)
    want = R.neighbours(words, max_distance=L)
    assert md == want[0] and np.array_equal(off, want[1]) and np.array_equal(idx, want[2])


def test_short_cap_leaves_idx_untouched_and_count_only_call():
    words, _ = pool(COLS + 1, 1, 8)
    want = R.neighbours(words, 0.125)
    total = int(want[1][-1])
    md, off, idx, tot = raw(words, 0.125, cap=total - 1)
    assert md == want[0] and tot == total and np.array_equal(off, want[1]) and (idx == SENTINEL).all()
    md, off, idx, tot = raw(words, 0.125, cap=0, want_idx=False)
    assert md == want[0] and tot == total and np.array_equal(off, want[1])
    md, off, idx, tot = raw(words, 0.125, cap=total)        # exactly enough
    assert np.array_equal(idx[:total], want[2])


def test_wrapper_retries_once_and_refuses_a_threshold_that_keeps_every_pair():
    words = np.full((100, 1), 7, np.uint64)                 # 10 000 entries: more than the first guess of the wrapper (4096)
    nb = DP.hamming_neighbours(words, prune_thr=0.5)
    assert nb.max_dist == 0 and nb.indices.size == 10000 and np.array_equal(nb.row(99), np.arange(100))
    with pytest.raises(ValueError, match="keeps nearly every pair"):
        DP.hamming_neighbours(words, prune_thr=0.5, max_entries=9999)
    assert DP.hamming_neighbours(words, prune_thr=0.5, max_entries=10000).indices.size == 10000


@pytest.mark.parametrize("W", [1, 4])
def test_prune_equals_the_mirror(W):
    N = 2 * COLS + 3
    words, _ = pool(N, W, 8 * W)
    _, off, idx = R.neighbours(words, 0.125)
    want = R.kept_from_groups(R.groups_of(off, idx), N, np.random.RandomState(21))
    got = DP.prune(words, 0.125, np.random.RandomState(21))
    assert 0 < N - want.size <= 8 and np.array_equal(got, want)
    np.random.seed(21)
    assert np.array_equal(DP.prune(words, 0.125), want)


@pytest.mark.filterwarnings("ignore:divide by zero")        # the all-equal pool ends empty; the reference divides by its length
@pytest.mark.parametrize("c", GOLD_CASES)
def test_prune_pool_reproduces_the_reference(c):
    g = {k[len(c) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(c + "_")}
    strategy, thr, seed = str(g["strategy"]), float(g["prune_thr"][0]), int(g["seed"][0])
    np.random.seed(seed)
    avail, budget, kept = DP.prune_pool(strategy, g["words"], g["avail_before"].tolist(), g["budget_before"].tolist(), thr)
    assert np.array_equal(np.asarray(kept, np.int64), g["kept_inds"])
    assert np.array_equal(np.asarray(avail, np.int64), g["avail_after"])
    assert np.array_equal(np.asarray(budget, np.float64), g["budget_after"])
    if "rand" not in strategy:
        nb = DP.hamming_neighbours(g["words"], prune_thr=thr)
        groups = DP.duplicate_groups(nb)
        assert nb.max_dist == int(g["max_dist"][0]) and len(groups) == g["dup_off"].size - 1
        assert np.array_equal(np.concatenate(groups), g["dup_idx"])
