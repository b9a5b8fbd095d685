#!/usr/bin/env python3
"""Cost of the quadratic part of dataset pruning (`dataset_pruning.hamming_neighbours` -> `uda_hash_neighbors_np`; reference
active_learning_loop.py:240-270): matrix maximum and the rows of near-duplicates.

  For two pool sizes - --n-kitti (KITTI's 7 481 training images) and --n-bdd (a BDD100K-sized pool) - of seeded random 64-bit
  hashes (W = 1) with 2 % planted near-duplicates (0 to 5 bits from a random other image), prune_thr 0.1:
    device      one call end to end: upload of the hashes, the four passes, download of the rows; the host clock around the call,
                which ends in a device-to-host copy (a synchronise)
    numpy       a vectorised stand-in on this machine's CPU: np.bitwise_count on blocks of --block rows, one sweep for the maximum
                and one for the rows; it never holds the matrix either.  Timed once per size
    objects     the reference's way at --n-objects hashes only (it is quadratic in Python): an object array of hash values whose
                subtraction counts differing bits, the N x N matrix built one subtraction at a time, its maximum, np.where per row
  Device and numpy must agree entry for entry before their times mean anything.

Wall-clock p50 / mean over --steps calls after --warmup.  Prints ONE JSON line.

    python tools/bench_prune.py [--n-kitti 7481] [--n-bdd 69863] [--n-objects 2000] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THR = 0.1


def synthetic(N, seed=7):
    rng = np.random.default_rng([seed, N])
    words = rng.integers(0, 2 ** 64, N, dtype=np.uint64)
    dup = rng.choice(N, max(1, N // 50), replace=False)
    for i in dup:
        src = int(rng.integers(0, N))
        flips = rng.choice(64, int(rng.integers(0, 6)), replace=False)
        words[i] = words[src] ^ np.bitwise_or.reduce(np.uint64(1) << flips.astype(np.uint64), initial=np.uint64(0))
    return words.reshape(N, 1)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(p50_ms=round(float(np.median(t)), 3), mean_ms=round(float(np.mean(t)), 3))


def numpy_neighbours(words, thr, block):
    col = words.reshape(-1)
    n = col.size
    max_dist = 0
    for i in range(0, n, block):
        max_dist = max(max_dist, int(np.bitwise_count(col[i:i + block, None] ^ col[None, :]).max()))
    lim = max_dist * thr
    counts, cols = [], []
    for i in range(0, n, block):
        r, c = np.nonzero(np.bitwise_count(col[i:i + block, None] ^ col[None, :]) <= lim)
        counts.append(np.bincount(r, minlength=min(block, n - i)))
        cols.append(c.astype(np.int32))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.concatenate(counts))
    return max_dist, off, np.concatenate(cols)


class HashValue:
    """imagehash.ImageHash as far as the loop uses it."""

    def __init__(self, bits):
        self.hash = bits

    def __sub__(self, other):
        return np.count_nonzero(self.hash.flatten() != other.hash.flatten())


def object_loop(bits, thr):
    values = np.empty(len(bits), object)
    values[:] = [HashValue(b) for b in bits]
    matrix = np.asarray([values - values[i] for i in range(len(values))])
    max_dist = np.max(matrix)
    rows = [np.where(matrix[i] <= max_dist * thr)[0] for i in range(len(values))]
    return int(max_dist), rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-kitti", type=int, default=7481)
    ap.add_argument("--n-bdd", type=int, default=69863)
    ap.add_argument("--n-objects", type=int, default=2000)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from uda_amd import dataset_pruning as DP
    res = dict(prune_thr=THR, words=1)
    for name, N in (("kitti", a.n_kitti), ("bdd", a.n_bdd)):
        words = synthetic(N)
        got = DP.hamming_neighbours(words, prune_thr=THR)
        t0 = time.perf_counter()
        want = numpy_neighbours(words, THR, a.block)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        assert got.max_dist == want[0] and np.array_equal(got.row_offsets, want[1]) and np.array_equal(got.indices, want[2]), \
            "device and numpy disagree"
        r = dict(hashes=N, max_dist=got.max_dist, entries=int(got.indices.size), groups=len(DP.duplicate_groups(got)),
                 device=timed(lambda: DP.hamming_neighbours(words, prune_thr=THR), a.steps, a.warmup), numpy_ms=round(numpy_ms, 1))
        r["speedup_vs_numpy"] = round(numpy_ms / r["device"]["p50_ms"], 1)
        res[name] = r
    if a.n_objects > 0:
        words = synthetic(a.n_objects)
        bits = DP.unpack_hashes(words).reshape(-1, 8, 8)
        t0 = time.perf_counter()
        max_dist, rows = object_loop(bits, THR)
        obj_ms = (time.perf_counter() - t0) * 1e3
        got = DP.hamming_neighbours(words, prune_thr=THR)
        assert got.max_dist == max_dist and all(np.array_equal(got.row(i), rows[i]) for i in range(a.n_objects)), \
            "device and the object loop disagree"
        dev = timed(lambda: DP.hamming_neighbours(words, prune_thr=THR), a.steps, a.warmup)
        res["objects"] = dict(hashes=a.n_objects, object_loop_ms=round(obj_ms, 1), device=dev,
                              speedup_vs_objects=round(obj_ms / dev["p50_ms"], 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
