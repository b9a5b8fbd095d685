"""Generates tests/golden/prune_golden.npz by running the REAL reference method `ActiveLearning.extract_hash_matrix`
(src/active_learning_loop.py:198-316) on hash values made here.  Its body is numpy only; the module imports TensorFlow and
friends at the top, which are stubbed.  Run once where a checkout of the reference exists; the .npz (data only) is committed and
is what the tests read.

    python tests/golden/make_prune_golden.py <src directory of the reference's checkout>

The object is built with `__new__` and given the attributes the method reads (im_names, available_indices, scoring_strategy,
data_dir, hash_method, iteration_budget); `prune_thr` and `hash_method` are module globals of the reference and are set on the
module.  <data_dir>/p_hash_ims.npy is saved beforehand with a stand-in for imagehash.ImageHash (`.hash`, `__sub__` = number of
differing bits), so the method loads hashes instead of opening images.  np.random is seeded per case.

One shim, in this maker only: the reference hands np.save the ragged list `duplicates`, which numpy >= 1.24 refuses; here np.save
wraps such a list into an object array first.

Stored per case k<i>_: words (uint64 [N, W], dataset_pruning.pack_hashes' order), prune_thr, seed, strategy, budget_before /
budget_after, avail_before / avail_after, kept_inds, max_dist (the matrix maximum) and the saved `duplicates` as dup_off / dup_idx."""
import os
import sys
import tempfile
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_prune_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
for name in ("tensorflow", "tensorflow_probability", "uncertainty_toolbox", "uncertainty_toolbox.viz", "absl", "absl.logging",
             "imagehash", "uncertainty_analysis", "cv2", "datasets", "datasets.BDD100K", "datasets.BDD100K.bdd_tf_creator",
             "datasets.KITTI", "datasets.KITTI.kitti_tf_creator"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np                       # noqa: E402
import active_learning_loop as ALL      # noqa: E402  (the reference module)
import prune_ref as R                    # noqa: E402  (only to assert the planted structure)
from uda_amd import dataset_pruning as DP   # noqa: E402  (pack_hashes: the fixture holds the package's word order)

AL = ALL.ActiveLearning
BUDGET = [5, 5, 5, 10, 20, 30, 25]


class StubHash:
    """What the method needs of imagehash.ImageHash."""

    def __init__(self, bits):
        self.hash = np.asarray(bits, bool)

    def __sub__(self, other):
        return int(np.count_nonzero(self.hash.flatten() != other.hash.flatten()))


def flip(bits, where):
    out = bits.copy().reshape(-1)
    out[list(where)] ^= True
    return out.reshape(bits.shape)


def pool_main(rng):
    """N = 130, hash size 8: a complementary pair (max_dist 64) and copies at distances 0, 3, 8 and 9 whose members lie on both
    sides of index 64, and a three-member group; every other pair is further apart than 9 bits."""
    b = rng.random((130, 8, 8)) < 0.5
    b[120] = ~b[5]
    b[70] = b[10]
    b[80] = flip(b[20], (0, 31, 63))
    b[64] = flip(b[63], range(8, 16))
    b[100] = flip(b[30], range(40, 49))
    b[41] = flip(b[40], (1, 2))
    b[110] = flip(b[40], (61, 62))
    return b


def pool_three(rng):
    b = rng.random((20, 8, 8)) < 0.5
    b[7] = flip(b[3], (5,))
    b[15] = flip(b[3], (6,))
    return b


def pool_wide(rng):
    """N = 70, hash size 16 (W = 4): copies that differ in the last word only, in the first only, and across all four."""
    b = rng.random((70, 16, 16)) < 0.5
    b[69] = ~b[0]
    b[65] = flip(b[2], (255,))
    b[40] = flip(b[33], (0, 64, 128, 192))
    b[50] = flip(b[12], range(200, 232))
    b[51] = flip(b[12], range(200, 233))
    return b


def pool_equal(rng):
    return np.repeat(rng.random((1, 8, 8)) < 0.5, 5, axis=0)


# name, pool, strategy, prune_thr, seed
CASES = [("main_0125", pool_main, "prune_entropy", 0.125, 11), ("main_01", pool_main, "prune_entropy", 0.1, 12),
         ("three", pool_three, "prune_mean_alluncert", 0.05, 13), ("full", pool_main, "full_prune_entropy", 0.125, 14),
         ("rand", pool_main, "prune_rand", 0.3, 15), ("wide", pool_wide, "prune_entropy", 0.125, 16),
         ("equal", pool_equal, "prune_entropy", 0.1, 17)]


def save_shim(real):
    def save(file, arr, *args, **kw):
        if isinstance(arr, list) and arr and isinstance(arr[0], np.ndarray):
            boxed = np.empty(len(arr), object)
            boxed[:] = arr
            arr = boxed
        return real(file, arr, *args, **kw)
    return save


def run_reference(bits, strategy, thr, seed, td):
    n = bits.shape[0]
    hashes = np.empty(n, object)
    hashes[:] = [StubHash(b) for b in bits]
    np.save(os.path.join(td, "p_hash_ims.npy"), hashes, allow_pickle=True)
    ALL.prune_thr, ALL.hash_method = thr, "p"
    obj = AL.__new__(AL)
    obj.im_names = ["%06d.png" % i for i in range(3 * n + 2)]
    obj.available_indices = [3 * i + 1 for i in range(n)]
    obj.scoring_strategy, obj.data_dir, obj.hash_method, obj.iteration_budget = strategy, td, "p", list(BUDGET)
    np.random.seed(seed)
    with mock.patch.object(np, "save", save_shim(np.save)):
        names, n_after, kept = obj.extract_hash_matrix(n)
    assert names == [obj.im_names[3 * i + 1] for i in range(n)] and n_after == len(obj.available_indices)
    out = {"kept_inds": np.asarray(kept, np.int64), "avail_before": np.asarray([3 * i + 1 for i in range(n)], np.int64),
           "avail_after": np.asarray(obj.available_indices, np.int64), "budget_before": np.asarray(BUDGET, np.int64),
           "budget_after": np.asarray(obj.iteration_budget, np.float64)}
    if "rand" not in strategy:
        dup = np.load(os.path.join(td, "p_prune_duplicates_thr%s.npy" % thr), allow_pickle=True)
        dup = [np.asarray(g, np.int64) for g in dup]
        out["dup_off"] = np.concatenate([[0], np.cumsum([g.size for g in dup])]).astype(np.int64)
        out["dup_idx"] = np.concatenate(dup).astype(np.int64) if dup else np.zeros(0, np.int64)
        out["max_dist"] = np.array([int(np.max(obj.dist_matrix))])
    return out


def main():
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, pool, strategy, thr, seed in CASES:
        bits = pool(np.random.default_rng(20241019))
        words = DP.pack_hashes(bits)
        with tempfile.TemporaryDirectory() as td:
            got = run_reference(bits, strategy, thr, seed, td)
        got.update(words=words, prune_thr=np.array([thr]), seed=np.array([seed]), strategy=np.array(strategy))
        for k, v in got.items():
            out["%s_%s" % (name, k)] = v
        print("%-10s N %3d W %d  thr %-5s  max_dist %s  groups %s  kept %d  budget %s" % (
            name, words.shape[0], words.shape[1], thr, got.get("max_dist"), len(got["dup_off"]) - 1 if "dup_off" in got else "-",
            got["kept_inds"].size, got["budget_after"].tolist()))
    # the planted structure the tests rely on
    d = R.distance_matrix(out["main_0125_words"]).astype(int)
    assert d.max() == 64 and d[5, 120] == 64
    assert (d[10, 70], d[20, 80], d[63, 64], d[30, 100], d[40, 41], d[40, 110], d[41, 110]) == (0, 3, 8, 9, 2, 2, 4)
    planted = {(10, 70), (20, 80), (63, 64), (30, 100), (40, 41), (40, 110), (41, 110)}
    far = [d[i, j] for i in range(130) for j in range(i + 1, 130) if (i, j) not in planted]
    assert min(far) > 9, min(far)
    g = lambda name: [out[name + "_dup_idx"][a:b].tolist() for a, b in zip(out[name + "_dup_off"][:-1], out[name + "_dup_off"][1:])]  # noqa: E731
    assert [63, 64] in g("main_0125") and [30, 100] not in g("main_0125")          # limit 8.0: distance 8 in, 9 out
    assert [20, 80] in g("main_01") and [63, 64] not in g("main_01")               # limit 6.4
    assert [40, 41, 110] in g("main_0125") and [3, 7, 15] in g("three")
    assert out["full_budget_after"].tolist() == [100] and out["rand_kept_inds"].size == int((1 - 0.3) * 130)
    dw = R.distance_matrix(out["wide_words"]).astype(int)
    assert dw.max() == 256 and (dw[2, 65], dw[33, 40], dw[12, 50], dw[12, 51]) == (1, 4, 32, 33)
    assert [12, 50] in g("wide") and [50, 51] in g("wide") and [12, 50, 51] in g("wide")   # limit 32.0: 12-51 (33 bits) is out
    assert out["equal_max_dist"][0] == 0 and len(g("equal")) == 5
    dst = os.path.join(HERE, "prune_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 100000


if __name__ == "__main__":
    main()
