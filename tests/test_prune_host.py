"""Dataset pruning, host side (no GPU): the numpy mirror (tests/prune_ref.py) against what the reference's own
`extract_hash_matrix` returned (tests/golden/prune_golden.npz), the package's host half (`dataset_pruning`: packing, draws,
removal, budget, the strategy branches) against the same fixture with the mirror standing in for the device call, the new
symbol in header / binding / library, its refusals, and the perceptual hash against the DCT formula."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import prune_ref as R
from common import ROOT
from uda_amd import capi
from uda_amd import dataset_pruning as DP

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prune_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
HASHED = [c for c in CASES if "rand" not in str(GOLD[c + "_strategy"])]


def gold_case(c):
    g = {k[len(c) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(c + "_")}
    g["prune_thr"], g["seed"], g["strategy"] = float(g["prune_thr"][0]), int(g["seed"][0]), str(g["strategy"])
    return g


def gold_groups(g):
    return [g["dup_idx"][a:b] for a, b in zip(g["dup_off"][:-1], g["dup_off"][1:])]


def assert_pool(got, g):
    avail, budget, kept = got
    assert np.array_equal(np.asarray(kept, np.int64), g["kept_inds"])
    assert np.array_equal(np.asarray(avail, np.int64), g["avail_after"])
    assert np.array_equal(np.asarray(budget, np.float64), g["budget_after"])      # bit for bit: the same float64 expression


def test_fixture_holds_the_cases_the_tests_rely_on():
    assert set(CASES) == {"main_0125", "main_01", "three", "full", "rand", "wide", "equal"}
    assert GOLD["main_0125_words"].shape == (130, 1) and GOLD["wide_words"].shape == (70, 4) and GOLD["equal_words"].shape == (5, 1)
    assert [int(GOLD[c + "_max_dist"][0]) for c in ("main_0125", "wide", "equal")] == [64, 256, 0]


@pytest.mark.parametrize("c", HASHED)
def test_mirror_reproduces_the_reference_rows(c):
    g = gold_case(c)
    max_dist, off, idx = R.neighbours(g["words"], g["prune_thr"])
    assert max_dist == int(g["max_dist"][0])
    groups, want = R.groups_of(off, idx), gold_groups(g)
    assert len(groups) == len(want) and all(np.array_equal(a, b) for a, b in zip(groups, want))


@pytest.mark.filterwarnings("ignore:divide by zero")        # the all-equal pool ends empty; the reference divides by its length
@pytest.mark.parametrize("c", CASES)
def test_mirror_reproduces_the_reference_outcome(c):
    g = gold_case(c)
    assert_pool(R.prune_pool(g["strategy"], g["words"], g["avail_before"].tolist(), g["budget_before"].tolist(), g["prune_thr"],
                             np.random.RandomState(g["seed"])), g)


def test_inclusive_limit_is_the_float64_product():
    """max_dist 64 * 0.125 = 8.0: the pair at 8 bits is in, the pair at 9 bits is out; 64 * 0.1 = 6.4 drops the pair at 8."""
    in8 = [g.tolist() for g in gold_groups(gold_case("main_0125"))]
    in6 = [g.tolist() for g in gold_groups(gold_case("main_01"))]
    assert [63, 64] in in8 and [30, 100] not in in8 and not any(30 in g for g in in8)
    assert [20, 80] in in6 and [63, 64] not in in6
    assert [40, 41, 110] in in8 and [3, 7, 15] in [g.tolist() for g in gold_groups(gold_case("three"))]


@pytest.fixture
def mirror_device(monkeypatch):
    """The device call of the package replaced by the mirror: what is left is the package's host half."""
    def fake(hashes, prune_thr=None, max_distance=None, device=0, max_entries=1 << 26):
        return DP.Neighbours(*R.neighbours(DP.pack_hashes(hashes), prune_thr, max_distance))
    monkeypatch.setattr(DP, "hamming_neighbours", fake)


@pytest.mark.filterwarnings("ignore:divide by zero")
@pytest.mark.parametrize("c", CASES)
def test_package_host_half_reproduces_the_reference(c, mirror_device):
    g = gold_case(c)
    args = (g["strategy"], None if c == "rand" else g["words"], g["avail_before"].tolist(), g["budget_before"].tolist(), g["prune_thr"])
    assert_pool(DP.prune_pool(*args, rng=np.random.RandomState(g["seed"])), g)
    np.random.seed(g["seed"])                               # rng=None: numpy's global legacy stream, as the reference
    assert_pool(DP.prune_pool(*args), g)
    if c in HASHED:
        nb = DP.hamming_neighbours(g["words"], g["prune_thr"])
        assert all(np.array_equal(a, b) for a, b in zip(DP.duplicate_groups(nb), gold_groups(g)))
        assert len(DP.duplicate_groups(nb)) == len(gold_groups(g))


def test_adjust_budget_and_random_prune_match_the_golden():
    for c in CASES:
        g = gold_case(c)
        if g["kept_inds"].size:
            got = DP.adjust_budget(g["budget_before"].tolist(), g["avail_before"].size, g["kept_inds"].size, "full_prune" in g["strategy"])
            assert np.array_equal(np.asarray(got, np.float64), g["budget_after"]), c
    assert DP.adjust_budget([5, 5], 10, 9, full_prune=True) == [100]
    g = gold_case("rand")
    kept = DP.random_prune(g["avail_before"].size, g["prune_thr"], np.random.RandomState(g["seed"]))
    assert np.array_equal(kept, g["kept_inds"]) and kept.size == int((1 - g["prune_thr"]) * 130)
    assert not np.array_equal(kept, np.sort(kept))          # drawn order, not sorted: available_indices is re-indexed in it


def test_prune_without_groups_keeps_everything_and_draws_nothing(mirror_device):
    words = np.array([0x0, 0xFFFF, 0xFFFF0000, 0xFFFFFFFF00000000], np.uint64)     # pairwise >= 16 bits apart, max 64
    rng = np.random.RandomState(3)
    state = rng.get_state()[1].copy()
    assert np.array_equal(DP.prune(words, 0.1, rng), np.arange(4))
    assert np.array_equal(rng.get_state()[1], state)
    assert np.array_equal(DP.prune(words[:1], 0.5, rng), [0])                      # a pool of one


def test_pack_hashes_round_trips_and_is_order_stable():
    rng = np.random.default_rng(0)
    for s in (8, 16):
        bits = rng.random((9, s, s)) < 0.5
        words = DP.pack_hashes(bits)
        assert words.dtype == np.uint64 and words.shape == (9, s * s // 64) and words.flags.c_contiguous
        assert np.array_equal(DP.unpack_hashes(words).reshape(bits.shape), bits)
        assert np.array_equal(DP.pack_hashes(bits.reshape(9, -1)), words)
        assert np.array_equal(DP.pack_hashes(words), words)

        class Value:                                        # imagehash.ImageHash as far as the package reads it
            def __init__(self, b):
                self.hash = b
        values = [Value(b) for b in bits]
        assert np.array_equal(DP.pack_hashes(values), words)
        boxed = np.empty(9, object)
        boxed[:] = values
        assert np.array_equal(DP.pack_hashes(boxed), words)
        # distances survive the packing
        d = R.distance_matrix(words)
        assert d[2, 7] == np.count_nonzero(bits[2] != bits[7])
    one = np.zeros((1, 8, 8), bool)
    one[0, 0, 0] = True                                     # the first bit is the most significant of word 0
    assert DP.pack_hashes(one)[0, 0] == np.uint64(1) << np.uint64(63)
    one[0, 0, 0], one[0, 7, 7] = False, True
    assert DP.pack_hashes(one)[0, 0] == 1
    wide = np.zeros((1, 16, 16), bool)
    wide[0, 4, 0] = True                                    # bit 64: the first of word 1
    assert DP.pack_hashes(wide)[0].tolist() == [0, 1 << 63, 0, 0]
    assert DP.pack_hashes(np.arange(3, dtype=np.uint64)).shape == (3, 1)
    assert np.array_equal(DP.pack_hashes(np.ones((2, 70), bool)), [[2 ** 64 - 1, 0b111111 << 58]] * 2)    # zero padding
    for bad in (np.zeros((2, 5), np.uint64), np.zeros((2, 2), np.int64), np.zeros((2, 257), bool), np.zeros(4, bool)):
        with pytest.raises(ValueError):
            DP.pack_hashes(bad)


def test_argument_checks_of_the_python_layer():
    w = np.zeros((2, 1), np.uint64)
    for kw in (dict(), dict(prune_thr=0.1, max_distance=3), dict(prune_thr=-0.1), dict(prune_thr=float("nan")),
               dict(prune_thr=float("inf")), dict(max_distance=-1), dict(max_distance=1.5)):
        with pytest.raises(ValueError):
            DP.hamming_neighbours(w, **kw)
    with pytest.raises(ValueError, match="wavelet"):
        DP.hash_files([], method="w")
    with pytest.raises(ValueError, match="3 hashes for a pool of 2"):
        DP.prune_pool("prune_entropy", np.zeros(3, np.uint64), [0, 1], [50, 50], 0.1)


# ---- the C ABI
def test_header_binding_and_library_agree_on_the_new_symbol():
    header = open(os.path.join(ROOT, "include", "uda_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int uda_hash_neighbors_np\(([^)]*)\);", code)
    assert m, "the header does not declare uda_hash_neighbors_np"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["int32_t device", "const uint64_t* hashes", "int32_t N", "int32_t W", "double prune_thr", "int32_t max_distance",
                      "int64_t cap", "int32_t* max_dist", "int64_t* row_off", "int32_t* idx", "int64_t* total"]
    res, args = capi._SIGNATURES["uda_hash_neighbors_np"]
    assert res is C.c_int and len(args) == len(params)
    assert [args[i] for i in (0, 2, 3, 4, 5, 6)] == [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int64]
    assert "uda_hash_neighbors_np <-" in header             # the map of entry points to reference lines
    defs = dict(re.findall(r"#define (UDA_PRUNE_[A-Z_]+) (\d+)", header))
    assert (int(defs["UDA_PRUNE_ROWS"]), int(defs["UDA_PRUNE_COLS"]), int(defs["UDA_PRUNE_MAX_N"])) == \
        (capi.PRUNE_ROWS, capi.PRUNE_COLS, capi.PRUNE_MAX_N)
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    assert hasattr(C.CDLL(capi.LIB_PATH), "uda_hash_neighbors_np")


def test_library_refuses_bad_arguments_before_it_touches_a_device():
    lib = capi.load()
    w = np.zeros((4, 4), np.uint64)
    off, md, tot = np.zeros(5, np.int64), C.c_int32(), C.c_int64()

    def call(hashes=w.ctypes.data, N=4, W=1, thr=0.1, maxd=-1, cap=0, md_p=C.byref(md), off_p=off.ctypes.data, tot_p=C.byref(tot)):
        rc = lib.uda_hash_neighbors_np(0, hashes, N, W, thr, maxd, cap, md_p, off_p, None, tot_p)
        return rc, lib.uda_last_error(None).decode()

    for kw, words in ((dict(N=0), "0 hashes, 1..1048576"), (dict(N=capi.PRUNE_MAX_N + 1), "1048577 hashes"), (dict(N=-3), "-3 hashes"),
                      (dict(W=0), "0 words per hash, 1..4"), (dict(W=5), "5 words per hash"), (dict(hashes=None), "NULL input"),
                      (dict(off_p=None), "NULL input"), (dict(tot_p=None), "NULL input"), (dict(md_p=None), "NULL input"),
                      (dict(cap=-1), "cap -1"), (dict(thr=-0.5), "prune_thr -0.5 is negative or not finite"),
                      (dict(thr=float("nan")), "negative or not finite"), (dict(thr=float("inf")), "negative or not finite")):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("uda_hash_neighbors_np: ") and words in msg, (kw, rc, msg)


def test_fails_loudly_without_gpu():
    """Valid arguments, no HIP device: 1 and the entry point's name in front of HIP's own words, like its siblings; also with an
    absolute limit, where a bad prune_thr is not looked at."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import ctypes as C\n"
            "import numpy as np\n"
            "from uda_amd import capi\n"
            "lib = capi.load()\n"
            "w = np.arange(4, dtype=np.uint64); off = np.zeros(5, np.int64); idx = np.zeros(16, np.int32)\n"
            "md, tot = C.c_int32(), C.c_int64()\n"
            "for thr, maxd in ((0.1, -1), (-1.0, 2)):\n"
            "    rc = lib.uda_hash_neighbors_np(0, w.ctypes.data, 4, 1, thr, maxd, 16, C.byref(md), off.ctypes.data, idx.ctypes.data,\n"
            "                                   C.byref(tot))\n"
            "    print('%%d|%%s' %% (rc, lib.uda_last_error(None).decode()))\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [line.split("|", 1) for line in out.stdout.splitlines() if "|" in line]
    assert len(rows) == 2, out.stdout
    for rc, msg in rows:
        assert rc == "1" and msg.startswith("uda_hash_neighbors_np:") and "no ROCm-capable device is detected" in msg, (rc, msg)


# ---- the perceptual hash (host code; imagehash itself is not available to compare with)
def dct2_unnormalised(x):
    """scipy.fftpack.dct type 2, norm=None, along axis 0 then axis 1: y[k] = 2 sum_n x[n] cos(pi k (2 n + 1) / (2 N))."""
    n = x.shape[0]
    k = np.arange(n)
    basis = 2.0 * np.cos(np.pi * k[:, None] * (2 * k[None, :] + 1) / (2 * n))
    return basis @ x.astype(np.float64) @ basis.T


def test_phash_on_a_32x32_grey_image_is_the_dct_formula():
    from PIL import Image
    px = np.random.default_rng(4).integers(0, 128, (32, 32), dtype=np.uint8)
    got = DP.phash(Image.fromarray(px))
    assert got.shape == (8, 8) and got.dtype == np.bool_
    low = dct2_unnormalised(px)[:8, :8]
    margin = np.abs(low - np.median(low)).min()
    assert margin > 1e-6                                    # no coefficient sits on the median: float summation order cannot flip a bit
    assert np.array_equal(got, low > np.median(low))
    assert np.array_equal(DP.phash(px), got)                # an array is taken as an image
    assert np.array_equal(DP.phash(Image.fromarray(px)), got)                 # deterministic
    assert np.array_equal(DP.phash(Image.fromarray((px * 2).astype(np.uint8))), got)   # exact doubling: every coefficient doubles
    assert DP.pack_hashes(got[None]).shape == (1, 1)


def test_hash_files_resizes_then_hashes(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    paths = []
    for i in range(3):
        p = tmp_path / ("im%d.png" % i)
        Image.fromarray(rng.integers(0, 256, (40 + i, 70, 3), dtype=np.uint8)).save(p)
        paths.append(str(p))
    words = DP.hash_files(paths + paths[:1])
    assert words.shape == (4, 1) and words.dtype == np.uint64 and words[0, 0] == words[3, 0] and len(set(words[:3, 0].tolist())) == 3
    with Image.open(paths[1]) as im:
        assert np.array_equal(DP.pack_hashes(DP.phash(im.resize((512, 256)))[None]), words[1:2])
    assert DP.hash_files([]).shape == (0, 1)
