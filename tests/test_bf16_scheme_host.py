"""CPU tests of the one-piece bf16 scheme (`UDA_PW_SCHEME=bf16` / `uda_pw_scheme = "bf16"`, UDA_SPLIT_BF16X1 = 6): the switch,
the planner under it, the binding against the header, the shipped code objects of its kernels, and the rounding-exact model
(tests/bf16x1_ref.py) the GPU tests hold the kernels to."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from common import FULL_MC, HEAD_MC, ROOT, make_params, make_weights


@pytest.fixture
def clean_env(monkeypatch):
    monkeypatch.delenv("UDA_PW_SCHEME", raising=False)
    monkeypatch.delenv("UDA_PW_TERMS", raising=False)
    return monkeypatch


def _plan(p, w, scheme=None):
    from uda_amd import plan
    return plan.Plan(dict(p, uda_pw_scheme=scheme) if scheme else p, w, chunk_images=2, max_images=2)


def test_pw_scheme_reads_bf16(clean_env):
    from uda_amd import plan
    clean_env.setenv("UDA_PW_SCHEME", "bf16")
    assert plan.pw_scheme() == "bf16"
    assert plan.PW_SCHEMES == ("f16x2", "bf16x3", "bf16x2", "f32", "f16")       # unchanged: the new name lives in PW_SCHEMES_ALL
    assert plan.PW_SCHEMES_ALL == plan.PW_SCHEMES + ("bf16",)
    assert plan.PW_SCHEME_CODES["bf16"] == 6
    assert plan.split_pieces("bf16") == 1 and plan.split_pieces("f16") == 1 and plan.split_pieces("bf16x2") == 2
    p = make_params(**FULL_MC)
    assert _plan(p, make_weights(p)).pw_scheme == "bf16"        # the process default reaches a handle without a scheme of its own
    for bad in ("f8", "fp8"):
        clean_env.setenv("UDA_PW_SCHEME", bad)
        with pytest.raises(ValueError, match="UDA_PW_SCHEME"):
            plan.pw_scheme()


@pytest.mark.parametrize("mc", ["full", "head"])
def test_plan_matches_f16(clean_env, mc):
    """The cost structure of f16: the same ops on the same buffers, the arena laid out alike."""
    p = make_params(**(FULL_MC if mc == "full" else HEAD_MC))
    w = make_weights(p, seed=1)
    a, b = _plan(p, w, "f16"), _plan(p, w, "bf16")
    assert b.pw_scheme == "bf16" and b.to_c()[0].pw_scheme == 6 and a.to_c()[0].pw_scheme == 5
    key = lambda bf: (bf.H, bf.W, bf.C, bf.per_sample, bf.kind, bf.level, bf.offset, bf.name)
    assert [key(bf) for bf in a.bufs] == [key(bf) for bf in b.bufs]
    assert len(a.ops) == len(b.ops) and a.arena_floats == b.arena_floats
    for x, y in zip(a.ops, b.ops):
        assert x == y


@pytest.mark.parametrize("mc", ["full", "head"])
def test_exactly_the_fused_front_halves_outputs_are_bf16(clean_env, mc):
    from uda_amd import capi
    p = make_params(**(FULL_MC if mc == "full" else HEAD_MC))
    w = make_weights(p, seed=1)
    pl = _plan(p, w, "bf16")
    mbx_out = {o["out"] for o in pl.ops if o["kind"] == capi.OP_MBX}
    marked = {i for i, b in enumerate(pl.bufs) if b.storage == "bf16"}
    assert mbx_out and marked == mbx_out
    assert all(b.storage in ("bf16", "f32") for b in pl.bufs)          # nothing is marked "f16"
    # and the f16 marks are the same buffers under their own name
    assert {i for i, b in enumerate(_plan(p, w, "f16").bufs) if b.storage == "f16"} == marked


def test_support_mirrors_equal_the_f16_answers():
    from uda_amd import plan
    for c in (64, 112):
        for cout in (c, 36, 63, 72, 144):
            assert plan.sep_tin_supported(c, cout, "bf16") == plan.sep_tin_supported(c, cout, "f16"), (c, cout)
            assert plan.sepf_supported(c, cout, "bf16") == plan.sepf_supported(c, cout, "f16"), (c, cout)
        assert plan.sep_tin_supported(c, c, "bf16") and plan.sepf_supported(c, c, "bf16")
        for k in (3, 5):
            for stride in (1, 2):
                assert plan.mbx_supported(c, 6 * c, k, stride, "bf16") == plan.mbx_supported(c, 6 * c, k, stride, "f16")
                assert plan.mbx_tiles(24, 40, k, stride, c, "bf16") == plan.mbx_tiles(24, 40, k, stride, c, "f16")
    assert plan.mbx_supported(24, 144, 3, 1, "bf16") and plan.mbx_tiles(35, 51, 3, 1, 24, "bf16") == plan.mbx_tiles(35, 51, 3, 1, 24, "f16")


def test_driver_accepts_bf16(clean_env):
    """`uda_pw_scheme = "bf16"` reaches the handle's creation in the model struct (code 6), not through the environment, which
    is untouched while the handle is created; an unknown value is still refused before anything is created."""
    from uda_amd import capi
    from uda_amd.infer_lib import KerasDriver
    seen = []

    class Lib:
        def uda_create(self, model, *rest):
            seen.append((os.environ.get("UDA_PW_SCHEME"), os.environ.get("UDA_PW_TERMS"), model._obj.pw_scheme))
            return 0
    clean_env.setattr(capi, "load", lambda: Lib())
    p = make_params(**FULL_MC)
    w = make_weights(p)
    d = KerasDriver("_", False, p["name"], 1, False, dict(p, uda_pw_scheme="bf16"), weights=w)
    assert seen == [(None, None, 6)]
    assert d.pw_scheme == "bf16" and d.plan.pw_scheme == "bf16" and d.plan.to_c()[0].pw_scheme == 6
    assert "UDA_PW_SCHEME" not in os.environ and "UDA_PW_TERMS" not in os.environ
    for bad in ("f8", "fp8"):
        with pytest.raises(ValueError, match="uda_pw_scheme"):
            KerasDriver("_", False, p["name"], 1, False, dict(p, uda_pw_scheme=bad), weights=w)
    assert len(seen) == 1
    # mixed_precision / strategy stay inert: the scheme is not derived from them
    q = dict(p, mixed_precision=True, strategy="tpu")
    assert _plan(q, w).pw_scheme == "f16x2"


def test_header_enum_equals_the_binding():
    from uda_amd import plan
    text = open(os.path.join(ROOT, "include", "uda_hip.h")).read()
    body = re.search(r"enum uda_pw_scheme \{(.*?)\};", text, re.S).group(1)
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"(UDA_SPLIT_\w+)\s*=\s*(\d+)", body)}
    assert enum == {"UDA_SPLIT_NONE": 0, "UDA_SPLIT_BF16X2": 2, "UDA_SPLIT_BF16X3": 3, "UDA_SPLIT_F16X2": 4, "UDA_SPLIT_F16X1": 5,
                    "UDA_SPLIT_BF16X1": 6}
    assert enum["UDA_SPLIT_BF16X1"] == plan.PW_SCHEME_CODES["bf16"]
    assert sorted(enum.values()) == sorted(plan.PW_SCHEME_CODES.values())


def test_library_exports_and_holds_the_bf16_kernels():
    """The cross-compiled library exports what it did before and holds the one-piece bf16 instantiation of every
    split-precision kernel, beside its fp16 twin."""
    from uda_amd import capi
    assert os.path.exists(capi.LIB_PATH), "libuda_hip.so not built"
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [n for n in capi.EXPORTS if not hasattr(lib, n)] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "codeobj.py"), "resources", "--lib", capi.LIB_PATH],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = r.stdout
    for k in ("pwb_kernel<1, 1, 4, 1, %d,", "pws_kernel<%d, 1, true, false>", "pws_kernel<%d, 2, false, true>",
              "w0gate_kernel<%d>", "mbxb_kernel<3, 1, 2, true, %d, false>", "mbxb_kernel<3, 1, 2, true, %d, true>",
              "mbxd_kernel<5, 14, %d, 1, false, false>", "mbxd_kernel<5, 14, %d, 1, false, true>", "sep_kernel<2, %d, 2, 1>",
              "sep_kernel<4, %d, 2, 2>", "sep_kernel<2, %d, 3, 0>", "sepf_kernel<2, %d, true, 16>"):
        assert k % 5 in names and k % 6 in names, k


# ---------------------------------------------------------------- the model on its own
def _operands(seed, m=40, k=88, n=24):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (m, k)).astype(np.float32), (rng.normal(0, 1, (k, n)) / np.sqrt(k)).astype(np.float32)


def test_model_separates_rounding_models():
    """On random operands the model differs from the one-piece fp16 model and from the exact-operand product by more than
    its bound on most outputs: the bound (float32 accumulation error) is far below either operand rounding."""
    import bf16x1_ref as B
    from oracle import split_ref as S
    a, b = _operands(1)
    val, bnd = B.contract(a, b)
    f16, _ = S.contract(a, b, S.F16X1)
    exact = a.astype(np.float64) @ b.astype(np.float64)
    assert (np.abs(val - f16) > bnd).mean() > 0.9
    assert (np.abs(val - exact) > bnd).mean() > 0.9
    # ... and it is the bf16 rounding of the operands, nothing coarser: relative to the summed magnitudes, within 2 x 2^-9
    mag = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    assert (np.abs(val - exact) <= 2.0 ** -8 * mag).all()
    ex, _ = B.contract(a, b, exact_operands=True)
    np.testing.assert_array_equal(ex, _ksteps(a.astype(np.float64), b.astype(np.float64)))


def _ksteps(a, b):
    out = np.zeros((a.shape[0], b.shape[1]))
    for k0 in range(0, a.shape[1], 16):
        out += a[:, k0:k0 + 16] @ b[k0:k0 + 16]
    return out


def test_model_is_exact_on_bf16_operands():
    import bf16x1_ref as B
    from oracle import split_ref as S
    a, b = _operands(2)
    a, b = S.bf16_rne(a), S.bf16_rne(b)
    val, bnd = B.contract(a, b)
    np.testing.assert_array_equal(val, _ksteps(a.astype(np.float64), b.astype(np.float64)))
    assert (bnd > 0).all()
    y, _ = B.pointwise(a[None], b, None, None, None, None, None, None, 1, False)
    np.testing.assert_array_equal(y[0], val)


@pytest.mark.parametrize("big", [1e6, 1e30])
def test_model_stays_finite_far_above_fp16_range(big):
    import bf16x1_ref as B
    from oracle import split_ref as S
    a, b = _operands(3)
    x = a[None].copy()
    x[0, 7, 5] = big
    sc, sh = np.full(24, 0.75, np.float32), np.full(24, 0.1, np.float32)
    y, bnd = B.pointwise(x, b, None, sc, sh, None, None, None, 1, True)
    assert np.isfinite(y).all() and np.isfinite(bnd).all()
    with np.errstate(all="ignore"):
        h, _ = S.pointwise(x, b, None, sc, sh, None, None, None, 1, True, S.F16X1)
    assert not np.isfinite(h).all()                 # (what the fp16 piece makes of the same input)
