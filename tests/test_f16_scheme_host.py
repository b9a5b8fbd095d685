"""CPU tests of the one-piece fp16 scheme (`UDA_PW_SCHEME=f16` / `uda_pw_scheme = "f16"`): the switch, the planner under it and
the shipped code objects of its kernels."""
import os
import subprocess
import sys

import pytest

from common import FULL_MC, HEAD_MC, ROOT, make_params, make_weights


@pytest.fixture
def scheme_env(monkeypatch):
    def set_(v):
        monkeypatch.delenv("UDA_PW_TERMS", raising=False)
        monkeypatch.setenv("UDA_PW_SCHEME", v)
    return set_


def test_pw_scheme_reads_f16(scheme_env):
    from uda_amd import plan
    scheme_env("f16")
    assert plan.pw_scheme() == "f16"
    assert plan.PW_SCHEMES[:4] == ("f16x2", "bf16x3", "bf16x2", "f32")      # appended, the others keep their places
    assert plan.split_pieces("f16") == 1 and plan.split_pieces("f16x2") == 2 and plan.split_pieces("bf16x3") == 3


def _plan(p, w):
    from uda_amd import plan
    return plan.Plan(p, w, chunk_images=2, max_images=2)


@pytest.mark.parametrize("mc", ["full", "head"])
def test_plan_matches_f16x2(scheme_env, mc):
    """One piece frees LDS but changes no lowering decision: the same ops on the same buffers as under f16x2 (in particular
    the deferred head dropout site keeps its deferred-input conv at 64 channels)."""
    p = make_params(**(FULL_MC if mc == "full" else HEAD_MC))
    w = make_weights(p, seed=1)
    plans = {}
    for s in ("f16x2", "f16"):
        scheme_env(s)
        plans[s] = _plan(p, w)
    a, b = plans["f16x2"], plans["f16"]
    assert [(bf.H, bf.W, bf.C, bf.per_sample) for bf in a.bufs] == [(bf.H, bf.W, bf.C, bf.per_sample) for bf in b.bufs]
    assert len(a.ops) == len(b.ops)
    for x, y in zip(a.ops, b.ops):
        assert x == y


@pytest.mark.parametrize("mc", ["full", "head"])
def test_exactly_the_fused_front_halves_outputs_are_fp16(scheme_env, mc):
    """Under f16 the planner marks the output of every fused MBConv front half - and nothing else - as fp16 storage; under f16x2
    nothing is."""
    from uda_amd import capi
    p = make_params(**(FULL_MC if mc == "full" else HEAD_MC))
    w = make_weights(p, seed=1)
    scheme_env("f16")
    pl = _plan(p, w)
    mbx_out = {o["out"] for o in pl.ops if o["kind"] == capi.OP_MBX}
    marked = {i for i, b in enumerate(pl.bufs) if b.storage == "f16"}
    assert mbx_out and marked == mbx_out
    assert all(b.storage in ("f16", "f32") for b in pl.bufs)
    scheme_env("f16x2")
    assert all(b.storage == "f32" for b in _plan(p, w).bufs)


def test_support_mirrors_with_one_piece(scheme_env):
    from uda_amd import plan
    scheme_env("f16")
    # the deferred-input mode at the heads' widths (D0 64, D2 112): the A region is widened to hold the epilogue staging
    for c in (64, 112):
        for cout in (c, 36, 63, 72):
            assert plan.sep_tin_supported(c, cout) == plan.sep_tin_supported(c, cout, "f16x2"), (c, cout)
    assert plan.sepf_supported(64, 64) and plan.sepf_supported(112, 112)


def test_driver_accepts_f16(monkeypatch):
    """The driver's validation of `uda_pw_scheme` accepts "f16" and hands it to the handle's creation (stubbed: the handle
    itself needs a GPU), where the planner reads it; an unknown value is refused."""
    from uda_amd import plan
    from uda_amd.infer_lib import ServingDriver, KerasDriver
    seen = []

    class Created(Exception):
        pass

    def create(self, *a, **k):
        seen.append((self.pw_scheme, plan.pw_scheme()))
        raise Created          # (stop here: what follows needs the handle)
    monkeypatch.setattr(ServingDriver, "_create", create)
    monkeypatch.delenv("UDA_PW_SCHEME", raising=False)
    p = make_params(**FULL_MC)
    w = make_weights(p)
    with pytest.raises(Created):
        KerasDriver("_", False, p["name"], 1, False, dict(p, uda_pw_scheme="f16"), weights=w)
    assert seen == [("f16", "f16")]
    assert "UDA_PW_SCHEME" not in os.environ          # (set for the creation only)
    with pytest.raises(ValueError, match="uda_pw_scheme"):
        KerasDriver("_", False, p["name"], 1, False, dict(p, uda_pw_scheme="f8"), weights=w)


def test_isa_lint_covers_the_one_piece_kernels():
    """The shipped library holds the one-piece instantiations of every split-precision kernel, and the ISA hazard lint of
    tests/test_isa_hazards.py passes on it (it disassembles every kernel of the library)."""
    from uda_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        pytest.skip("libuda_hip.so not built")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "codeobj.py"), "resources", "--lib", capi.LIB_PATH],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = r.stdout
    for k in ("pwb_kernel<1, 1, 4, 1, 5,", "pws_kernel<5, 1, true, false>", "pws_kernel<5, 1, true, true>",
              "w0gate_kernel<5>", "mbxb_kernel<3, 1, 2, true, 5, false>", "mbxb_kernel<3, 1, 2, true, 5, true>",
              "mbxd_kernel<5, 14, 5, 1, false, false>", "mbxd_kernel<5, 14, 5, 1, false, true>", "sep_kernel<2, 5, 2, 1>", "sep_kernel<4, 5, 2, 2>", "sepf_kernel<2, 5, true, 16>"):
        assert k in names, k
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "codeobj.py"), "lint", "--lib", capi.LIB_PATH],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 within 5 wait states" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
