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


def test_support_mirrors_with_one_piece():
    from uda_amd import plan
    # the deferred-input mode at the heads' widths (D0 64, D2 112): the A region is widened to hold the epilogue staging
    for c in (64, 112):
        for cout in (c, 36, 63, 72):
            assert plan.sep_tin_supported(c, cout, "f16") == plan.sep_tin_supported(c, cout, "f16x2"), (c, cout)
    assert plan.sepf_supported(64, 64, "f16") and plan.sepf_supported(112, 112, "f16")


def _fake_library(monkeypatch, seen):
    """capi.load() -> a stand-in whose uda_create records the environment and the model struct it is handed (a real handle
    needs a GPU) and leaves the handle NULL."""
    from uda_amd import capi

    class Lib:
        def uda_create(self, model, *rest):
            seen.append((os.environ.get("UDA_PW_SCHEME"), os.environ.get("UDA_PW_TERMS"), model._obj.pw_scheme))
            return 0
    monkeypatch.setattr(capi, "load", lambda: Lib())


def test_driver_accepts_f16(monkeypatch):
    """`uda_pw_scheme = "f16"` reaches the handle's creation in the model struct (code 5), not through the environment, which
    is untouched while the handle is created; the driver's and the plan's scheme say f16; an unknown value is refused."""
    from uda_amd.infer_lib import KerasDriver
    seen = []
    _fake_library(monkeypatch, seen)
    monkeypatch.delenv("UDA_PW_SCHEME", raising=False)
    monkeypatch.delenv("UDA_PW_TERMS", raising=False)
    p = make_params(**FULL_MC)
    w = make_weights(p)
    d = KerasDriver("_", False, p["name"], 1, False, dict(p, uda_pw_scheme="f16"), weights=w)
    assert seen == [(None, None, 5)]
    assert d.pw_scheme == "f16" and d.plan.pw_scheme == "f16" and d.plan.to_c()[0].pw_scheme == 5
    assert "UDA_PW_SCHEME" not in os.environ and "UDA_PW_TERMS" not in os.environ
    with pytest.raises(ValueError, match="uda_pw_scheme"):
        KerasDriver("_", False, p["name"], 1, False, dict(p, uda_pw_scheme="f8"), weights=w)
    assert len(seen) == 1           # (refused before anything was created)


def test_params_win_over_the_environment(monkeypatch):
    """UDA_PW_SCHEME is the default only: a handle whose params name a scheme plans with that one, whatever the environment says."""
    from uda_amd import plan
    from uda_amd.infer_lib import KerasDriver
    seen = []
    _fake_library(monkeypatch, seen)
    monkeypatch.delenv("UDA_PW_TERMS", raising=False)
    monkeypatch.setenv("UDA_PW_SCHEME", "bf16x3")
    p = make_params(**FULL_MC)
    w = make_weights(p)
    assert _plan(dict(p, uda_pw_scheme="f16"), w).pw_scheme == "f16"
    assert _plan(p, w).pw_scheme == "bf16x3" and _plan(p, w).to_c()[0].pw_scheme == 3
    a = KerasDriver("_", False, p["name"], 1, False, dict(p, uda_pw_scheme="f16"), weights=w)
    b = KerasDriver("_", False, p["name"], 1, False, p, weights=w)
    assert (a.pw_scheme, b.pw_scheme) == ("f16", "bf16x3")
    assert seen == [("bf16x3", None, 5), ("bf16x3", None, 3)]
    assert {s: plan.PW_SCHEME_CODES[s] for s in plan.PW_SCHEMES} == {"f32": 0, "bf16x2": 2, "bf16x3": 3, "f16x2": 4, "f16": 5}


def _plan_state(pl):
    bufs = [(b.H, b.W, b.C, b.per_sample, b.kind, b.level, b.offset, b.name, b.storage) for b in pl.bufs]
    return bufs, pl.ops, pl.sites, pl.arena_floats


@pytest.mark.parametrize("mc", ["full", "head"])
def test_plans_of_two_schemes_do_not_disturb_each_other(monkeypatch, mc):
    """Two Plans with different schemes built alternately in one process equal the plans built alone: nothing a Plan decides
    depends on what another one was given (f32 against f16: unfused against fused with fp16 storage, the widest difference)."""
    monkeypatch.delenv("UDA_PW_SCHEME", raising=False)
    monkeypatch.delenv("UDA_PW_TERMS", raising=False)
    p = make_params(**(FULL_MC if mc == "full" else HEAD_MC))
    w = make_weights(p, seed=1)
    alone = {s: _plan_state(_plan(dict(p, uda_pw_scheme=s), w)) for s in ("f32", "f16", "bf16x3")}
    assert alone["f32"] != alone["f16"]
    for s in ("f16", "f32", "bf16x3", "f32", "f16", "bf16x3"):
        assert _plan_state(_plan(dict(p, uda_pw_scheme=s), w)) == alone[s], s
    assert _plan_state(_plan(p, w)) == _plan_state(_plan(dict(p, uda_pw_scheme="f16x2"), w))      # the default, either way


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
