"""The C-ABI library loads on a machine without a GPU, exports every function that
include/uda_hip.h declares, and the ctypes structures have the C layout.  No compute calls."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from common import ROOT
from uda_amd import capi

HEADER = os.path.join(ROOT, "include", "uda_hip.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(uda_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib_path():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.LIB_PATH


def test_header_and_binding_agree():
    declared = _declared_functions()
    assert declared, "no functions parsed from the header"
    assert sorted(capi.EXPORTS) == declared


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for name in _declared_functions():
        assert hasattr(lib, name), "libuda_hip.so lacks %s" % name


def test_struct_layouts_match_c(tmp_path):
    csrc = tmp_path / "sz.c"
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uda_hip.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(uda_buf_desc_t), sizeof(uda_op_t),'
                    'sizeof(uda_drop_site_t), sizeof(uda_model_t), offsetof(uda_op_t, w_off), offsetof(uda_op_t, fuse_w),'
                    'offsetof(uda_model_t, arena_floats), offsetof(uda_model_t, nms_soft_sigma), offsetof(uda_model_t, pw_scheme));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(capi.BufDesc), ctypes.sizeof(capi.Op), ctypes.sizeof(capi.DropSite),
            ctypes.sizeof(capi.Model), capi.Op.w_off.offset, capi.Op.fuse_w.offset,
            capi.Model.arena_floats.offset, capi.Model.nms_soft_sigma.offset, capi.Model.pw_scheme.offset]
    assert got[6:8] == [176, 140]       # the fields of ABI 4 keep their places: pw_scheme is appended
    assert got == want


def test_create_fails_loudly_without_gpu(lib_path):
    """No CPU fallback: without a HIP device uda_create must return an error, not a handle."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import ctypes as C\n"
            "from uda_amd import capi\n"
            "lib = capi.load()\n"
            "m = capi.Model(); m.abi_version = capi.UDA_ABI_VERSION; m.num_levels = 1; m.chunk_images = 1\n"
            "m.max_images = 1; m.mc_samples = 1\n"
            "import numpy as np\n"
            "w = np.zeros(4, np.float32); h = C.c_void_p()\n"
            "rc = lib.uda_create(C.byref(m), (capi.BufDesc * 1)(), 1, (capi.Op * 1)(), 0, (capi.DropSite * 1)(),\n"
            "                    w.ctypes.data, 4, w.ctypes.data, 0, C.byref(h))\n"
            "print('rc', rc, 'handle', h.value, lib.uda_last_error(None).decode())\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "rc 1" in out.stdout and "handle None" in out.stdout, out.stdout


def test_host_array_entry_points_fail_loudly_without_gpu(lib_path):
    """Every entry point that works on scratch device memory of its own returns 1 without a HIP device, and the error text
    names the entry point and carries HIP's own words (small valid arguments: the failure is the missing device)."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import ctypes as C\n"
            "import numpy as np\n"
            "from uda_amd import capi\n"
            "lib = capi.load()\n"
            "n, M, G, N, NC = 1, 4, 2, 4, 3\n"
            "p = lambda a: a.ctypes.data\n"
            "f32 = lambda *s: np.ones(s, np.float32)\n"
            "f64 = lambda *s: np.ones(s, np.float64)\n"
            "i32 = lambda *s: np.zeros(s, np.int32)\n"
            "desc = capi.ScoreDesc(); desc.n_comp = 1; desc.reduce_mean = 1; desc.n_terms[0] = 1\n"
            "desc.term[0][0].source = capi.SCORE_DET_SCORE; desc.term[0][0].transform = capi.SCORE_SCALAR\n"
            "desc.term[0][0].weight = 1.0\n"
            "comp, cnt, ccnt = f64(n, 1), i32(n), i32(n, NC)\n"
            "thrs = np.array([0.5]); nout = C.c_int32(); ms = C.c_float()\n"
            "calls = {\n"
            "  'uda_assign_gt_np': lambda: lib.uda_assign_gt_np(0, p(f32(n, M, 4)), p(f32(n, G, 4)), p(f32(n, G)), n, M, G,\n"
            "      capi.ASSIGN_IOU, capi.ASSIGN_KEEP_VALIDATE, p(i32(n, G)), p(f64(n, G)), p(i32(n))),\n"
            "  'uda_score_images_np': lambda: lib.uda_score_images_np(0, C.byref(desc), 0.1, p(f64(n, M, 4)), p(f64(n, M)),\n"
            "      p(f64(n, M)), None, None, None, None, n, M, NC, 0, p(comp), p(cnt), p(ccnt)),\n"
            "  'uda_score_images_np_f32': lambda: lib.uda_score_images_np_f32(0, C.byref(desc), 0.1, p(f32(n, M, 4)), p(f32(n, M)),\n"
            "      p(f32(n, M)), None, None, None, None, n, M, NC, 0, p(comp), p(cnt), p(ccnt)),\n"
            "  'uda_eval_match_np': lambda: lib.uda_eval_match_np(0, p(f32(n, M, 7)), p(f32(n, G, 7)), n, M, G, NC, p(thrs), 1,\n"
            "      p(np.zeros(n * M * 44, np.uint8)), p(i32(n, NC, 4)), p(i32(n))),\n"
            "  'uda_thr_objective_np': lambda: lib.uda_thr_objective_np(0, p(f64(1, N)), p(f64(N)), p(np.ones(N, np.uint8)), None,\n"
            "      N, 1, 0, p(thrs), 1, p(f64(1, 1)), 1, 1, 0.95, p(f64(1, 1)), p(f64(1, 1)), p(f64(1, 1))),\n"
            "  'uda_nms_np': lambda: lib.uda_nms_np(0, p(f64(3, 5)), 3, 0, 0.5, 0.5, 0.001, p(f64(3, 5)), C.byref(nout)),\n"
            "  'uda_per_class_nms_np': lambda: lib.uda_per_class_nms_np(0, p(f32(3, 4)), p(f32(3)), p(i32(3)), 3, 0.0, 1.0, NC, 4,\n"
            "      0, 0.5, 0.5, 0.001, p(f32(4, 7))),\n"
            "  'uda_debug_pw': lambda: lib.uda_debug_pw(0, p(f32(1, 4, 4)), p(f32(4, 4)), None, None, None, None, None, None,\n"
            "      1, 1, 4, 4, 4, 0, 0, 0, p(f32(1, 4, 4)), C.byref(ms)),\n"
            "}\n"
            "for name, call in calls.items():\n"
            "    print('%%s|%%d|%%s' %% (name, call(), lib.uda_last_error(None).decode()))\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [line.split("|", 2) for line in out.stdout.splitlines() if line.count("|") >= 2]
    assert [r[0] for r in rows] == ["uda_assign_gt_np", "uda_score_images_np", "uda_score_images_np_f32", "uda_eval_match_np",
                                    "uda_thr_objective_np", "uda_nms_np", "uda_per_class_nms_np", "uda_debug_pw"], out.stdout
    for name, rc, msg in rows:
        assert rc == "1", (name, rc, msg)
        assert msg.startswith(name + ":") and "no ROCm-capable device is detected" in msg, (name, msg)
