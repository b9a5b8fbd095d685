"""What the planner decided reaches the library in the model description and the op list, and nowhere else: no environment
switch is read on both sides, and the split scheme is not an environment matter of the library at all."""
import glob
import os
import re

from common import ROOT
from uda_amd import plan

PKG = os.path.join(ROOT, "uncertainty-detection-autolabeling_amd")


def _strip_c_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def library_switches():
    """UDA_* names csrc/ reads from the environment: getenv("UDA_...") or the uda_env_int("UDA_...", default) helper."""
    names = set()
    for f in glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")):
        names |= set(re.findall(r'\b(?:getenv|uda_env_int)\(\s*"(UDA_\w+)"', _strip_c_comments(open(f).read())))
    return names


def package_switches():
    """UDA_* names the Python package reads: environ...("UDA_...") and the planner's table, which Plan.__init__ reads by key."""
    names = set(plan.PLAN_SWITCHES)
    for f in glob.glob(os.path.join(PKG, "*.py")):
        names |= set(re.findall(r'environ(?:\.get|\.pop|\.setdefault)?\s*[\[(]\s*"(UDA_\w+)"', open(f).read()))
    return names


def test_no_switch_is_read_on_both_sides():
    lib, pkg = library_switches(), package_switches()
    assert len(lib) > 20 and {"UDA_NMS_COOP", "UDA_LANES", "UDA_SEP_OCC"} <= lib          # (the scan sees the executor's knobs)
    assert {"UDA_PW_SCHEME", "UDA_PW_TERMS", "UDA_LIB", "UDA_FUSE_MBX", "UDA_SEP_MULTI"} <= pkg
    assert not lib & pkg, sorted(lib & pkg)
    assert not lib & {"UDA_PW_SCHEME", "UDA_PW_TERMS"}


def test_retired_switches_are_gone():
    """UDA_MBXD_WIDE / UDA_MBX_BF16 / UDA_MBXB_S2_TILE chose tile geometry on both sides (buffer sizes here, grids there)."""
    retired = ("UDA_MBXD_WIDE", "UDA_MBX_BF16", "UDA_MBXB_S2_TILE")
    for f in glob.glob(os.path.join(PKG, "*.py")) + glob.glob(os.path.join(PKG, "csrc", "*.h*")):
        src = open(f).read()
        assert not [n for n in retired if n in src], f


def test_the_package_reads_the_planner_switches_in_one_place():
    """plan.py touches the environment in pw_scheme() and Plan.__init__ only; infer_lib.py not at all."""
    assert "os.environ" not in open(os.path.join(PKG, "infer_lib.py")).read()
    src = open(os.path.join(PKG, "plan.py")).read()
    where = set()
    for m in re.finditer(r"os\.environ", src):
        where.add(re.findall(r"^    def (\w+)|^def (\w+)", src[:m.start()], flags=re.M)[-1])
    assert where == {("", "pw_scheme"), ("__init__", "")}, where
