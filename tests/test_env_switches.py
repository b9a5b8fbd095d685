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


# Every switch the library reads.  A new one is written down here, and named by the test that exercises the path it selects.
LIBRARY_SWITCHES = {
    "UDA_NMS_SOLO", "UDA_NMS_PREFIX", "UDA_NMS_REG", "UDA_NMS_COOP", "UDA_NMS_COOP_CAP", "UDA_NMS_COOP_IPT", "UDA_NMS_COOP_SPIN",
    "UDA_NMS_WINNERS", "UDA_NMS_DEBUG", "UDA_AGG_REG", "UDA_TOPK_MULTI", "UDA_PW_SHARED", "UDA_PW_SKINNY", "UDA_STEM_U8",
    "UDA_LANES", "UDA_POST_OVERLAP", "UDA_F16_MIN_RMS", "UDA_SYNC_EACH",
}


def test_no_switch_is_read_on_both_sides():
    lib, pkg = library_switches(), package_switches()
    assert lib == LIBRARY_SWITCHES, sorted(lib ^ LIBRARY_SWITCHES)          # (the scan sees the executor's knobs, and no others)
    assert {"UDA_PW_SCHEME", "UDA_PW_TERMS", "UDA_LIB", "UDA_FUSE_MBX", "UDA_SEP_MULTI"} <= pkg
    assert not lib & pkg, sorted(lib & pkg)
    assert not lib & {"UDA_PW_SCHEME", "UDA_PW_TERMS"}


# A/B switches whose run is decided (DESIGN sections 4-5): fixed at their defaults, the losing side no longer compiled.
RETIRED_AB_SWITCHES = (
    "UDA_PW_BIG", "UDA_PW_MAXNT", "UDA_PW_MAXNT_SMALLK", "UDA_MBX_WAVES", "UDA_MBX_STAMPS", "UDA_MBXP", "UDA_MBX_REMAP",
    "UDA_MBX_SPLIT", "UDA_MBX_SPLIT_MAX", "UDA_MBX_SPLIT_SLABS", "UDA_PWB_CFG", "UDA_PWB_WIDE", "UDA_PWB_DEEP", "UDA_SEPF_PC",
    "UDA_SEPF_GENERIC", "UDA_SEPF_ALL", "UDA_SEP_REMAP", "UDA_SEP_OCC", "UDA_STEM16", "UDA_W0GATE", "UDA_F16_KINDS",
    "UDA_F16_SEP_SHIFT", "UDA_FUSE_MBXD_S2", "UDA_MBXD_MAXKSF", "UDA_DEFER_HEAD",
)


def test_retired_switches_are_gone():
    """UDA_MBXD_WIDE / UDA_MBX_BF16 / UDA_MBXB_S2_TILE chose tile geometry on both sides (buffer sizes here, grids there); the
    decided A/B switches are gone from the package and from csrc/, comments included."""
    retired = ("UDA_MBXD_WIDE", "UDA_MBX_BF16", "UDA_MBXB_S2_TILE")
    for f in glob.glob(os.path.join(PKG, "*.py")) + glob.glob(os.path.join(PKG, "csrc", "*.h*")):
        src = open(f).read()
        assert not [n for n in retired if n in src], f
        # (whole words: UDA_MBXP is a prefix of the build macro UDA_MBXP_STAMPS, which stays)
        assert not [n for n in RETIRED_AB_SWITCHES if re.search(r"\b%s\b" % n, src)], f


def test_the_package_reads_the_planner_switches_in_one_place():
    """plan.py touches the environment in pw_scheme() and Plan.__init__ only; infer_lib.py not at all."""
    assert "os.environ" not in open(os.path.join(PKG, "infer_lib.py")).read()
    src = open(os.path.join(PKG, "plan.py")).read()
    where = set()
    for m in re.finditer(r"os\.environ", src):
        where.add(re.findall(r"^    def (\w+)|^def (\w+)", src[:m.start()], flags=re.M)[-1])
    assert where == {("", "pw_scheme"), ("__init__", "")}, where
