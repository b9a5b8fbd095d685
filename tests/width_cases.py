"""The case table of the BiFPN / head width tests (test_widths_host.py without a device, test_gpu_widths.py on one).

D0's backbone at 192x128 with two BiFPN cells and two head layers; only `fpn_num_filters` (F), the class count, the dropout
configuration and the split scheme vary.  Per case the literals say which lowering the planner chooses - they are checked on
the host, so that a planner change that moves a case off the kernel it is meant to reach fails without a device:

  sepf      OP_SEP ops with `fuse_in` (sepf_kernel: the BiFPN fusion inside the node's separable conv; 8 nodes x 2 cells)
  sep       OP_SEP ops without it (sep_kernel: 2 heads x (2 layers + predict) x 5 levels)
  tin       of those, ops with `drop_site2 >= 0` (sep_kernel's deferred-input mode: first head layer defers, its reader takes)
  fuse, dw  OP_FUSE / OP_DW ops of the unfused lowering (widths above 128, and widths that are no multiple of 8)
  named     oracle taps the plan names, of the `taps` the oracle records; all but the by-design exceptions are compared
"""
import collections

from common import FULL_MC, HEAD_MC, LOSS_ATT

SIZE = "192x128"
N_IMAGES, RAW, SEED = 3, (100, 180), 91
COMMON = dict(image_size=SIZE, model="efficientdet-d0", fpn_cell_repeats=2, box_class_repeats=2)
DROPOUT = {"full_mc": FULL_MC, "head_mc": HEAD_MC, "loss_att": LOSS_ATT}
SCHEMES = ("f16x2", "bf16x3", "bf16x2", "f16")      # ("bf16", one bf16 piece, has no per-tap bar: out of scope; "f32" never fuses)

Case = collections.namedtuple("Case", "F classes dropout scheme sepf sep tin fuse dw named taps")

CASES = {
    #                    F  classes  dropout    scheme   sepf sep tin fuse dw named taps
    "w16":         Case(16,   4, "full_mc",  None,      16, 30,  0,  0,  0, 66, 98),
    "w24":         Case(24,   7, "full_mc",  None,      16, 30,  0,  0,  0, 66, 98),
    "w88":         Case(88,  13, "head_mc",  None,      16, 30, 10,  0,  0, 66, 98),
    "w88_f16":     Case(88,   7, "full_mc",  "f16",     16, 30,  0,  0,  0, 66, 98),
    "w88_bf16x3":  Case(88,   7, "full_mc",  "bf16x3",  16, 30,  0,  0,  0, 66, 98),
    "w120":        Case(120, 15, "head_mc",  None,      16, 30,  0,  0,  0, 66, 98),
    "w128":        Case(128, 90, "head_mc",  None,      16, 30,  0,  0,  0, 66, 98),
    "w128_bf16x3": Case(128, 12, "loss_att", "bf16x3",  16, 30,  0,  0,  0, 66, 98),
    "w128_f16":    Case(128, 13, "head_mc",  "f16",     16, 30, 10,  0,  0, 66, 98),
    "w136":        Case(136,  7, "full_mc",  None,       0,  0,  0, 16, 46, 82, 98),
    "w160":        Case(160, 90, "head_mc",  None,       0,  0,  0, 16, 46, 82, 98),
    "w384":        Case(384,  7, "loss_att", None,       0,  0,  0, 16, 46, 82, 98),
    "w20":         Case(20,   7, "full_mc",  None,       0,  0,  0, 16, 46, 82, 98),
}
WIDTHS = sorted({c.F for c in CASES.values()})


def params_of(case):
    """model_params of one case (no `uda_keep_buffers`: the GPU test adds it)"""
    from common import make_params
    c = CASES[case]
    p = make_params(num_classes=c.classes, fpn_num_filters=c.F, **dict(COMMON, **DROPOUT[c.dropout]))
    if c.scheme:
        p["uda_pw_scheme"] = c.scheme
    return p


def path_counts(plan):
    """(sepf, sep, tin, fuse, dw) of a plan: the BiFPN / head part of its op list (the backbone's depthwise ops are not counted)"""
    from uda_amd import capi
    names = {i: n for n, i in plan.buffer_names.items()}
    sep = [o for o in plan.ops if o["kind"] == capi.OP_SEP]
    dw = [o for o in plan.ops if o["kind"] == capi.OP_DW and not names.get(o["out"], "").startswith("blocks_")]
    return (sum(bool(o["fuse_in"]) for o in sep), sum(not o["fuse_in"] for o in sep), sum(o["drop_site2"] >= 0 for o in sep),
            sum(o["kind"] == capi.OP_FUSE for o in plan.ops), len(dw))
