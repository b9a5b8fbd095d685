"""Generates tests/golden/service_edges_golden.npz: what the REAL reference functions return on the edge cases of
tests/service_cases.py - `utils_extra.gt_box_assigner` / `utils_box.calc_iou_np` on every assign case, and
`coco_metric.EvaluationMetric` + `custom_cocoeval.COCOeval_all` on the coco cases up to M = 300.  It reuses the two generators
beside it (their stubs for TensorFlow and pycocotools, their `run_reference`).  Run once where a checkout of the reference
exists; the .npz is committed and is what the tests read.

    python tests/golden/make_service_edges_golden.py <src directory of the reference's checkout>

The file holds OUTPUTS only, and per case a checksum of the inputs (service_cases.checksum): the inputs are regenerated from the
seed, and test_service_cases_host.py fails when they no longer are the ones the reference saw.
  assign  a_<case>_crc; per method and keep rule a_<case>_<method>_<keep>_ok (0: the reference raised, or ran past the
          detections), _idx int32 [n, G], _iou float64 [n, G]
  coco    c_<case>_crc; c_<case>_rec (the standard 10 thresholds packed as the match kernel's records), _npig, _used, _evaluated
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit("usage: make_service_edges_golden.py <src directory of a checkout of the reference>")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np                                   # noqa: E402
import make_gt_assign_golden as GA                   # noqa: E402  (stubs, then the reference's utils_box / utils_extra)
import make_coco_eval_golden as GC                   # noqa: E402  (stubs, then the reference's custom_cocoeval / coco_metric)
import service_cases as SC                           # noqa: E402


def assign_reference(case):
    dets, gtb, gtc = case["dets"], case["gt_boxes"], case["gt_classes"]
    n, G = gtc.shape
    M = dets.shape[1]
    out = {}
    for method in SC.ASSIGN_METHODS:
        for keep in SC.ASSIGN_KEEPS:
            idx = np.full((n, G), -1, np.int32)
            iou = np.zeros((n, G), np.float64)
            ok = 1
            for im in range(n):
                rows = np.where(gtc[im] > 0)[0] if keep == "validate" else [i for i in range(min(G, M)) if gtc[im][i] >= 0]
                for i in rows:
                    try:
                        k = int(GA.utils_extra.gt_box_assigner(method, gtb[im], dets[im], i))
                    except (ValueError, IndexError):  # no detections: calc_iou_np indexes, np.argmin reduces nothing
                        ok = 0
                        continue
                    if k >= M:                       # the reference would index past the detections next
                        ok = 0
                        continue
                    idx[im, i] = k
                    v = GA.utils_box.calc_iou_np([gtb[im][i]], [dets[im][k]])
                    assert v.dtype == np.float64
                    iou[im, i] = v[0]
            tag = "%s_%s" % (method, keep)
            out[tag + "_ok"] = np.array([ok])
            if ok:
                out[tag + "_idx"], out[tag + "_iou"] = idx, iou
    return out


def main():
    out = {}
    for name in SC.ASSIGN_CASES:
        case = SC.assign_case(name)
        out["a_%s_crc" % name] = SC.checksum(case["dets"], case["gt_boxes"], case["gt_classes"])
        out.update({"a_%s_%s" % (name, k): v for k, v in assign_reference(case).items()})
    for name in SC.COCO_GOLDEN_CASES:
        case = SC.coco_case(name)
        n = case["det"].shape[0]
        res, _, _, _ = GC.run_reference(dict(C=case["num_classes"], gt=case["gt"], det=case["det"], batches=[(0, n)]))
        out["c_%s_crc" % name] = SC.checksum(case["det"], case["gt"])
        for k in ("rec_std", "npig_std", "used", "evaluated"):
            out["c_%s_%s" % (name, k.replace("_std", ""))] = res[k]
        print(name, "evaluated rows", int(res["evaluated"].sum()), "of", int(res["used"].sum()))
    dst = os.path.join(HERE, "service_edges_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
