// calc_iou_np of the reference (utils_box.py:56-89) for the services that compare their IoUs with it bit for bit - the label
// check (kernels_glc.hip) and the pseudo-label audit (kernels_audit.hip).  Both files are built without FMA contraction.
#pragma once
#include <hip/hip_runtime.h>

namespace uda {

// calc_iou_np (utils_box.py:56-89) on float32 boxes: float32 coordinate differences, float64 products, union = (areaA + areaB)
// - inter, 0 where the union is 0 - the arithmetic of iou_np in kernels_post.hip
__device__ __forceinline__ double glc_iou(const float* a, const float* b) {
  const float yA = fmaxf(a[0], b[0]), xA = fmaxf(a[1], b[1]);
  const float yB = fminf(a[2], b[2]), xB = fminf(a[3], b[3]);
  const double inter = (double)fmaxf(0.0f, xB - xA) * (double)fmaxf(0.0f, yB - yA);
  const double areaA = (double)fabsf(a[3] - a[1]) * (double)fabsf(a[2] - a[0]);
  const double areaB = (double)fabsf(b[3] - b[1]) * (double)fabsf(b[2] - b[0]);
  const double uni = (areaA + areaB) - inter;
  return uni != 0.0 ? inter / uni : 0.0;
}
// the same on float64 boxes (the literals read back from a prediction_data.txt or a label file): everything float64
__device__ __forceinline__ double glc_iou(const double* a, const double* b) {
  const double yA = fmax(a[0], b[0]), xA = fmax(a[1], b[1]);
  const double yB = fmin(a[2], b[2]), xB = fmin(a[3], b[3]);
  const double inter = fmax(0.0, xB - xA) * fmax(0.0, yB - yA);
  const double areaA = fabs(a[3] - a[1]) * fabs(a[2] - a[0]);
  const double areaB = fabs(b[3] - b[1]) * fabs(b[2] - b[0]);
  const double uni = (areaA + areaB) - inter;
  return uni != 0.0 ? inter / uni : 0.0;
}

}  // namespace uda
