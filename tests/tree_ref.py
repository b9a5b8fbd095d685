"""The one numpy statement of the float64 zero-padded pairwise tree sum that the contracts of uda_uncert_report_np,
uda_class_report_np, uda_thr_report_np and uda_thr_post_np (include/uda_hip.h) promise bit for bit.  The mirrors of those
contracts take it from here under their own names; on the device it is stated in csrc/wave_fold.h."""
import numpy as np


def tree(terms):
    """Root of the perfect binary tree over `terms`, zero-padded to a power of two; 0.0 for no terms."""
    b = np.asarray(terms, np.float64).ravel()
    if len(b) == 0:
        return np.float64(0.0)
    size = 1
    while size < len(b):
        size *= 2
    b = np.concatenate([b, np.zeros(size - len(b))])
    while len(b) > 1:
        b = b[0::2] + b[1::2]
    return b[0]
