"""MI355X-native hot path of uncertainty-detection-autolabeling.

Import this package as ``uda_amd`` (see ``uda_amd/__init__.py``).
Modules:
  hparams_config  mirror of the reference's config object for this path
  dataset_data    dataset letter -> label map / raw image shape
  weights         reference-named weight sets (random init per reference initialisers)
  plan            network topology -> flat op list + packed weight blob for the C-ABI
  capi            ctypes binding of include/uda_hip.h (csrc/libuda_hip.so)
  infer_lib       ServingDriver-shaped boundary (serve / predict / benchmark)
  dist            image sharding + detection gather (torch.distributed / RCCL)
  pseudo_labels   the STAC teacher's selection: candidate rows from the device, dataset-wide rule, KITTI / BDD pseudo ground truth
  uncertainty_report  the validation uncertainty report: ECE, NLL, coverage, RMSUE, sharpness of every sigma column from one device call
  class_report    the classification calibration report: reliability bins, ECE, MCE, Brier, NLL, SCE of every probability table from one device call
  thresholding    failure-recognition weights and threshold from validation rows (roc_objective, UncertOptimal, autolabel_verdict)
  epal            the epistemic-vs-aleatoric comparison: grid search, corner detections, metric lists and the Gaussian KDE of all configurations from one device call
  post_thresholding  where the threshold acts: the heat maps, spider metrics and image lists after thresholding (heat_maps, spider_metrics, rank_images)
"""
