"""References of the multi-class (5 to 16 classes) pieces that tests/_fp64_loss_ref.py and tests/_fp64_tail_ref.py do not hold:
the table remap of the label path and the per-class IoU of a confusion matrix.  The loss, classifier and confusion references of
those two modules are generic in the class count (tests/test_multiclass_ref_host.py checks them at 5, 9 and 16 classes against
torch's own float64 operators) and are used as they are."""
import numpy as np
import torch


def remap_table(raw, table):
    """kd_semantic_remap_table: out[i] = table[raw[i]] for 0 <= raw[i] < len(table), else 0.  Tensors in (any device), tensor out."""
    ntab = table.numel()
    ok = (raw >= 0) & (raw < ntab)
    return torch.where(ok, table[raw.clamp(0, ntab - 1)], torch.zeros_like(raw))


def class_iou(conf):
    """SegmentationMetrics.compute on an [M, M] integer matrix (numpy): tp / (tp + fp + fn) per class, 0 where the class is absent"""
    conf = np.asarray(conf, np.int64)
    tp = np.diag(conf).astype(np.float64)
    denom = conf.sum(0) + conf.sum(1) - np.diag(conf)
    return [float(t / d) if d > 0 else 0.0 for t, d in zip(tp, denom)]
