"""What the volume post-processing entry points share (metrics.py, data/brats_prepare.py, the two data providers): the stream handle,
argument validation, region sets, the cached workspaces and the error of a refused size - each stated once."""
import torch

from . import _ffi


def stream(device):
    """the caller's current stream on `device` as the integer handle the C ABI takes"""
    return torch.cuda.current_stream(device).cuda_stream


def is_prediction(x):
    return hasattr(x, "labels") and hasattr(x, "mean_label")


def prediction_maps(pred, planar=False):
    """(labels, mean_label) of a Prediction of one volume, checked: labels (S, 1, D, H, W) and mean_label (1, D, H, W), both uint8;
    planar=True also admits a 2-D model's labels (S, B, H, W) and mean_label (B, H, W)"""
    labels, mean_label = pred.labels, pred.mean_label
    if not isinstance(labels, torch.Tensor) or not isinstance(mean_label, torch.Tensor) or labels.dtype != torch.uint8 or mean_label.dtype != torch.uint8:
        raise TypeError("Prediction.labels and Prediction.mean_label must be uint8")
    volume = labels.dim() == 5 and int(labels.shape[1]) == 1
    if not (volume or (planar and labels.dim() == 4)) or tuple(mean_label.shape) != tuple(labels.shape[1:]):
        got = f"got {tuple(labels.shape)} and {tuple(mean_label.shape)}"
        if planar:
            raise ValueError("Prediction expected with labels (S, 1, D, H, W) and mean_label (1, D, H, W), or labels (S, B, H, W) and mean_label (B, H, W), " + got)
        raise ValueError("Prediction of one volume expected: labels (S, 1, D, H, W) and mean_label (1, D, H, W), " + got)
    return labels, mean_label


def prediction_rows(labels, mean_label):
    """rows (N, D, H, W): the samples, then the mean label; a 2-D Prediction's S*B + B maps become volumes of depth 1"""
    if labels.dim() == 5:
        return torch.cat([labels[:, 0], mean_label], 0)
    H, W = int(labels.shape[2]), int(labels.shape[3])
    return torch.cat([labels.reshape(-1, 1, H, W), mean_label.reshape(-1, 1, H, W)], 0)


def label_tensor(t, what, shape, rank=None, also=""):
    """t, a uint8 tensor of `rank` dimensions (None: the caller compares the shape itself); `shape` is the text of the messages"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise TypeError(f"{what} must be {also}a uint8 tensor {shape}")
    if rank is not None and t.dim() != rank:
        raise ValueError(f"{what} {tuple(t.shape)} is not {shape}")
    return t


def on_device(t, what):
    if not t.is_cuda:
        raise ValueError(f"{what} must be on the device, not on {t.device}")


def region_sets(regions, what):
    sets = []
    for reg in regions:
        m = 0
        for v in reg:
            v = int(v)
            if not 0 <= v < 32:
                raise ValueError(f"{what}: label value {v} in region {tuple(reg)} - a region is a set of values 0 .. 31")
            m |= 1 << v
        sets.append(m)
    return sets


def region_set_pair(pred_regions, ref_regions):
    """the sets of pred_regions and of ref_regions (None: the same regions, made once), one per region each"""
    if ref_regions is None:
        sets = region_sets(pred_regions, "pred_regions")
        return sets, sets
    if len(ref_regions) != len(pred_regions):
        raise ValueError(f"{len(pred_regions)} regions of pred against {len(ref_regions)} of the reference")
    return region_sets(pred_regions, "pred_regions"), region_sets(ref_regions, "ref_regions")


_workspaces = {}                                    # owner -> (key, uint8 tensor); every call runs on the caller's current stream


def workspace(owner, key, nbytes, device):
    """The workspace of entry point `owner`: kept while `key` (device and sizes) repeats, replaced when it changes - one shape at a
    time, a validation loop works on volumes of one size.  One slot per owner, so alternating entry points keep theirs."""
    slot = _workspaces.get(owner)
    if slot is None or slot[0] != key:
        slot = _workspaces[owner] = None             # both references dropped: the old block goes back before the new one is asked for
        slot =_workspaces[owner] = (key, torch.empty(nbytes, dtype=torch.uint8, device=device))
    return slot[1]


def refused(what, detail):
    """the error of a size query that returned 0"""
    return _ffi.UzError(f"{what}: sizes refused ({detail})")
