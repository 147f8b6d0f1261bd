"""Validation metrics of the reference harness, computed on the device.

Same call signatures as the reference helpers (``utils.generalised_energy_distance`` utils.py:148-200,
``utils.variance_ncc_dist`` utils.py:202-247, the per-label Dice of ``UNetModel.validate``
train_model.py:212-224); the pixel loops run in libuz_hip.so (integer pair counts, cross-entropy maps,
correlations), only the O(N*M) scalar bookkeeping stays on the host.
"""
import collections
import ctypes as C

import torch

from . import _ffi


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def pair_counts(a, b, label):
    """a (Na,H,W), b (Nb,H,W) integer label maps on the GPU -> int32 (Na, Nb, 3): intersection, |a|, |b| for `label`."""
    a8 = a.reshape(a.shape[0], -1).to(torch.uint8).contiguous()
    b8 = b.reshape(b.shape[0], -1).to(torch.uint8).contiguous()
    out = torch.empty(a8.shape[0], b8.shape[0], 3, dtype=torch.int32, device=a.device)
    _ffi.check(_ffi.lib().uz_label_pair_counts(a8.data_ptr(), a8.shape[0], b8.data_ptr(), b8.shape[0], a8.shape[1], int(label),
                                               out.data_ptr(), _stream(a)), "label_pair_counts")
    return out


def _iou_dist_sum(a, b, label_range, nlabels):
    """sum over all pairs of 1 - mean_label IoU, with the reference's empty-mask conventions."""
    tot = None
    for lbl in label_range:
        c = pair_counts(a, b, lbl).cpu().double()
        inter, ca, cb = c[..., 0], c[..., 1], c[..., 2]
        union = ca + cb - inter
        iou = torch.where((ca == 0) & (cb == 0), torch.ones_like(inter),
                          torch.where((ca == 0) | (cb == 0), torch.zeros_like(inter), inter / union.clamp(min=1)))
        tot = iou if tot is None else tot + iou
    return float((1 - tot / nlabels).sum())


def generalised_energy_distance(sample_arr, gt_arr, nlabels=1, **kwargs):
    label_range = kwargs.get("label_range", range(nlabels))
    N, M = sample_arr.shape[0], gt_arr.shape[0]
    d_sy = _iou_dist_sum(sample_arr, gt_arr, label_range, nlabels)
    d_ss = _iou_dist_sum(sample_arr, sample_arr, label_range, nlabels)
    d_yy = _iou_dist_sum(gt_arr, gt_arr, label_range, nlabels)
    return (2. / (N * M)) * d_sy - (1. / N ** 2) * d_ss - (1. / M ** 2) * d_yy


def variance_ncc_dist(sample_arr, gt_arr):
    """sample_arr (N,K,H,W) softmax samples, gt_arr (M,K,H,W) one-hot (any dtype); returns the mean NCC."""
    N, K, H, W = sample_arr.shape
    M = gt_arr.shape[0]
    s = sample_arr.float().contiguous()
    g = gt_arr.float().contiguous()
    ess = torch.empty(H * W, device=s.device)
    esy = torch.empty(M, H * W, device=s.device)
    out = torch.empty(M, device=s.device)
    L = _ffi.lib()
    _ffi.check(L.uz_ncc_maps(s.data_ptr(), g.data_ptr(), N, M, K, H * W, ess.data_ptr(), esy.data_ptr(), _stream(s)), "ncc_maps")
    _ffi.check(L.uz_ncc(ess.data_ptr(), esy.data_ptr(), M, H * W, out.data_ptr(), _stream(s)), "ncc")
    return float(out.double().mean())


def per_label_dice(pred, gt, n_classes):
    out = []
    for lbl in range(n_classes):
        c = pair_counts(pred.reshape(1, *pred.shape[-2:]), gt.reshape(1, *gt.shape[-2:]), lbl).cpu()[0, 0]
        inter, ca, cb = int(c[0]), int(c[1]), int(c[2])
        if ca == 0 and cb == 0:
            out.append(1.0)
        elif ca == 0 or cb == 0:
            out.append(0.0)
        else:
            out.append(2.0 * inter / float(ca + cb))
    return out


# --------------------------------------------------------------------------- S samples of B images against A annotators, one call
Scores = collections.namedtuple("Scores", "ged dice ncc ncc_pairs counts packed")
Scores.__doc__ = """What score_prediction returns, all on the device: ged (B) fp64, dice (B, A, K) fp64 - the mean label of image b against
EVERY annotator, the caller picks its own -, ncc (B) fp64 and ncc_pairs (B, A) fp32 (both None when the Prediction carries no `soft`),
counts (B, K, S*A + S*S + A*A, 3) int32 or None: per image and label the pair-count matrices samples x annotators, samples x samples,
annotators x annotators, flattened one behind the other, each in pair_counts' layout.  ged, ncc and dice are views of `packed`, one
fp64 buffer [ged (B) | ncc (B) | dice (B*A*K)], so that a caller copies them to the host in one transfer."""


def score_prediction(pred, annotations, return_counts=False):
    """GED, NCC and per-label Dice of a Prediction (models/phiseg.py: S samples of B images, or PHISeg3D's S samples of one volume)
    against `annotations` (B, A, ...), an integer tensor of annotator label maps on the device - for all B images in ONE
    uz_score_samples call (csrc/score.hip): one workspace allocation, no host synchronisation, no ATen arithmetic on the maps
    (annotations that are not uint8 already are converted once).  Per image the values are those of generalised_energy_distance
    (labels 1 .. K-1), variance_ncc_dist and per_label_dice above on pred.labels[:, b], pred.soft[:, b] and pred.mean_label[b];
    K is the class dimension of pred.mean_soft.  Returns a Scores of device tensors."""
    labels, mean_label, soft = pred.labels, pred.mean_label, pred.soft
    S, B = int(labels.shape[0]), int(labels.shape[1])
    K = int(pred.mean_soft.shape[1])
    P = 1
    for d in labels.shape[2:]:
        P *= int(d)
    if annotations.dim() < 3 or int(annotations.shape[0]) != B or tuple(annotations.shape[2:]) != tuple(labels.shape[2:]):
        raise ValueError(f"annotations {tuple(annotations.shape)} do not match (B, A) + {tuple(labels.shape[2:])} with B = {B}")
    if annotations.device != labels.device:
        raise ValueError("annotations must be on the device of the Prediction")
    A = int(annotations.shape[1])
    ann = annotations if annotations.dtype == torch.uint8 else annotations.to(torch.uint8)
    ann, labels, mean_label = ann.contiguous(), labels.contiguous(), mean_label.contiguous()
    if labels.dtype != torch.uint8 or mean_label.dtype != torch.uint8:
        raise TypeError("Prediction.labels and Prediction.mean_label must be uint8")
    if soft is not None:
        if soft.dtype != torch.float32 or tuple(soft.shape) != (S, B, K) + tuple(labels.shape[2:]):
            raise ValueError(f"Prediction.soft {tuple(soft.shape)} {soft.dtype} is not fp32 (S, B, K, ...)")
        soft = soft.contiguous()
    L, dev = _ffi.lib(), labels.device
    nbytes = L.uz_score_workspace(B, S, A, K, P)
    if nbytes == 0:
        raise _ffi.UzError(f"score_prediction: sizes refused (B {B} S {S} A {A} K {K} P {P}; 2 <= K <= 8, every element count within int32)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)                # (the caching allocator hands out 512-byte aligned blocks)
    packed = torch.empty(2 * B + B * A * K, dtype=torch.float64, device=dev)
    ged, ncc, dice = packed[:B], packed[B:2 * B], packed[2 * B:].view(B, A, K)
    ncc_pairs = torch.empty(B, A, dtype=torch.float32, device=dev) if soft is not None else None
    counts = torch.empty(B, K, S * A + S * S + A * A, 3, dtype=torch.int32, device=dev) if return_counts else None
    _ffi.check(L.uz_score_samples(labels.data_ptr(), ann.data_ptr(), mean_label.data_ptr(), soft.data_ptr() if soft is not None else None,
                                  B, S, A, K, P, ws.data_ptr(), counts.data_ptr() if return_counts else None, ged.data_ptr(),
                                  ncc_pairs.data_ptr() if soft is not None else None, ncc.data_ptr() if soft is not None else None,
                                  dice.data_ptr(), _stream(labels)), "score_samples")
    return Scores(ged=ged, dice=dice, ncc=ncc if soft is not None else None, ncc_pairs=ncc_pairs, counts=counts, packed=packed)
