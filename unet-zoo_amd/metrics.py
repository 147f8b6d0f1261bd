"""Validation metrics of the reference harness, computed on the device.

Same call signatures as the reference helpers (``utils.generalised_energy_distance`` utils.py:148-200,
``utils.variance_ncc_dist`` utils.py:202-247, the per-label Dice of ``UNetModel.validate``
train_model.py:212-224); the pixel loops run in libuz_hip.so (integer pair counts, cross-entropy maps,
correlations), only the O(N*M) scalar bookkeeping stays on the host.
"""
import collections
import ctypes as C
import math

import torch

from . import _ffi, _vol


def pair_counts(a, b, label):
    """a (Na,H,W), b (Nb,H,W) integer label maps on the GPU -> int32 (Na, Nb, 3): intersection, |a|, |b| for `label`."""
    a8 = a.reshape(a.shape[0], -1).to(torch.uint8).contiguous()
    b8 = b.reshape(b.shape[0], -1).to(torch.uint8).contiguous()
    out = torch.empty(a8.shape[0], b8.shape[0], 3, dtype=torch.int32, device=a.device)
    _ffi.check(_ffi.lib().uz_label_pair_counts(a8.data_ptr(), a8.shape[0], b8.data_ptr(), b8.shape[0], a8.shape[1], int(label),
                                               out.data_ptr(), _vol.stream(a.device)), "label_pair_counts")
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
    _ffi.check(L.uz_ncc_maps(s.data_ptr(), g.data_ptr(), N, M, K, H * W, ess.data_ptr(), esy.data_ptr(), _vol.stream(s.device)), "ncc_maps")
    _ffi.check(L.uz_ncc(ess.data_ptr(), esy.data_ptr(), M, H * W, out.data_ptr(), _vol.stream(s.device)), "ncc")
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
        raise _vol.refused("score_prediction", f"B {B} S {S} A {A} K {K} P {P}; 2 <= K <= 8, every element count within int32")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)                # (the caching allocator hands out 512-byte aligned blocks)
    packed = torch.empty(2 * B + B * A * K, dtype=torch.float64, device=dev)
    ged, ncc, dice = packed[:B], packed[B:2 * B], packed[2 * B:].view(B, A, K)
    ncc_pairs = torch.empty(B, A, dtype=torch.float32, device=dev) if soft is not None else None
    counts = torch.empty(B, K, S * A + S * S + A * A, 3, dtype=torch.int32, device=dev) if return_counts else None
    _ffi.check(L.uz_score_samples(labels.data_ptr(), ann.data_ptr(), mean_label.data_ptr(), soft.data_ptr() if soft is not None else None,
                                  B, S, A, K, P, ws.data_ptr(), counts.data_ptr() if return_counts else None, ged.data_ptr(),
                                  ncc_pairs.data_ptr() if soft is not None else None, ncc.data_ptr() if soft is not None else None,
                                  dice.data_ptr(), _vol.stream(labels.device)), "score_samples")
    return Scores(ged=ged, dice=dice, ncc=ncc if soft is not None else None, ncc_pairs=ncc_pairs, counts=counts, packed=packed)


# --------------------------------------------------------------------------- N label volumes against one reference: the BraTS region scores
BRATS_REGIONS = ((1, 2, 4), (1, 4), (4,))          # raw BraTS labels: whole tumour, tumour core, enhancing tumour (bratsUtils.py:86-93)
BRATS_REGION_NAMES = ("WT", "TC", "ET")
BRATS_LABELS = (0, 1, 2, 4)                         # class index -> raw BraTS label: the lut of data.restore_volume

VolumeScores = collections.namedtuple("VolumeScores", "dice sensitivity specificity hd95 counts")
VolumeScores.__doc__ = """What score_volume returns, all on the device: dice, sensitivity, specificity, hd95 (N, R) fp64 - views of one (N, R, 4)
buffer - and counts (N, R, 4) int64 = {tp, |pred|, |ref|, voxels}.  hd95 is -1 where a mask is empty and NaN when it was not asked for."""


def score_volume(pred, reference, pred_regions, ref_regions=None, hd95=True):
    """Dice, sensitivity, specificity and HD95 (bratsUtils.py:6-24,57-84) of N label volumes against ONE reference volume, for R regions
    given as sequences of label-value tuples (BRATS_REGIONS for raw BraTS labels; ref_regions defaults to pred_regions, give both when the
    prediction's labels are class indices and the reference's raw values) - one uz_vol_region_scores call (csrc/volscore.hip): no host
    round trip, no synchronisation.  pred: a Prediction of PHISeg3D.predict - the rows are its S samples, then mean_label, N = S + 1 - or
    a uint8 tensor (N, D, H, W); reference: uint8 (D, H, W) on the same device, for instance the y_raw of BratsDataset.  Returns a
    VolumeScores of device tensors."""
    if _vol.is_prediction(pred):
        rows = _vol.prediction_rows(*_vol.prediction_maps(pred))
    else:
        rows = _vol.label_tensor(pred, "pred", "(N, D, H, W)", 4, also="a Prediction or ")
    _vol.label_tensor(reference, "reference", "(D, H, W)")
    if tuple(reference.shape) != tuple(rows.shape[1:]):
        raise ValueError(f"reference {tuple(reference.shape)} does not match the volumes {tuple(rows.shape[1:])} of pred")
    if reference.device != rows.device:
        raise ValueError("reference must be on the device of pred")
    psets, rsets = _vol.region_set_pair(pred_regions, ref_regions)
    N, D, H, W = (int(d) for d in rows.shape)
    R = len(psets)
    L, dev = _ffi.lib(), rows.device
    nbytes = L.uz_vol_region_scores_workspace(N, R, D, H, W, int(bool(hd95)))
    if nbytes == 0:
        raise _vol.refused("score_volume", f"N {N} R {R} volume {D} x {H} x {W}; 1 <= R <= 8, D*H*W < 2^31, D^2 + H^2 + W^2 <= 2^22 with hd95")
    rows, reference = rows.contiguous(), reference.contiguous()
    ws = _vol.workspace("score_volume", (dev, N, R, D, H, W, bool(hd95)), nbytes, dev)
    scores = torch.empty(N, R, 4, dtype=torch.float64, device=dev)
    counts = torch.empty(N, R, 4, dtype=torch.int64, device=dev)
    U32 = C.c_uint32 * R
    _ffi.check(L.uz_vol_region_scores(rows.data_ptr(), N, U32(*psets), reference.data_ptr(), U32(*rsets), R, D, H, W, int(bool(hd95)),
                                      ws.data_ptr(), counts.data_ptr(), scores.data_ptr(), _vol.stream(rows.device)), "vol_region_scores")
    return VolumeScores(dice=scores[..., 0], sensitivity=scores[..., 1], specificity=scores[..., 2], hd95=scores[..., 3], counts=counts)


# --------------------------------------------------------------------------- connected components of label volumes: the clean-up between drawing and scoring
def _components_workspace(rows, what):
    N, D, H, W = (int(d) for d in rows.shape)
    L, dev = _ffi.lib(), rows.device
    nbytes = L.uz_vol_components_workspace(N, D, H, W)
    if nbytes == 0:
        raise _vol.refused(what, f"N {N} volume {D} x {H} x {W}; no empty axis, 1 <= N <= 65536, N*D*H*W < 2^31")
    return _vol.workspace("components", (dev, N, D, H, W), nbytes, dev)              # label_components and keep_largest_components share it


def _prediction_rows(pred):
    """(rows (N, D, H, W) uint8, is_prediction): a Prediction's samples, then its mean label, as score_volume concatenates them; a 2-D
    Prediction's (S, B, H, W) and (B, H, W) become S*B + B volumes of depth 1"""
    if not _vol.is_prediction(pred):
        return _vol.label_tensor(pred, "pred", "(N, D, H, W)", 4), False
    return _vol.prediction_rows(*_vol.prediction_maps(pred, planar=True)), True


def _filtered_prediction(pred, out):
    """a new Prediction: labels and mean_label cut out of the filtered rows, every other field the same object"""
    labels, mean_label = pred.labels, pred.mean_label
    n_lab = int(out.shape[0]) - int(mean_label.shape[0])
    fields = {k: getattr(pred, k) for k in type(pred).__slots__} if hasattr(type(pred), "__slots__") else dict(pred._asdict())
    fields["labels"] = out[:n_lab].reshape(labels.shape)
    fields["mean_label"] = out[n_lab:].reshape(mean_label.shape)
    return type(pred)(**fields)


def _connectivity(connectivity):
    if isinstance(connectivity, bool) or not isinstance(connectivity, int):
        raise TypeError(f"connectivity must be the int 1, 2 or 3, not {connectivity!r}")
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity {connectivity}: 1 (faces), 2 (faces and edges) or 3 (faces, edges and corners)")
    return connectivity


def _per_region(value, R, what):
    """None -> None; one int -> R of it; a sequence -> its ints, R of them"""
    if value is None:
        return None
    if isinstance(value, int):
        return [value] * R
    out = [int(v) for v in value]
    if len(out) != R:
        raise ValueError(f"{len(out)} {what} for {R} regions")
    return out


def label_components(volumes, values, return_sizes=False, connectivity=1):
    """Connected components of {label in values} in N label volumes, uint8 (N, D, H, W) on the device - one uz_vol_label_components
    call (connectivity 1, faces: 6 neighbours, 4 when D == 1) or uz_vol_label_components_ex call (connectivity 2: 18, or 3: 26
    neighbours, skimage's full connectivity; 8 when D == 1) (csrc/volcomp.hip) on the caller's current stream, no synchronisation.
    Returns int32 labels (N, D, H, W): 0 on background, 1 + the smallest local index (z*H + y)*W + x of the voxel's component
    elsewhere - canonical, so a repeated call is bit-equal -, or (labels, sizes) with the voxel count of each voxel's component."""
    _connectivity(connectivity)
    rows = _vol.label_tensor(volumes, "volumes", "(N, D, H, W)", 4)
    (bits,) = _vol.region_sets((tuple(values),), "values")
    _vol.on_device(rows, "volumes")
    ws = _components_workspace(rows, "label_components")
    rows = rows.contiguous()
    labels = torch.empty(rows.shape, dtype=torch.int32, device=rows.device)
    sizes = torch.empty(rows.shape, dtype=torch.int32, device=rows.device) if return_sizes else None
    N, D, H, W = (int(d) for d in rows.shape)
    tail = (labels.data_ptr(), sizes.data_ptr() if return_sizes else None, ws.data_ptr(), _vol.stream(rows.device))
    if connectivity == 1:
        _ffi.check(_ffi.lib().uz_vol_label_components(rows.data_ptr(), N, D, H, W, bits, *tail), "vol_label_components")
    else:
        _ffi.check(_ffi.lib().uz_vol_label_components_ex(rows.data_ptr(), N, D, H, W, bits, connectivity, *tail), "vol_label_components_ex")
    return (labels, sizes) if return_sizes else labels


def keep_largest_components(pred, regions=((1,), (2,), (3,)), min_voxels=None, unlisted="zero", connectivity=1, relabel=None):
    """keep_largest_connected_components (data/BratsProcessing/utils.py:228-251) on the device - one uz_vol_keep_components call
    (csrc/volcomp.hip) on the caller's current stream, no host round trip, no synchronisation.  Each region, a tuple of label values,
    is labelled on its own (the regions may be nested: ((1, 2, 3),) keeps the largest whole tumour); of a region with min_voxels 0 the
    largest component per volume is kept (ties: the one whose first voxel comes first), with min_voxels m >= 1 every component of at
    least m voxels.  A voxel keeps its label when every region that contains the label keeps the voxel's component, else it becomes
    0; labels in no region become 0 (unlisted="zero", the reference) or stay (unlisted="keep").  min_voxels: None (all 0), one int,
    or one int per region.  The default regions with the other defaults are the reference function.
    pred: a uint8 tensor (N, D, H, W) -> the filtered tensor; or a Prediction - PHISeg3D's, labels (S, 1, D, H, W) and mean_label
    (1, D, H, W), or a 2-D model's, labels (S, B, H, W) and mean_label (B, H, W), run as D = 1 - whose samples and mean label go through
    ONE call -> a new Prediction with the filtered labels and mean_label.  Every other field is the same object: soft, mean_soft and
    entropy describe the UNFILTERED draw.  The result goes into score_volume as it is.
    connectivity: 1, 2 or 3 - 6, 18 or 26 neighbours (skimage's `connectivity`).  relabel: None, or one entry per region, each None
    (a removed voxel becomes 0) or an int 0 .. 255 that a voxel removed by that region becomes; the regions run in order, all on the
    unfiltered input, and the last region that removes a voxel decides.  The BraTS rule "a small enhancing component is necrosis":
    keep_largest_components(pred, regions=((3,),), min_voxels=500, relabel=(1,), unlisted="keep").  With connectivity 1 and relabel
    None the call is uz_vol_keep_components, else uz_vol_keep_components_ex."""
    if unlisted not in ("zero", "keep"):
        raise ValueError(f"unlisted must be 'zero' or 'keep', not {unlisted!r}")
    sets = _vol.region_sets(regions, "regions")
    R = len(sets)
    if min_voxels is None:
        mv = [0] * R
    elif isinstance(min_voxels, int):
        mv = [min_voxels] * R
    else:
        mv = [int(m) for m in min_voxels]
        if len(mv) != R:
            raise ValueError(f"{len(mv)} min_voxels for {R} regions")
    if any(m < 0 for m in mv):
        raise ValueError(f"min_voxels {tuple(mv)}: a threshold is a voxel count >= 0")
    _connectivity(connectivity)
    rl = None
    if relabel is not None:
        rl = list(relabel)
        if len(rl) != R:
            raise ValueError(f"{len(rl)} relabel entries for {R} regions")
        for v in rl:
            if v is not None and (isinstance(v, bool) or not isinstance(v, int)):
                raise TypeError(f"relabel {tuple(rl)}: an entry is None or an int")
            if v is not None and not 0 <= v <= 255:
                raise ValueError(f"relabel {tuple(rl)}: a label value is 0 .. 255")
        rl = [-1 if v is None else v for v in rl]
    rows, is_pred = _prediction_rows(pred)
    if R < 1 or R > 8:
        raise _vol.refused("keep_largest_components", f"{R} regions; 1 <= R <= 8")
    _vol.on_device(rows, "pred")
    ws = _components_workspace(rows, "keep_largest_components")
    rows = rows.contiguous()
    out = torch.empty_like(rows)
    N, D, H, W = (int(d) for d in rows.shape)
    tail = (int(unlisted == "keep"), out.data_ptr(), ws.data_ptr(), _vol.stream(rows.device))
    if connectivity == 1 and rl is None:
        _ffi.check(_ffi.lib().uz_vol_keep_components(rows.data_ptr(), N, D, H, W, (C.c_uint32 * R)(*sets), (C.c_int32 * R)(*mv), R, *tail), "vol_keep_components")
    else:
        _ffi.check(_ffi.lib().uz_vol_keep_components_ex(rows.data_ptr(), N, D, H, W, (C.c_uint32 * R)(*sets), (C.c_int32 * R)(*mv),
                                                        (C.c_int32 * R)(*(rl or [-1] * R)), R, connectivity, *tail), "vol_keep_components_ex")
    if not is_pred:
        return out
    return _filtered_prediction(pred, out)


def fill_holes(pred, regions=((1, 2, 3),), fill=None, max_voxels=None, connectivity=1):
    """scipy.ndimage.binary_fill_holes per region on the device - one uz_vol_fill_holes call (csrc/volcomp.hip) on the caller's current
    stream, no host round trip, no synchronisation.  A hole of a region, a tuple of label values, is a connected component of the
    voxels whose label is NOT in the region that touches no face of the volume (of a 2-D map: no edge of the image); its voxels
    become `fill` - None: the region's first value, or one int per region, a member of its region.  max_voxels: None or 0 (holes of
    any size), one int, or one int per region: only holes of at most that many voxels are filled.  connectivity: 1, 2 or 3, the
    BACKGROUND's, as binary_fill_holes' `structure` is (default 1: a cavity that a diagonal gap opens stays a hole).  Every region
    sees the input; a later region overwrites an earlier one, so list nested regions from outer to inner.
    pred: what keep_largest_components takes, and the same kind of thing comes back: a uint8 tensor (N, D, H, W), or a Prediction,
    whose samples and mean label go through ONE call -> a new Prediction with the filled labels and mean_label."""
    sets = _vol.region_sets(regions, "regions")
    R = len(sets)
    if fill is None:
        if any(len(tuple(reg)) == 0 for reg in regions):
            raise ValueError("fill_holes: an empty region has no value to fill with")
        fv = [int(tuple(reg)[0]) for reg in regions]
    else:
        fv = _per_region(fill, R, "fill values")
        for v, reg in zip(fv, regions):
            if v not in tuple(int(x) for x in reg):
                raise ValueError(f"fill value {v} is no member of its region {tuple(reg)}")
    mx = _per_region(max_voxels, R, "max_voxels") or [0] * R
    if any(m < 0 for m in mx):
        raise ValueError(f"max_voxels {tuple(mx)}: a limit is a voxel count >= 0")
    _connectivity(connectivity)
    rows, is_pred = _prediction_rows(pred)
    if R < 1 or R > 8:
        raise _vol.refused("fill_holes", f"{R} regions; 1 <= R <= 8")
    _vol.on_device(rows, "pred")
    N, D, H, W = (int(d) for d in rows.shape)
    nbytes = _ffi.lib().uz_vol_components_workspace(N, D, H, W)
    if nbytes == 0:
        raise _vol.refused("fill_holes", f"N {N} volume {D} x {H} x {W}; no empty axis, 1 <= N <= 65536, N*D*H*W < 2^31")
    ws = _vol.workspace("fill_holes", (rows.device, N, D, H, W), nbytes, rows.device)   # its own slot: a loop alternates it with the keep call
    rows = rows.contiguous()
    out = torch.empty_like(rows)
    _ffi.check(_ffi.lib().uz_vol_fill_holes(rows.data_ptr(), N, D, H, W, (C.c_uint32 * R)(*sets), (C.c_int32 * R)(*fv), (C.c_int32 * R)(*mx), R, connectivity,
                                            out.data_ptr(), ws.data_ptr(), _vol.stream(rows.device)), "vol_fill_holes")
    if not is_pred:
        return out
    return _filtered_prediction(pred, out)


# --------------------------------------------------------------------------- binary morphology and lesion-wise scores (the BraTS rankings since 2023)
def _morph(what, volumes, values, iterations, connectivity, erode):
    _connectivity(connectivity)
    if isinstance(iterations, bool) or not isinstance(iterations, int):
        raise TypeError(f"iterations must be an int >= 0, not {iterations!r}")
    if iterations < 0:
        raise ValueError(f"iterations {iterations}: a number of passes >= 0")
    rows = _vol.label_tensor(volumes, "volumes", "(N, D, H, W)", 4)
    (bits,) = _vol.region_sets((tuple(values),), "values")
    _vol.on_device(rows, "volumes")
    N, D, H, W = (int(d) for d in rows.shape)
    L, dev = _ffi.lib(), rows.device
    nbytes = L.uz_vol_morph_workspace(N, D, H, W)
    if nbytes == 0:
        raise _vol.refused(what, f"N {N} volume {D} x {H} x {W}; no empty axis, 1 <= N <= 65536, N*D*H*W < 2^31")
    ws = _vol.workspace("morph", (dev, N, D, H, W), nbytes, dev)
    rows = rows.contiguous()
    out = torch.empty_like(rows)
    _ffi.check(L.uz_vol_morph(rows.data_ptr(), N, D, H, W, bits, connectivity, iterations, erode, out.data_ptr(), ws.data_ptr(), _vol.stream(dev)), "vol_morph")
    return out


def binary_dilation(volumes, values, iterations=1, connectivity=1):
    """scipy.ndimage.binary_dilation of {label in values} in N label volumes, uint8 (N, D, H, W) on the device, with
    structure = generate_binary_structure(3, connectivity) - 6, 18 or 26 neighbours; the 2-D structure when D == 1 -, `iterations`
    passes and border_value = 0: one uz_vol_morph call (csrc/volmorph.hip) on the caller's current stream, no synchronisation.
    `volumes`, `values` and `connectivity` are what label_components takes.  Returns a uint8 tensor (N, D, H, W) of 0 / 1;
    iterations = 0 gives the membership mask itself.  Volumes never touch each other."""
    return _morph("binary_dilation", volumes, values, iterations, connectivity, 0)


def binary_erosion(volumes, values, iterations=1, connectivity=1):
    """scipy.ndimage.binary_erosion, as binary_dilation: a voxel outside the volume reads as 0, so an erosion eats inward from the
    faces (border_value = 0, scipy's default)."""
    return _morph("binary_erosion", volumes, values, iterations, connectivity, 1)


def binary_opening(volumes, values, iterations=1, connectivity=1):
    """scipy.ndimage.binary_opening: `iterations` erosions, then as many dilations of the result - two uz_vol_morph calls"""
    return _morph("binary_opening", _morph("binary_opening", volumes, values, iterations, connectivity, 1), (1,), iterations, connectivity, 0)


def binary_closing(volumes, values, iterations=1, connectivity=1):
    """scipy.ndimage.binary_closing: `iterations` dilations, then as many erosions of the result - two uz_vol_morph calls.  The border
    reads as 0 in both, as scipy's does: a closing can eat foreground that lies within `iterations` voxels of a face."""
    return _morph("binary_closing", _morph("binary_closing", volumes, values, iterations, connectivity, 0), (1,), iterations, connectivity, 1)


class LesionScores(collections.namedtuple("LesionScores", "lesion_dice sensitivity precision f1 counts lesions")):
    """What score_lesions returns, all on the device: lesion_dice, sensitivity, precision, f1 (N, R) fp64 - views of one (N, R, 4) buffer;
    NaN where a table overflowed - counts (N, R, 8) int64 = {n_ref, n_kept, n_tp, n_fn, n_fp, n_pred, lesions beyond max_lesions, components with links
    beyond max_links}, and lesions (N, R, max_lesions, 3) int64 = {gt_vol, inter, pred_vol} per reference lesion, or None when it was not asked for.
    hd95, hd_lesions and hd_counts read as None: the lesion-wise HD95 was not asked for (score_lesions(hd95=True) returns a LesionHD95Scores)."""
    __slots__ = ()
    hd95 = hd_lesions = hd_counts = None


LesionHD95Scores = collections.namedtuple("LesionHD95Scores", LesionScores._fields + ("hd95", "hd_lesions", "hd_counts"))
LesionHD95Scores.__doc__ = """What score_lesions(hd95=True) returns: the six fields of LesionScores, then hd95 (N, R) fp64, the lesion-wise HD95 - NaN where a table or a
border list overflowed -, hd_lesions (N, R, max_lesions, 3) int64 = {m, s[k0], s[k1]} per matched reference lesion (the number of surface distances
and the two squared distances the 95th percentile lies between), or None when the per-lesion tables were not asked for, and hd_counts (N, R, 2)
int64 = {reference border voxels beyond max_border, (predicted border voxel, lesion) entries of the row beyond max_border}."""


def score_lesions(pred, reference, pred_regions, ref_regions=None, dilation=3, min_ref_voxels=50, min_pred_voxels=0, max_lesions=256, max_links=4,
                  return_lesions=False, hd95=False, hd95_penalty=374.0, max_border=None):
    """Lesion-wise scores of N label volumes against ONE reference volume for R regions, the operands of score_volume (a 3-D
    Prediction, filtered or not - its S samples, then mean_label - or a uint8 tensor (N, D, H, W); reference uint8 (D, H, W)) - one
    uz_vol_lesion_scores call (csrc/vollesion.hip) on the caller's current stream: no host round trip, no synchronisation.
    Per region: the reference lesions are the 26-connected components of the reference region dilated `dilation` times with the
    18-neighbour structure (two blobs the dilation joins are one lesion; a lesion's volume counts its undilated voxels); a lesion is
    matched to every predicted 26-connected component that reaches its dilated extent, and its Dice is 2 |lesion and prediction| /
    (|lesion| + the full sizes of those components).  Lesions of fewer than min_ref_voxels voxels are dropped from every sum; a
    predicted component that reaches no dilated lesion at all and has at least min_pred_voxels voxels is a false positive.
    lesion_dice = (sum of the kept lesions' Dice) / (kept lesions + false positives), 1 when both are none: every missed lesion and
    every false positive enters as a 0.  sensitivity, precision and f1 count kept lesions with a match, without one, and the false
    positives.  The definition is this project's contract (include/uz_api.h spells it out); it follows the description of the BraTS
    2023 ranking, parity with the challenge's own tool is not pinned, and the defaults - dilation 3, min_ref_voxels 50 - are OUR
    reading of its glioma settings.
    max_lesions (1 .. 4096) bounds the per-lesion tables and max_links (1 .. 16) the lesions one predicted component may reach; where
    either is exceeded the scores of that (row, region) are NaN and counts[..., 6] / counts[..., 7] say by how much - nothing is
    looked at on the host, so nothing raises.  Returns a LesionScores of device tensors.
    hd95=True adds the lesion-wise HD95 (one uz_vol_lesion_scores_ex call) and returns a LesionHD95Scores: per matched lesion the 95th
    percentile (score_volume's rule) of the surface distances, both directions, between the lesion's undilated voxels and the union of
    the predicted components matched to it, each component whole; hd95 = (the kept lesions' values, hd95_penalty for every missed one
    and for every false positive) / (kept lesions + false positives), 0 when both are none.  hd95_penalty, a finite real >= 0,
    defaults to 374, the value the challenge's description gives.  max_border caps two lists per row, the border voxels of the
    reference lesions and the (border voxel, lesion) entries of the predicted components: None = max(4096, D*H*W // 8), at most D*H*W - a border is
    a few per cent of a mask and a tumour about 1 % of a case - or an int 1 .. D*H*W.  Where a list overflows, hd95 of that (row,
    region) is NaN, hd_counts says by how much, and the other scores stand: call again with a larger max_border (D*H*W always
    suffices for the reference list; the workspace grows by 20 bytes per row and entry)."""
    if _vol.is_prediction(pred):
        rows = _vol.prediction_rows(*_vol.prediction_maps(pred))
    else:
        rows = _vol.label_tensor(pred, "pred", "(N, D, H, W)", 4, also="a Prediction or ")
    _vol.label_tensor(reference, "reference", "(D, H, W)")
    if tuple(reference.shape) != tuple(rows.shape[1:]):
        raise ValueError(f"reference {tuple(reference.shape)} does not match the volumes {tuple(rows.shape[1:])} of pred")
    if reference.device != rows.device:
        raise ValueError("reference must be on the device of pred")
    psets, rsets = _vol.region_set_pair(pred_regions, ref_regions)
    for name, v, lo, hi in (("dilation", dilation, 0, 16), ("min_ref_voxels", min_ref_voxels, 0, None), ("min_pred_voxels", min_pred_voxels, 0, None),
                            ("max_lesions", max_lesions, 1, 4096), ("max_links", max_links, 1, 16)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} must be an int, not {v!r}")
        if v < lo or (hi is not None and v > hi):
            raise ValueError(f"{name} {v}: {lo} <= {name}" + (f" <= {hi}" if hi is not None else ""))
    N, D, H, W = (int(d) for d in rows.shape)
    if not isinstance(hd95, bool):
        raise TypeError(f"hd95 must be a bool, not {hd95!r}")
    if isinstance(hd95_penalty, bool) or not isinstance(hd95_penalty, (int, float)):
        raise TypeError(f"hd95_penalty must be a real number, not {hd95_penalty!r}")
    if not (math.isfinite(hd95_penalty) and hd95_penalty >= 0):
        raise ValueError(f"hd95_penalty {hd95_penalty}: a finite distance >= 0")
    if max_border is not None:
        if isinstance(max_border, bool) or not isinstance(max_border, int):
            raise TypeError(f"max_border must be None or an int, not {max_border!r}")
        if max_border < 1 or max_border > D * H * W:
            raise ValueError(f"max_border {max_border}: 1 <= max_border <= D*H*W = {D * H * W}")
    elif hd95:
        max_border = min(max(4096, D * H * W // 8), D * H * W)
    _vol.on_device(rows, "pred")
    R = len(psets)
    L, dev = _ffi.lib(), rows.device
    too_large = f"N {N} R {R} volume {D} x {H} x {W}; no empty axis, 1 <= N <= 65536, 1 <= R <= 8, N*D*H*W < 2^31"
    if hd95:
        nbytes = L.uz_vol_lesion_scores_workspace_ex(N, R, D, H, W, max_lesions, 1, max_border)
        too_large += ", D^2 + H^2 + W^2 <= 2^30"
    else:
        nbytes = L.uz_vol_lesion_scores_workspace(N, R, D, H, W, max_lesions)
    if nbytes == 0:
        raise _vol.refused("score_lesions", too_large)
    rows, reference = rows.contiguous(), reference.contiguous()
    ws = _vol.workspace("score_lesions", (dev, N, R, D, H, W, max_lesions, bool(hd95), max_border if hd95 else None), nbytes, dev)
    scores = torch.empty(N, R, 4, dtype=torch.float64, device=dev)
    counts = torch.empty(N, R, 8, dtype=torch.int64, device=dev)
    lesions = torch.empty(N, R, max_lesions, 3, dtype=torch.int64, device=dev) if return_lesions else None
    U32 = C.c_uint32 * R
    head = (rows.data_ptr(), N, U32(*psets), reference.data_ptr(), U32(*rsets), R, D, H, W, dilation, min_ref_voxels, min_pred_voxels, max_lesions, max_links)
    tail = (ws.data_ptr(), counts.data_ptr(), lesions.data_ptr() if return_lesions else None, scores.data_ptr())
    six = dict(lesion_dice=scores[..., 0], sensitivity=scores[..., 1], precision=scores[..., 2], f1=scores[..., 3], counts=counts, lesions=lesions)
    if not hd95:
        _ffi.check(L.uz_vol_lesion_scores(*head, *tail, _vol.stream(dev)), "vol_lesion_scores")
        return LesionScores(**six)
    hd = torch.empty(N, R, dtype=torch.float64, device=dev)
    hd_counts = torch.empty(N, R, 2, dtype=torch.int64, device=dev)
    hd_lesions = torch.empty(N, R, max_lesions, 3, dtype=torch.int64, device=dev) if return_lesions else None
    _ffi.check(L.uz_vol_lesion_scores_ex(*head, 1, C.byref(C.c_double(float(hd95_penalty))), max_border, *tail, hd_counts.data_ptr(),
                                         hd_lesions.data_ptr() if return_lesions else None, hd.data_ptr(), _vol.stream(dev)), "vol_lesion_scores_ex")
    return LesionHD95Scores(hd95=hd, hd_lesions=hd_lesions, hd_counts=hd_counts, **six)


# --------------------------------------------------------------------------- S samples of one volume as an uncertainty estimate: filtered Dice, calibration
UncertaintyScores = collections.namedtuple("UncertaintyScores", "table levels dice ftp ftn auc calibration votes")
UncertaintyScores.__doc__ = """What score_uncertainty returns, all on the device, per region r: table (R, S+1, 2, 2) int64 = voxels with c of the S samples in
the region, decision d and reference t; levels (R, S+1, 4) int64 = {tp, fp, fn, tn} over the voxels on which at most j samples contradict the
decision; dice, ftp, ftn (R, S+1) fp64 - views of one (R, S+1, 3) buffer -: the filtered Dice and the filtered shares of true positives and
true negatives at level j; auc (R, 4) fp64 = {auc_dice, auc_ftp, auc_ftn, score}, score the BraTS uncertainty-task score; calibration (R, 3)
fp64 = {ece, mce, brier} of the vote frequencies c / S; votes (R, D, H, W) uint8 = c, or None when it was not asked for."""


def score_uncertainty(pred, reference, pred_regions, ref_regions=None, decision=None, return_votes=False):
    """Judges S samples of ONE volume as an uncertainty estimate against `reference`, for R regions given as in score_volume - one
    uz_vol_uncertainty call (csrc/voluncert.hip) on the caller's current stream: no host round trip, no synchronisation, no ATen
    arithmetic on the volumes.  A voxel's uncertainty in a region is the share of the samples that contradict the decision there;
    the levels j = 0 .. S keep the voxels with at most j such samples (include/uz_api.h "volume uncertainty" has every definition).
    pred: a Prediction of PHISeg3D.predict / predict_volume - labels (S, 1, D, H, W), the decision is mean_label -, as it is or as
    keep_largest_components returns it; or a uint8 tensor (S, D, H, W), and then `decision` is required.  decision: uint8 (D, H, W)
    or (1, D, H, W), overrides the decision volume (for instance the filtered mean label while the samples stay unfiltered).
    reference: uint8 (D, H, W) on the same device.  Returns an UncertaintyScores of device tensors."""
    if _vol.is_prediction(pred):
        labels, mean_label = _vol.prediction_maps(pred)
        samples = labels[:, 0]
        dec = mean_label[0] if decision is None else decision
    else:
        samples = _vol.label_tensor(pred, "pred", "(S, D, H, W)", 4, also="a Prediction or ")
        if decision is None:
            raise ValueError("decision is required when pred is a tensor of samples: the volume the samples are judged against")
        dec = decision
    vol = tuple(samples.shape[1:])
    _vol.label_tensor(dec, "decision", "(D, H, W)")
    _vol.label_tensor(reference, "reference", "(D, H, W)")
    if dec.dim() == 4 and int(dec.shape[0]) == 1:
        dec = dec[0]
    if tuple(dec.shape) != vol:
        raise ValueError(f"decision {tuple(dec.shape)} does not match the volumes {vol} of pred")
    if tuple(reference.shape) != vol:
        raise ValueError(f"reference {tuple(reference.shape)} does not match the volumes {vol} of pred")
    if reference.device != samples.device or dec.device != samples.device:
        raise ValueError("reference and decision must be on the device of pred")
    psets, rsets = _vol.region_set_pair(pred_regions, ref_regions)
    _vol.on_device(samples, "pred")
    S, D, H, W = (int(d) for d in samples.shape)
    R = len(psets)
    L, dev = _ffi.lib(), samples.device
    nbytes = L.uz_vol_uncertainty_workspace(S, R, D, H, W)
    if nbytes == 0:
        raise _vol.refused("score_uncertainty", f"S {S} R {R} volume {D} x {H} x {W}; 1 <= S <= 255, 1 <= R <= 8, no empty axis, S*D*H*W < 2^31")
    samples, dec, reference = samples.contiguous(), dec.contiguous(), reference.contiguous()
    ws = _vol.workspace("score_uncertainty", (dev, S, R, D, H, W), nbytes, dev)
    table = torch.empty(R, S + 1, 2, 2, dtype=torch.int64, device=dev)
    levels = torch.empty(R, S + 1, 4, dtype=torch.int64, device=dev)
    curves = torch.empty(R, S + 1, 3, dtype=torch.float64, device=dev)
    auc = torch.empty(R, 4, dtype=torch.float64, device=dev)
    calibration = torch.empty(R, 3, dtype=torch.float64, device=dev)
    votes = torch.empty(R, D, H, W, dtype=torch.uint8, device=dev) if return_votes else None
    U32 = C.c_uint32 * R
    _ffi.check(L.uz_vol_uncertainty(samples.data_ptr(), S, dec.data_ptr(), U32(*psets), reference.data_ptr(), U32(*rsets), R, D, H, W,
                                    ws.data_ptr(), table.data_ptr(), levels.data_ptr(), curves.data_ptr(), auc.data_ptr(), calibration.data_ptr(),
                                    votes.data_ptr() if return_votes else None, _vol.stream(samples.device)), "vol_uncertainty")
    return UncertaintyScores(table=table, levels=levels, dice=curves[..., 0], ftp=curves[..., 1], ftn=curves[..., 2], auc=auc,
                             calibration=calibration, votes=votes)
