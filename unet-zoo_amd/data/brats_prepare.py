"""Both ends of the mask-free loop of the 3-D model: raw BraTS cases in, native-space maps out.

``prepare_case`` / ``prepare_cases`` restate what the reference's loaders do to the four stacked modalities before the HDF5 file
stores them (data/BratsProcessing/brats18_data_loader.py:31-96,196-220, brats18_validation_data_loader.py:27-74,172-191) -
``crop_volume_allDim``, ``crop_or_pad_slice_to_size`` (centred for training, at the corner for validation), ``normalise_image`` - as
ONE uz_vol_prepare call per case (csrc/volprep.hip) on the caller's current stream: the case is uploaded once if it is on the host,
the box never comes back.  ``restore_volume`` is the way back: label maps, vote maps and entropy maps of target extent into the
240 x 240 x 155 case, raw label values 0 / 1 / 2 / 4 on request - what a BraTS segmentation or uncertainty submission holds.
include/uz_api.h "volume preparation" has every rule.

Statistics follow the validation loader's fp64 route (DESIGN.md 2g says what the training loader's fp32 route does instead).

Not built: reading NIfTI files (arrays in, arrays out), resampling to another resolution (``pixel_size != target_resolution`` raises
NotImplementedError; BraTS is 1 mm isotropic), int16 input, the soft / hard one-hot label schemes.
"""
import collections
import ctypes as C

import numpy as np
import torch

from .. import _ffi, _vol

PLACEMENTS = {"centre": 0, "center": 0, "corner": 1}


class PreparedCase(collections.namedtuple("PreparedCase", "image mask info stats")):
    """What prepare_case returns, all on the device: image (Xt, Yt, Zt, C) fp32 - the HDF5 layout BratsDataset keeps resident -, mask
    (Xt, Yt, Zt) uint8 or None, info int32[16] = {box x0 y0 z0 x1 y1 z1, n[3], t[3], e[3], flags} and stats (C, 3) fp64 = {count, mean,
    std} (include/uz_api.h "volume preparation")."""
    __slots__ = ()

    @property
    def place(self):
        """info[6..14] = {n, t, e} on the device: what restore_volume takes"""
        return self.info[6:15]

    def offsets(self):
        """The three ints the validation writer stores as xOffsets / yOffsets / zOffsets: the origin of the box.  Reads info once
        (this synchronises).  An empty case raises ValueError - the reference's crop raises there too."""
        h = self.info.cpu().tolist()
        if h[15] & 1:
            raise ValueError("empty case: no voxel > 0 in any channel, there is no box")
        return int(h[0]), int(h[1]), int(h[2])


class PreparedSplit(collections.namedtuple("PreparedSplit", "images masks pids info")):
    """What prepare_cases returns: images (N, Xt, Yt, Zt, C) fp32 and masks (N, Xt, Yt, Zt) uint8 (or None) on the device, pids a list
    of str, info (N, 16) int32 on the device."""
    __slots__ = ()

    def as_mapping(self, mode):
        """The images_<mode> / masks_<mode> / pids_<mode> / xOffsets_<mode> / yOffsets_<mode> / zOffsets_<mode> mapping BratsDataset
        takes as filePath; images and masks stay the device tensors they are.  Reads info once for the offsets."""
        h = self.info.cpu().numpy()
        m = {"images_" + mode: self.images, "pids_" + mode: list(self.pids)}
        if self.masks is not None:
            m["masks_" + mode] = self.masks
        for k, ax in enumerate("xyz"):
            m[ax + "Offsets_" + mode] = h[:, k].astype(np.int64)
        return m


def _device(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise _ffi.UzError("no GPU visible: cases are prepared on the device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _upload(a, dtype, what, dev):
    if isinstance(a, torch.Tensor):
        if a.dtype != dtype:
            raise TypeError(f"{what} must be {dtype}, not {a.dtype}")
        dev = a.device if dev is None and a.is_cuda else _device(dev)
        return a.to(dev).contiguous(), dev
    a = np.asarray(a)
    want = np.float32 if dtype == torch.float32 else np.uint8
    if a.dtype != want:
        raise TypeError(f"{what} must be {np.dtype(want).name}, not {a.dtype}")
    dev = _device(dev)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev), dev


def prepare_case(raw, mask=None, size=(160, 192, 160), placement="centre", pixel_size=None, target_resolution=None, out=None, device=None):
    """One raw case -> PreparedCase.  raw: numpy or torch (X, Y, Z, C) fp32, the stacked modalities; mask: (X, Y, Z) uint8 or None;
    size: the target extent; placement "centre" (the training loader) or "corner" (the validation loader).  out: (image, mask) or
    (image, None) to write into - dense device tensors of the result's shapes, for instance slice i of a split's resident tensors."""
    if (pixel_size is None) != (target_resolution is None) or \
            (pixel_size is not None and tuple(float(v) for v in pixel_size) != tuple(float(v) for v in target_resolution)):
        raise NotImplementedError("resampling to another resolution (pixel_size != target_resolution) is not built: BraTS is 1 mm isotropic")
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be 'centre' or 'corner', not {placement!r}")
    if len(size) != 3 or any(int(v) < 1 for v in size):
        raise ValueError(f"size {tuple(size)} is not three positive extents")
    if getattr(raw, "ndim", 0) != 4:
        raise ValueError(f"raw {tuple(getattr(raw, 'shape', ()))} is not (X, Y, Z, C)")
    if mask is not None and tuple(mask.shape) != tuple(raw.shape[:3]):
        raise ValueError(f"mask {tuple(mask.shape)} does not match raw {tuple(raw.shape[:3])}")
    raw, dev = _upload(raw, torch.float32, "raw", device)
    if mask is not None:
        mask, _ = _upload(mask, torch.uint8, "mask", dev)
    X, Y, Z, Cn = (int(d) for d in raw.shape)
    Xt, Yt, Zt = (int(v) for v in size)
    L = _ffi.lib()
    nbytes = L.uz_vol_prepare_workspace(Cn, X, Y, Z, Xt, Yt, Zt)
    if nbytes == 0:
        raise _vol.refused("prepare_case", f"raw {X} x {Y} x {Z} x {Cn} into {Xt} x {Yt} x {Zt}; no empty axis, 1 <= C <= 8, X*Y*Z*C < 2^31, Xt*Yt*Zt*C < 2^31")
    if out is None:
        image = torch.empty(Xt, Yt, Zt, Cn, device=dev)
        mask_out = torch.empty(Xt, Yt, Zt, dtype=torch.uint8, device=dev) if mask is not None else None
    else:
        image, mask_out = out
        if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or tuple(image.shape) != (Xt, Yt, Zt, Cn) or \
                not image.is_contiguous() or image.device != dev:
            raise ValueError(f"out[0] must be a dense fp32 ({Xt}, {Yt}, {Zt}, {Cn}) tensor on {dev}")
        if (mask_out is None) != (mask is None):
            raise ValueError("out[1] goes with mask: both or neither")
        if mask_out is not None and (mask_out.dtype != torch.uint8 or tuple(mask_out.shape) != (Xt, Yt, Zt) or not mask_out.is_contiguous()
                                     or mask_out.device != dev):
            raise ValueError(f"out[1] must be a dense uint8 ({Xt}, {Yt}, {Zt}) tensor on {dev}")
    ws = _vol.workspace("prepare_case", (dev, Cn, X, Y, Z, Xt, Yt, Zt), nbytes, dev)          # a split's cases share one
    info = torch.empty(16, dtype=torch.int32, device=dev)
    stats = torch.empty(Cn, 3, dtype=torch.float64, device=dev)
    _ffi.check(L.uz_vol_prepare(raw.data_ptr(), mask.data_ptr() if mask is not None else None, Cn, X, Y, Z, Xt, Yt, Zt, PLACEMENTS[placement],
                                ws.data_ptr(), image.data_ptr(), mask_out.data_ptr() if mask_out is not None else None, info.data_ptr(),
                                stats.data_ptr(), _vol.stream(raw.device)), "vol_prepare")
    return PreparedCase(image=image, mask=mask_out, info=info, stats=stats)


def prepare_cases(raws, masks, pids, size=(160, 192, 160), placement="centre", device=None):
    """A split: every case through prepare_case into slice i of ONE resident tensor -> PreparedSplit.  masks: a sequence as long as
    raws, or None.  The cases may differ in native shape (the workspace is then re-made per shape)."""
    raws, pids = list(raws), [str(p) for p in pids]
    if masks is not None:
        masks = list(masks)
        if len(masks) != len(raws):
            raise ValueError(f"{len(masks)} masks for {len(raws)} cases")
    if len(pids) != len(raws):
        raise ValueError(f"{len(pids)} pids for {len(raws)} cases")
    if not raws:
        raise ValueError("no cases")
    first = raws[0]
    dev = first.device if isinstance(first, torch.Tensor) and first.is_cuda and device is None else _device(device)
    N, Cn = len(raws), int(first.shape[-1])
    Xt, Yt, Zt = (int(v) for v in size)
    images = torch.empty(N, Xt, Yt, Zt, Cn, device=dev)
    mks = torch.empty(N, Xt, Yt, Zt, dtype=torch.uint8, device=dev) if masks is not None else None
    info = torch.empty(N, 16, dtype=torch.int32, device=dev)
    for i, raw in enumerate(raws):
        if int(raw.shape[-1]) != Cn:
            raise ValueError(f"case {i} has {int(raw.shape[-1])} channels, case 0 has {Cn}")
        case = prepare_case(raw, None if masks is None else masks[i], size, placement, out=(images[i], None if mks is None else mks[i]), device=dev)
        info[i].copy_(case.info)
    return PreparedSplit(images=images, masks=mks, pids=pids, info=info)


def _place_tensor(place, target, native, dev):
    """device int32[9] = {n, t, e}"""
    if isinstance(place, PreparedCase):
        place = place.place
    if isinstance(place, torch.Tensor):
        if place.dtype != torch.int32 or place.numel() != 9:
            raise ValueError(f"place as a tensor is int32[9] = info[6..14], not {place.dtype}{tuple(place.shape)}")
        if place.device != dev:
            raise ValueError("place must be on the device of x")
        return place.contiguous()
    off = [int(v) for v in place]
    if len(off) != 3:
        raise ValueError(f"place as host offsets is three ints (x, y, z), got {len(off)}")
    if any(o < 0 or o >= n for o, n in zip(off, native)):
        raise ValueError(f"offsets {tuple(off)} lie outside the native volume {tuple(native)}")
    ext = [min(t, n - o) for t, n, o in zip(target, native, off)]           # the corner placement of the validation writer
    return torch.tensor(off + [0, 0, 0] + ext, dtype=torch.int32).to(dev)


def _restore_rows(rows, place, native, lut, fill):
    N, Xt, Yt, Zt = (int(d) for d in rows.shape)
    X, Y, Z = native
    elem = 1 if rows.dtype == torch.uint8 else 4
    if elem == 4 and lut is not None:
        raise ValueError("lut maps uint8 rows only, not fp32")
    rows = rows.contiguous()
    out = torch.empty(N, X, Y, Z, dtype=rows.dtype, device=rows.device)
    lut_arg = None
    if lut is not None:
        table = np.arange(256, dtype=np.uint8)
        vals = np.asarray(lut)
        if vals.ndim != 1 or len(vals) > 256 or vals.min() < 0 or vals.max() > 255:
            raise ValueError("lut is at most 256 values 0 .. 255, index = value of x")
        table[:len(vals)] = vals.astype(np.uint8)
        lut_arg = table.ctypes.data
    if elem == 1:
        if not 0 <= int(fill) <= 255 or int(fill) != fill:
            raise ValueError(f"fill {fill!r} is not a byte")
        f = C.c_uint8(int(fill))
    else:
        f = C.c_float(float(fill))
    _ffi.check(_ffi.lib().uz_vol_restore(rows.data_ptr(), elem, N, Xt, Yt, Zt, place.data_ptr(), lut_arg, C.addressof(f), out.data_ptr(), X, Y, Z,
                                         _vol.stream(rows.device)), "vol_restore")
    return out


def restore_volume(x, place, native_shape=(240, 240, 155), lut=None, fill=0):
    """Target-extent maps back into the native case - uz_vol_restore (csrc/volprep.hip) on the caller's current stream.
    x: a uint8 or fp32 device tensor (N, Xt, Yt, Zt) -> (N, X, Y, Z), or (Xt, Yt, Zt) -> (X, Y, Z); or a Prediction of PHISeg3D -
    its S samples and mean label go through ONE call, its entropy through a second, fp32 one (fill 0) -> a new Prediction with labels
    (S, 1, X, Y, Z), mean_label (1, X, Y, Z) and entropy (1, X, Y, Z); mean_soft, levels and soft are in target space and become None.
    place: a PreparedCase or its device int32[9] info[6..14]; or the three host offsets of an HDF5 file (xOffsets, yOffsets, zOffsets:
    corner placement, extent = min(target, native - offset)).  lut: values indexed by the value of x, uint8 only - metrics.BRATS_LABELS
    turns class indices into raw labels; it maps x, never fill.  Voxels outside the placed block are `fill`."""
    native = tuple(int(v) for v in native_shape)
    if len(native) != 3 or any(v < 1 for v in native):
        raise ValueError(f"native_shape {native} is not three positive extents")
    if _vol.is_prediction(x):
        (labels, mean_label), entropy = _vol.prediction_maps(x), x.entropy
        _vol.on_device(labels, "x")
        rows = _vol.prediction_rows(labels, mean_label)
        pl = _place_tensor(place, tuple(rows.shape[1:]), native, rows.device)
        out = _restore_rows(rows, pl, native, lut, fill)
        S = int(labels.shape[0])
        ent = None
        if entropy is not None:
            ent = _restore_rows(entropy.reshape(1, *rows.shape[1:]).float(), pl, native, None, 0.0)
        return type(x)(labels=out[:S].unsqueeze(1), mean_soft=None, mean_label=out[S:], entropy=ent, levels=None, soft=None)
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.uint8, torch.float32):
        raise TypeError("x must be a Prediction or a uint8 / fp32 tensor (N, Xt, Yt, Zt) or (Xt, Yt, Zt)")
    if x.dim() not in (3, 4):
        raise ValueError(f"x {tuple(x.shape)} is not (N, Xt, Yt, Zt) or (Xt, Yt, Zt)")
    _vol.on_device(x, "x")
    rows = x if x.dim() == 4 else x[None]
    out = _restore_rows(rows, _place_tensor(place, tuple(rows.shape[1:]), native, rows.device), native, lut, fill)
    return out if x.dim() == 4 else out[0]
