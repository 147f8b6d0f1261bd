"""BraTS volume dataset - drop-in for the reference's ``data/bratsDataset.py`` ``BratsDataset`` (same constructor keywords, same
``expConfig`` names, ``__getitem__`` :34-113) with ``data/BratsProcessing/augmentation.py::augment3DImage`` (:12-104) behind it,
re-designed like ``batch_provider.py`` for a 288 GB GPU:

  * the split's volumes are uploaded ONCE, as the HDF5 file stores them (channels last), and stay resident in HBM;
  * an item costs the host only the random draws - rotation angle, scale, the two 3 x 3 elastic matrices, four intensity shifts
    and three flips from numpy's global RNG, then the crop origin from Python's ``random`` - in exactly the reference's order, so a
    seeded run consumes both random streams as the reference does;
  * rotate, scale + pad / crop, elastic warp, intensity shift, flips, random crop, ``_toEvaluationOneHot`` and the NCXYZ transpose
    are at most three stage launches of csrc/augment3d.hip (plus a small one for the elastic field) that write the
    (C, Xc, Yc, Zc) image and (3, Xc, Yc, Zc) label tensors ``PHISeg3D.forward`` consumes: no per-slice Python loop, no cv2.

``filePath`` is the HDF5 file (opened lazily, needs ``h5py``) or a mapping with ``images_<mode>`` (N, X, Y, Z, C), ``masks_<mode>``
(N, X, Y, Z) and ``pids_<mode>`` - and ``xOffsets_<mode>`` / ``yOffsets_<mode>`` / ``zOffsets_<mode>`` for ``returnOffsets=True``, which appends
the validation writer's crop offsets to the item as the reference does (bratsDataset.py:101-113).  A mapping's device tensors
(``data.prepare_cases(...).as_mapping(mode)``) are taken as they are, without a trip through the host.  Items are device tensors.  Without a GPU the dataset still draws (``draw_augmentation3d`` is host
code) but cannot assemble voxels - there is no CPU fallback for the product path.

Not built: ``NN_AUGMENTATION = False`` - the soft and hard one-hot label schemes, which resample one-hot label volumes bilinearly -
raises NotImplementedError.  Quirk kept: the intensity
shift is hard-coded to four channels (augmentation.py:83), so with fewer the reference raises and so does this.
"""
import random

import numpy as np
import torch

from .. import _ffi, _vol

NPRM = 34       # UZ_AUG3_NPRM (include/uz_api.h)


def _cfg(cfg, name):
    return cfg[name] if hasattr(cfg, "keys") else getattr(cfg, name)


def draw_augmentation3d(shape, cfg, randomCrop=None, augment=True):
    """The random parameters of one ``BratsDataset.__getitem__`` for a volume of `shape` = (X, Y, Z): the UZ_AUG3_NPRM float64 table
    {do_rot, cos, sin, do_scale, sX, sY, do_elastic, dx[9], dy[9], do_shift, shift[4], flips (bit 0, 1, 2 = axis X, Y, Z), ox, oy, oz}.
    numpy's global RNG in augment3DImage's order (:45, :52, :69, :73, :84, :89), each draw only when its stage is on and none with
    augment=False (mode != "train"); then Python's random.randint for the crop origin x, y, z (bratsDataset.py:80-84)."""
    X, Y, Z = shape
    p = np.zeros(NPRM, np.float64)
    p[1] = 1.0
    if augment:
        if _cfg(cfg, "DO_ROTATE"):
            ang = np.random.uniform(-_cfg(cfg, "ROT_DEGREES"), _cfg(cfg, "ROT_DEGREES"))
            p[0], p[1], p[2] = 1.0, np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))
        if _cfg(cfg, "DO_SCALE"):
            scale = np.random.uniform(1 / _cfg(cfg, "SCALE_FACTOR"), 1 * _cfg(cfg, "SCALE_FACTOR"))
            p[3], p[4], p[5] = 1.0, round(X * scale), round(Y * scale)
        if _cfg(cfg, "DO_ELASTIC_AUG"):
            p[6] = 1.0
            p[7:16] = np.random.normal(0, _cfg(cfg, "SIGMA"), 9)
            p[16:25] = np.random.normal(0, _cfg(cfg, "SIGMA"), 9)
        if _cfg(cfg, "DO_INTENSITY_SHIFT"):
            p[25] = 1.0
            for i in range(4):
                p[26 + i] = np.random.uniform(-_cfg(cfg, "MAX_INTENSITY_SHIFT"), _cfg(cfg, "MAX_INTENSITY_SHIFT"))
        if _cfg(cfg, "DO_FLIP"):
            flips = 0
            for i in range(3):
                if np.random.random() < 0.5:
                    flips |= 1 << i
            p[30] = flips
    if randomCrop is not None:
        p[31] = random.randint(0, X - randomCrop[0])
        p[32] = random.randint(0, Y - randomCrop[1])
        p[33] = random.randint(0, Z - randomCrop[2])
    return p


class BratsDataset(torch.utils.data.Dataset):
    # mode must be train, test or val
    def __init__(self, filePath, expConfig, mode="train", randomCrop=None, hasMasks=True, returnOffsets=False, device=None):
        super().__init__()
        self.filePath, self.mode, self.file = filePath, mode, None
        self.expConfig = expConfig
        self.trainOriginalClasses = _cfg(expConfig, "TRAIN_ORIGINAL_CLASSES")
        self.softAugmentation = _cfg(expConfig, "SOFT_AUGMENTATION")
        self.nnAugmentation = _cfg(expConfig, "NN_AUGMENTATION")
        for name in ("DO_ROTATE", "ROT_DEGREES", "DO_SCALE", "SCALE_FACTOR", "DO_FLIP", "DO_ELASTIC_AUG", "SIGMA", "DO_INTENSITY_SHIFT",
                     "MAX_INTENSITY_SHIFT"):
            _cfg(expConfig, name)                                  # a missing name fails here, as in the reference's constructor
        if not self.nnAugmentation:
            raise NotImplementedError("NN_AUGMENTATION = False (the soft / hard one-hot label schemes of bratsDataset.py:44-50,75-77) "
                                      "is not part of the native input pipeline")
        self.randomCrop = None if randomCrop is None else tuple(int(v) for v in randomCrop)
        self.hasMasks = hasMasks
        self.returnOffsets = returnOffsets
        self.device = torch.device(device) if device is not None else \
            (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        self._dev = None

    def openFileIfNotOpen(self):
        if self.file is None:
            if hasattr(self.filePath, "keys"):
                self.file = self.filePath
            else:
                import h5py
                self.file = h5py.File(self.filePath, "r")

    def __len__(self):
        self.openFileIfNotOpen()
        return self.file["images_" + self.mode].shape[0]

    def draw(self, shape):
        """The parameter table of the next item (host only)."""
        return draw_augmentation3d(shape, self.expConfig, self.randomCrop, augment=self.mode == "train")

    # ------------------------------------------------------------------ device residency
    def _resident(self):
        if self._dev is None:
            if self.device.type != "cuda":
                raise _ffi.UzError("no GPU visible: the native input pipeline assembles batches on the device (no CPU fallback)")
            self.openFileIfNotOpen()
            img = self.file["images_" + self.mode]
            if isinstance(img, torch.Tensor) and img.is_cuda:               # already resident (data.prepare_cases)
                img = img.to(self.device, torch.float32).contiguous()
            else:
                img = torch.as_tensor(np.ascontiguousarray(np.asarray(img[...], dtype=np.float32))).to(self.device)
            lbl = None
            if self.hasMasks:
                m = self.file["masks_" + self.mode]
                if isinstance(m, torch.Tensor) and m.is_cuda:
                    lbl = (m[..., 0] if m.dim() == 5 else m).to(self.device, torch.uint8).contiguous()
                else:
                    m = np.asarray(m[...])
                    if m.ndim == 5:
                        m = m[..., 0]
                    lbl = torch.as_tensor(np.ascontiguousarray(m.astype(np.uint8))).to(self.device)
            _, X, Y, Z, Cn = img.shape
            ws = torch.empty(_ffi.lib().uz_augment_volume_workspace(Cn, X, Y, Z), dtype=torch.uint8, device=self.device)
            self._dev = (img, lbl, ws)
        return self._dev

    def __getitem__(self, index):
        self.openFileIfNotOpen()
        shape = tuple(self.file["images_" + self.mode].shape[1:4])
        prm = self.draw(shape)
        img, lbl, ws = self._resident()
        _, X, Y, Z, Cn = img.shape
        Xc, Yc, Zc = self.randomCrop if self.randomCrop is not None else (X, Y, Z)
        x = torch.empty(Cn, Xc, Yc, Zc, device=self.device)
        y = torch.empty(3, Xc, Yc, Zc, device=self.device) if self.hasMasks else None
        _ffi.check(_ffi.lib().uz_augment_volume(img[index].data_ptr(), lbl[index].data_ptr() if self.hasMasks else None, Cn, X, Y, Z,
                                                prm.ctypes.data, Xc, Yc, Zc, ws.data_ptr(), x.data_ptr(),
                                                y.data_ptr() if self.hasMasks else None, None, _vol.stream(self.device)), "augment_volume")
        return self._item(index, x, y)

    def _item(self, index, x, y):
        """the reference's tuples (bratsDataset.py:98-113): image, pid, labels with masks, then the three crop offsets on request"""
        pid = self.file["pids_" + self.mode][index]
        item = (x, str(pid), y) if self.hasMasks else (x, pid)
        if self.returnOffsets:
            item += tuple(self.file[ax + "Offsets_" + self.mode][index] for ax in "xyz")
        return item
