"""Every case of tests/_augment3d.py through uz_augment_volume against the fp64 restatement of the stage rules, and BratsDataset on
top of it.  Every operand - the workspace included - is a view inside a larger allocation filled with NaN (floats) or a sentinel
(bytes): inputs must keep every bit, outputs every bit outside the view, and a result that read unwritten workspace would be NaN.
Gates: labels equal wherever the fp64 label margin is at least 1e-4 (y_eval exactly the three nested maps of the y_raw that was
written); elastic-only cases on a ramp of the voxel index within the fp32 rounding of ONE bilinear blend on every voxel - a single
differing entry of the integer maps moves a voxel by at least Z / 32 ramp units, so this demands equal maps, ties included; images
in general no further from fp64 than 4 x the numpy float32 restatement is on the same case, over voxels whose image margin is at
least 1e-4; at most 1 % of a case's voxels below a margin.  `-s` prints every measured distance.
The kernels of csrc/augment3d.hip are streaming kernels: they do not read the arithmetic mode, so nothing here sets one."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import _augment3d as A

pytestmark = pytest.mark.gpu

PAD = 8
BYTE_SENTINEL = 0xEE


def _g():
    from tests import _gpu
    return _gpu


def _rc(name, *args):
    from tests import _views
    return _views.rc(name, *args)


class Buf:
    """A contiguous array that starts `off` elements into an allocation filled with NaN / a sentinel (data None: an output)."""

    def __init__(self, shape, dtype, off, data=None):
        self.n, self.off = int(np.prod(shape, dtype=np.int64)), off
        fill = float("nan") if dtype == torch.float32 else BYTE_SENTINEL
        self.flat = torch.full((off + self.n + PAD,), fill, dtype=dtype, device=_g().dev())
        self.ptr = self.flat[off:off + self.n]
        if data is not None:
            self.ptr.copy_(torch.from_numpy(np.array(data)).reshape(-1).to(dtype))
        self.shape, self.bits = tuple(shape), torch.int32 if dtype == torch.float32 else torch.uint8
        self.before = self.flat.clone()
        assert self.flat.data_ptr() % 256 == 0

    def get(self):
        return self.ptr.cpu().numpy().reshape(self.shape)

    def outside_untouched(self):
        a, b = self.flat.view(self.bits), self.before.view(self.bits)
        return torch.equal(a[:self.off], b[:self.off]) and torch.equal(a[self.off + self.n:], b[self.off + self.n:])

    def untouched(self):
        return torch.equal(self.flat.view(self.bits), self.before.view(self.bits))


def _operands(c, r):
    X, Y, Z = c.shape
    ws_bytes = _g().L().uz_augment_volume_workspace(c.C, X, Y, Z)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ops = dict(img=Buf(r["img"].shape, torch.float32, 1 if c.offset4 else 4, r["img"]), lbl=Buf(r["lbl"].shape, torch.uint8, 3, r["lbl"]),
               ws=Buf((ws_bytes // 4,), torch.float32, 4), x=Buf((c.C, *c.out_shape), torch.float32, 7),
               ye=Buf((3, *c.out_shape), torch.float32, 5), yr=Buf(c.out_shape, torch.uint8, 3))
    assert (ops["img"].ptr.data_ptr() % 16 == 0) == (not c.offset4) and ops["ws"].ptr.data_ptr() % 16 == 0
    return ops


def _call(c, ops, prm, crop=None, null=()):
    P = lambda k: None if k in null else ops[k].ptr
    return _rc("uz_augment_volume", P("img"), P("lbl"), c.C, *c.shape, prm.ctypes.data, *(crop or c.out_shape), P("ws"), P("x"), P("ye"), P("yr"))


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_volume_against_the_fp64_restatement(name):
    r = A.reference(name)
    c = r["case"]
    out = (C.c_int * 2)()
    assert _g().L().uz_augment_volume_route(c.C, *c.shape, 4 if c.offset4 else 16, out) == 0
    assert out[0] == int(c.C == 4 and not c.offset4)
    ops = _operands(c, r)
    prm = np.array(r["prm"])
    assert _call(c, ops, prm) == 0
    assert ops["img"].untouched() and ops["lbl"].untouched() and np.array_equal(prm, r["prm"])
    for k in ("ws", "x", "ye", "yr"):
        assert ops[k].outside_untouched(), k
    x, ye, yr = ops["x"].get(), ops["ye"].get(), ops["yr"].get()
    # labels
    lsafe = np.ones(yr.shape, bool) if c.ramp else r["lmargin"] >= A.MARGIN
    isafe = np.ones(yr.shape, bool) if c.ramp else r["imargin"] >= A.MARGIN
    print(f"{name}: {int((~lsafe).sum())} labels and {int((~isafe).sum())} image voxels of {lsafe.size} below the margin, "
          f"{int((yr != r['y64']).sum())} labels differ in all")
    assert 1 - lsafe.mean() <= A.EXCLUDED_CAP and 1 - isafe.mean() <= A.EXCLUDED_CAP
    assert not ((yr != r["y64"]) & lsafe).any(), f"{int(((yr != r['y64']) & lsafe).sum())} labels differ where the fp64 margin is at least {A.MARGIN:g}"
    assert np.array_equal(ye, A.eval_maps(yr))
    # image (NaN - unwritten, or read from unwritten workspace - fails either comparison)
    err = np.abs(x.astype(np.float64) - r["x64"]).max(axis=0)
    assert not np.isnan(err).any()
    if c.ramp:
        gate = A.ramp_gate(r["img"])
        print(f"{name}: ramp error {err.max():.3e} (gate {gate:.3e}, one map step {c.shape[2] / 32:.3e})")
        assert err.max() <= gate
    else:
        e32 = float(np.abs(r["x32"].astype(np.float64) - r["x64"]).max(axis=0)[isafe].max())
        print(f"{name}: image error {err[isafe].max():.3e} (numpy float32 {e32:.3e}, gate {4 * e32:.3e})")
        assert err[isafe].max() <= 4 * e32
    # a repeated call is bit-equal
    assert _call(c, ops, prm) == 0
    assert np.array_equal(ops["x"].get().view(np.int32), x.view(np.int32)) and np.array_equal(ops["ye"].get(), ye) and np.array_equal(ops["yr"].get(), yr)


@pytest.mark.parametrize("name", ["all_A", "all_B_c3", "copy_offset4"])
def test_null_label_writes_the_image_only(name):
    r = A.reference(name)
    c = r["case"]
    ops = _operands(c, r)
    assert _call(c, ops, np.array(r["prm"]), null=("lbl", "ye", "yr")) == 0
    assert ops["ye"].untouched() and ops["yr"].untouched() and ops["lbl"].untouched() and ops["x"].outside_untouched() and ops["ws"].outside_untouched()
    x = ops["x"].get()
    full = _operands(c, r)
    assert _call(c, full, np.array(r["prm"])) == 0
    assert np.array_equal(x.view(np.int32), full["x"].get().view(np.int32))
    # each label output is optional on its own
    one = _operands(c, r)
    assert _call(c, one, np.array(r["prm"]), null=("ye",)) == 0
    assert one["ye"].untouched() and np.array_equal(one["yr"].get(), full["yr"].get())


def test_refused_call_writes_nothing():
    r = A.reference("all_A")
    c = r["case"]
    away = np.array(r["prm"]); away[31] = c.shape[0] - c.crop[0] + 1
    nan = np.array(r["prm"]); nan[16] = np.nan
    for kw in (dict(prm=away), dict(prm=nan), dict(crop=(8, 16, 9)), dict(null=("x",)), dict(null=("ws",)), dict(null=("lbl",)), dict(null=("img",))):
        ops = _operands(c, r)
        assert _call(c, ops, kw.get("prm", np.array(r["prm"])), kw.get("crop"), kw.get("null", ())) != 0, kw
        assert all(ops[k].untouched() for k in ops), kw
    r3 = A.reference("all_B_c3")
    shifted = np.array(r3["prm"]); shifted[25:30] = 1, 0.1, 0.1, 0.1, 0.1
    ops = _operands(r3["case"], r3)
    assert _call(r3["case"], ops, shifted) != 0 and all(ops[k].untouched() for k in ops)


# ================================================================================================ the dataset
class _Cfg:
    NN_AUGMENTATION, SOFT_AUGMENTATION, TRAIN_ORIGINAL_CLASSES = True, False, False
    DO_ROTATE, ROT_DEGREES, DO_SCALE, SCALE_FACTOR, DO_FLIP = True, 20, True, 1.1, True
    DO_ELASTIC_AUG, SIGMA, DO_INTENSITY_SHIFT, MAX_INTENSITY_SHIFT = True, 10, True, 0.1


def _split(mode, shape=(16, 24, 8)):
    vols = [A.case_volume(A.Case(name=f"v{i}", shape=shape, seed=50 + i)) for i in range(3)]
    return {f"images_{mode}": np.stack([v[0] for v in vols]), f"masks_{mode}": np.stack([v[1] for v in vols]), f"pids_{mode}": np.array([101, 102, 103])}


def test_dataset_items_are_the_kernel_on_the_drawn_table():
    from unet_zoo_amd.data.brats_dataset import BratsDataset
    data = _split("train")
    ds = BratsDataset(data, _Cfg, mode="train", randomCrop=(8, 16, 4))
    assert len(ds) == 3
    np.random.seed(3); random.seed(4)
    want = [ds.draw((16, 24, 8)) for _ in range(3)]
    np.random.seed(3); random.seed(4)
    for i in range(3):
        x, pid, y = ds[i]
        assert x.shape == (4, 8, 16, 4) and y.shape == (3, 8, 16, 4) and x.dtype == y.dtype == torch.float32
        assert x.device == y.device == _g().dev() and pid == str(data["pids_train"][i])
        x64, y64, lm, im = A.augment3d(data["images_train"][i], data["masks_train"][i], want[i], (8, 16, 4), np.float64)
        x32, _ = A.augment3d(data["images_train"][i], data["masks_train"][i], want[i], (8, 16, 4), np.float32)
        isafe, lsafe = im >= A.MARGIN, lm >= A.MARGIN
        err = np.abs(x.cpu().numpy().astype(np.float64) - x64).max(axis=0)[isafe].max()
        e32 = np.abs(x32.astype(np.float64) - x64).max(axis=0)[isafe].max()
        print(f"item {i}: image error {err:.3e} (numpy float32 {e32:.3e})")
        assert err <= 4 * e32
        assert not ((y.cpu().numpy() != A.eval_maps(y64)).any(axis=0) & lsafe).any()
    nomask = BratsDataset(data, _Cfg, mode="train", randomCrop=(8, 16, 4), hasMasks=False)
    item = nomask[1]
    assert len(item) == 2 and item[0].shape == (4, 8, 16, 4) and item[1] == 102


def test_dataset_val_mode_returns_the_volume_transposed():
    from unet_zoo_amd.data.brats_dataset import BratsDataset
    data = _split("val", (24, 16, 5))
    ds = BratsDataset(data, _Cfg, mode="val")
    state = np.random.get_state()[1].copy()
    x, pid, y = ds[2]
    assert np.array_equal(np.random.get_state()[1], state), "mode != train draws nothing from numpy"
    assert np.array_equal(x.cpu().numpy(), np.transpose(data["images_val"][2], (3, 0, 1, 2)))
    assert np.array_equal(y.cpu().numpy(), A.eval_maps(data["masks_val"][2])) and pid == "103"


def test_dataset_feeds_phiseg3d():
    from unet_zoo_amd.data.brats_dataset import BratsDataset
    from tests import _nets as N
    ds = BratsDataset(_split("train", (24, 24, 20)), _Cfg, mode="train", randomCrop=(16, 16, 16))
    np.random.seed(8); random.seed(9)
    x, _, y = ds[0]
    net = N.small_phiseg3d(dict(input_channels=4, num_classes=3, filters=[8, 16, 16], latent_levels=2, dhw=(16, 16, 16)))
    net.train()
    net.forward(x[None], y[None], training=True)
    loss = float(net.loss(y[1] + y[2]).detach())            # a class map 0..2 from the nested maps: background / whole, core, enhancing
    print(f"PHISeg3D loss on a dataset item: {loss:.4f}")
    assert np.isfinite(loss)
