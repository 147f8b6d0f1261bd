"""The volume input pipeline without a GPU: the case set of tests/_augment3d.py has the properties its GPU test relies on, every
deliberate defect of the numpy restatement changes what some case expects, the host-side draws consume numpy's and Python's random
streams as a replay of the reference's calls does, uz_augment_volume_route claims what the predicate says, and a bad call is
refused with its reason before anything is launched (the library loads, and refuses, without a device)."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import _augment3d as A


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib(), _ffi


# ================================================================================================ the case set
def test_case_set_covers_what_the_kernel_can_get_wrong():
    cs = A.CASES
    assert len({c.name for c in cs}) == len(cs)
    assert {c.shape for c in cs} == {(16, 24, 8), (24, 16, 5), (8, 8, 4)}
    assert {1, 3, 4} <= {c.C for c in cs}
    assert any(c.C == 4 and c.offset4 for c in cs) and any(c.C == 4 and not c.offset4 for c in cs)
    assert {0.0, 20.0, -20.0, 90.0} <= {c.angle for c in cs if c.angle is not None}
    scales = {c.scale for c in cs if c.scale is not None}
    assert {1 / 1.1, 1.1, A.SCALE_SAME} <= scales
    for shape in {c.shape for c in cs if c.scale == A.SCALE_SAME}:
        assert (round(shape[0] * A.SCALE_SAME), round(shape[1] * A.SCALE_SAME)) == shape[:2]
    assert {0.0, 10.0} <= {c.sigma for c in cs if c.sigma is not None}
    assert {c.flips for c in cs} == set(range(8))
    cropped = [c for c in cs if c.crop]
    assert all(c.crop == (8, 16, 4) for c in cropped)
    assert any(c.origin == (0, 0, 0) for c in cropped) and any(c.origin == tuple(s - k for s, k in zip(c.shape, c.crop)) for c in cropped)
    stages = lambda c: (c.angle is not None, c.scale is not None, c.sigma is not None or c.ties, c.shift, c.flips != 0)
    for alone in np.eye(5, dtype=bool):
        assert any(stages(c) == tuple(alone) for c in cs), alone
    assert any(all(stages(c)) for c in cs)
    for c in cs:
        assert not c.ramp or stages(c) == (False, False, True, False, False), c.name          # ramp cases are elastic only
        assert not c.shift or c.C >= 4
        lbl = A.case_volume(c)[1]
        assert set(np.unique(lbl)) <= {0, 1, 2, 4} and len(np.unique(lbl)) >= 3, c.name       # blobs: borders exist
        assert (np.diff(lbl.astype(int), axis=0) != 0).any() and (np.diff(lbl.astype(int), axis=1) != 0).any()


def test_sigma_10_reflects_more_than_once_and_ties_sit_on_ties():
    far = 0
    for c in A.CASES:
        if c.sigma == 10.0 and c.angle is None:
            X, Y, _ = c.shape
            p = A.case_prm(c)
            mx, my, _, _ = A.elastic_maps(X, Y, p[7:16], p[16:25])
            qx, qy = A.quantised_maps(mx, my)
            far += int((((qx >> 5) < -Y) | ((qx >> 5) >= 2 * Y) | ((qy >> 5) < -X) | ((qy >> 5) >= 2 * X)).sum())
    assert far > 0, "no sigma-10 case leaves the plane by more than its width"
    c = next(k for k in A.CASES if k.ties)
    p = A.case_prm(c)
    mx, my, _, _ = A.elastic_maps(c.shape[0], c.shape[1], p[7:16], p[16:25])
    for m in (mx, my):
        a = m.astype(np.float64) * 32
        assert (np.abs(a - np.floor(a) - 0.5) == 0).all()


def test_sigma_0_is_an_identity():
    for c in A.CASES:
        if c.sigma == 0.0 and not c.ties:
            r = A.reference(c.name)
            assert np.array_equal(r["x64"], np.transpose(r["img"], (3, 0, 1, 2)).astype(np.float64)), c.name
            assert np.array_equal(r["x32"], np.transpose(r["img"], (3, 0, 1, 2))), c.name
            assert np.array_equal(r["y64"], r["lbl"]) and np.array_equal(r["y32"], r["lbl"]), c.name


def _safe(r):
    """voxels of a case that a comparison keeps: all of a ramp case, else those whose two margins reach MARGIN"""
    if r["case"].ramp:
        return np.ones(r["lmargin"].shape, bool), np.ones(r["imargin"].shape, bool)
    return r["lmargin"] >= A.MARGIN, r["imargin"] >= A.MARGIN


def test_excluded_share_stays_under_its_cap():
    for c in A.CASES:
        r = A.reference(c.name)
        ls, is_ = _safe(r)
        assert 1 - ls.mean() <= A.EXCLUDED_CAP and 1 - is_.mean() <= A.EXCLUDED_CAP, (c.name, 1 - ls.mean(), 1 - is_.mean())


@pytest.mark.parametrize("defect", sorted(A.DEFECTS))
def test_every_defect_changes_what_some_case_expects(defect):
    hit = []
    for c in A.CASES:
        r = A.reference(c.name)
        x, y, _, _ = A.augment3d(r["img"], r["lbl"], r["prm"], c.crop, np.float64, defects=(defect,))
        ls, is_ = _safe(r)
        gate = A.ramp_gate(r["img"]) if c.ramp else 1e-3
        if (np.abs(x - r["x64"]).max(axis=0)[is_] > gate).any() or (y != r["y64"])[ls].any():
            hit.append(c.name)
    print(defect, "->", hit)
    assert hit, f"no case notices: {A.DEFECTS[defect]}"


def test_fp32_restatement_is_close_to_the_yardstick():
    for c in A.CASES:
        r = A.reference(c.name)
        ls, is_ = _safe(r)
        err = float(np.abs(r["x32"].astype(np.float64) - r["x64"]).max(axis=0)[is_].max())
        assert err <= 1e-4 * max(1.0, float(np.abs(r["x64"]).max())), (c.name, err)
        assert not (r["y32"] != r["y64"])[ls].any(), c.name


# ================================================================================================ host-side draws
class _Cfg:
    NN_AUGMENTATION, SOFT_AUGMENTATION, TRAIN_ORIGINAL_CLASSES = True, False, False
    DO_ROTATE, ROT_DEGREES, DO_SCALE, SCALE_FACTOR, DO_FLIP = True, 20, True, 1.1, True
    DO_ELASTIC_AUG, SIGMA, DO_INTENSITY_SHIFT, MAX_INTENSITY_SHIFT = True, 10, True, 0.1


def _replay(shape, cfg, crop, augment=True):
    """augment3DImage's calls to numpy's RNG (augmentation.py:45,52,69,73,84,89) and bratsDataset.py:82-84's to Python's, written out"""
    X, Y, Z = shape
    d = {}
    if augment:
        if cfg.DO_ROTATE:
            d["angle"] = np.random.uniform(-cfg.ROT_DEGREES, cfg.ROT_DEGREES)
        if cfg.DO_SCALE:
            d["scale"] = np.random.uniform(1 / cfg.SCALE_FACTOR, 1 * cfg.SCALE_FACTOR)
        if cfg.DO_ELASTIC_AUG:
            d["dx"] = np.random.normal(0, cfg.SIGMA, 9)
            d["dy"] = np.random.normal(0, cfg.SIGMA, 9)
        if cfg.DO_INTENSITY_SHIFT:
            d["shift"] = [np.random.uniform(-cfg.MAX_INTENSITY_SHIFT, cfg.MAX_INTENSITY_SHIFT) for _ in range(4)]
        if cfg.DO_FLIP:
            d["flips"] = sum(1 << i for i in range(3) if np.random.random() < 0.5)
    if crop is not None:
        x = random.randint(0, X - crop[0])
        y = random.randint(0, Y - crop[1])
        z = random.randint(0, Z - crop[2])
        d["origin"] = (x, y, z)
    return d


@pytest.mark.parametrize("off", [(), ("DO_ROTATE",), ("DO_SCALE", "DO_FLIP"), ("DO_ELASTIC_AUG",), ("DO_INTENSITY_SHIFT", "DO_ROTATE"),
                                 ("DO_ROTATE", "DO_SCALE", "DO_ELASTIC_AUG", "DO_INTENSITY_SHIFT", "DO_FLIP")])
@pytest.mark.parametrize("crop,augment", [((8, 16, 4), True), (None, True), ((8, 16, 4), False)])
def test_draws_consume_both_streams_as_the_reference_does(off, crop, augment):
    from unet_zoo_amd.data.brats_dataset import draw_augmentation3d
    cfg = type("Cfg", (_Cfg,), {k: False for k in off})
    shape = (16, 24, 8)
    np.random.seed(5); random.seed(7)
    want = [_replay(shape, cfg, crop, augment) for _ in range(3)]
    np_after, py_after = np.random.uniform(), random.random()
    np.random.seed(5); random.seed(7)
    got = [draw_augmentation3d(shape, cfg, crop, augment) for _ in range(3)]
    assert (np.random.uniform(), random.random()) == (np_after, py_after), "the streams are not where the reference leaves them"
    for d, p in zip(want, got):
        ref = A.make_prm(shape, d.get("angle"), d.get("scale"), d.get("dx"), d.get("dy"), d.get("shift"), d.get("flips", 0), d.get("origin", (0, 0, 0)))
        assert p.dtype == np.float64 and p.shape == (A.NPRM,) and np.array_equal(p, ref)
    # a mapping serves as expConfig too
    np.random.seed(5); random.seed(7)
    as_map = {k: getattr(cfg, k) for k in dir(cfg) if k.isupper()}
    assert np.array_equal(draw_augmentation3d(shape, as_map, crop, augment), got[0])


def test_dataset_reads_the_reference_config_and_refuses_what_is_not_built():
    from unet_zoo_amd.data.brats_dataset import BratsDataset
    rs = np.random.RandomState(0)
    data = dict(images_train=rs.standard_normal((2, 8, 8, 4, 4)).astype(np.float32), masks_train=np.zeros((2, 8, 8, 4), np.uint8), pids_train=np.array([11, 12]))
    ds = BratsDataset(data, _Cfg, randomCrop=(4, 4, 4), device="cpu")
    assert len(ds) == 2
    np.random.seed(1); random.seed(1)
    p = ds.draw((8, 8, 4))
    assert p[0] == 1 and p[3] == 1 and p[6] == 1 and p[25] == 1 and 0 <= p[31] <= 4 and p[33] == 0
    with pytest.raises(Exception, match="no GPU visible"):
        ds[0]
    soft = type("Soft", (_Cfg,), dict(NN_AUGMENTATION=False))
    with pytest.raises(NotImplementedError, match="NN_AUGMENTATION"):
        BratsDataset(data, soft)
    with pytest.raises(AttributeError):
        BratsDataset(data, type("Bare", (), dict(NN_AUGMENTATION=True, SOFT_AUGMENTATION=False, TRAIN_ORIGINAL_CLASSES=False)))


# ================================================================================================ route and refusals
def test_route_claims():
    L, _ = _lib()
    out = (C.c_int * 2)()
    for (C_, X, Y, Z), al, want in [((4, 16, 24, 8), 16, 1), ((4, 16, 24, 8), 4, 0), ((4, 16, 24, 8), 8, 0), ((3, 16, 24, 8), 16, 0),
                                    ((1, 8, 8, 4), 16, 0), ((8, 24, 16, 5), 16, 0), ((4, 240, 240, 155), 16, 1)]:
        assert L.uz_augment_volume_route(C_, X, Y, Z, al, out) == 0
        assert tuple(out) == (want, -(-X * Y * Z // 256)), (C_, X, Y, Z, al, tuple(out))
    assert L.uz_augment_volume_route(0, 8, 8, 4, 16, out) != 0 and L.uz_augment_volume_route(9, 8, 8, 4, 16, out) != 0
    assert L.uz_augment_volume_route(4, 0, 8, 4, 16, out) != 0 and L.uz_augment_volume_route(4, 8, 8, 4, 3, out) != 0
    assert L.uz_augment_volume_route(4, 8, 8, 4, 16, None) != 0
    assert L.uz_augment_volume_route(4, 2048, 2048, 128, 16, out) != 0                     # 2^31 elements
    assert L.uz_augment_volume_workspace(4, 8, 8, 4) >= 2 * 4 * 256 * 4 + 2 * 256 + 2 * 64 * 4
    assert L.uz_augment_volume_workspace(9, 8, 8, 4) == 0


def test_refusals_name_their_reason():
    """Refused before any launch: the pointers are host memory that is never read (prm excepted, a host table by contract)."""
    L, _ = _lib()
    host = np.zeros(4096, np.float32)
    ptr = host.ctypes.data
    assert ptr % 16 == 0
    good = A.make_prm((8, 8, 4))

    def call(C_=4, shape=(8, 8, 4), prm=good, crop=(8, 8, 4), img=ptr, lbl=ptr, ws=ptr, x=ptr, ye=ptr, yr=ptr):
        rc = L.uz_augment_volume(img, lbl, C_, *shape, None if prm is None else prm.ctypes.data, *crop, ws, x, ye, yr, None)
        return rc, L.uz_last_error().decode()

    def prm(**kw):
        return A.make_prm((8, 8, 4), **kw)
    nan = good.copy(); nan[7] = np.nan
    flips8 = good.copy(); flips8[30] = 8
    tiny = prm(scale=1.0); tiny[4] = 0
    for kw, reason in [(dict(img=None), "null"), (dict(prm=None), "null"), (dict(ws=None), "null"), (dict(x=None), "null"),
                       (dict(lbl=None), "label outputs without a label"), (dict(lbl=None, ye=None), "label outputs without a label"),
                       (dict(C_=0), "1 <= C <= 8"), (dict(C_=9), "1 <= C <= 8"), (dict(shape=(8, 0, 4)), "empty"),
                       (dict(shape=(2048, 2048, 128), crop=(8, 8, 4)), "int32"), (dict(ws=ptr + 4), "16-byte"),
                       (dict(crop=(9, 8, 4)), "leaves the volume"), (dict(crop=(0, 8, 4)), "leaves the volume"),
                       (dict(prm=prm(origin=(1, 0, 0))), "leaves the volume"), (dict(prm=prm(origin=(0, 0, -1))), "leaves the volume"),
                       (dict(crop=(4, 4, 2), prm=prm(origin=(4, 4, 3))), "leaves the volume"),
                       (dict(C_=3, prm=prm(shift=[0.1] * 4)), "channels 0..3"), (dict(prm=nan), "finite"), (dict(prm=flips8), "flips"),
                       (dict(prm=tiny), "scaled size")]:
        rc, msg = call(**kw)
        assert rc != 0 and reason in msg, (kw.keys(), rc, msg)
    assert not host.any()
