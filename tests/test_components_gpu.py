"""Volume components on the device: uz_vol_label_components and uz_vol_keep_components (csrc/volcomp.hip) through ctypes on the cases of
tests/_components.py against the numpy / scipy twin, then metrics.label_components and metrics.keep_largest_components.  The kernels
read no arithmetic mode (everything is an integer), so one mode suffices.  Gates: equality - labels and sizes integer for integer,
the filtered volumes byte for byte, no tolerance and no exempt share; a second call bit-equal; the input untouched; every output and
the workspace between canaries."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _components as K

pytestmark = pytest.mark.gpu

KEEP_IDS = [(c.name, k) for c in K.cases() for k in range(len(c.params))]


def _g():
    from tests import _gpu
    return _gpu


def _workspace(g, shape):
    nbytes = g.L().uz_vol_components_workspace(*shape)
    assert nbytes > 0
    raw, ws = g.guarded(nbytes, torch.uint8, 256)
    assert ws.data_ptr() % 16 == 0
    return raw, ws


def _label(g, vol, values, want_sizes=True):
    """One uz_vol_label_components call, outputs and workspace between canaries -> (labels, sizes or None) numpy"""
    dev, L = g.dev(), g.L()
    v = torch.from_numpy(np.array(vol)).to(dev)
    before = v.clone()
    T = vol.size
    ws_raw, ws = _workspace(g, vol.shape)
    lab_raw, lab = g.guarded(T, torch.int32)
    sz_raw, sz = g.guarded(T, torch.int32)
    rc = L.uz_vol_label_components(v.data_ptr(), *vol.shape, K.region_bits(values), lab.data_ptr(), sz.data_ptr() if want_sizes else None,
                                   ws.data_ptr(), g.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(ws_raw, ws) and g.intact(lab_raw, lab) and g.intact(sz_raw, sz) and torch.equal(v, before)
    if not want_sizes:
        assert bool((sz == g.CANARY[torch.int32]).all())
    return lab.cpu().numpy().reshape(vol.shape), sz.cpu().numpy().reshape(vol.shape) if want_sizes else None


def _keep(g, vol, regions, mv, unlisted):
    """One uz_vol_keep_components call, output and workspace between canaries -> out numpy"""
    dev, L = g.dev(), g.L()
    v = torch.from_numpy(np.array(vol)).to(dev)
    before = v.clone()
    T, R = vol.size, len(regions)
    ws_raw, ws = _workspace(g, vol.shape)
    out_raw, out = g.guarded(T, torch.uint8)
    sets = (C.c_uint32 * R)(*[K.region_bits(r) for r in regions])
    mins = (C.c_int32 * R)(*K.min_voxels_list(mv, R))
    rc = L.uz_vol_keep_components(v.data_ptr(), *vol.shape, sets, mins, R, int(unlisted == "keep"), out.data_ptr(), ws.data_ptr(), g.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(ws_raw, ws) and g.intact(out_raw, out) and torch.equal(v, before)                # vol untouched
    return out.cpu().numpy().reshape(vol.shape)


# ================================================================================================ the C entry points
@pytest.mark.parametrize("name", K.NAMES)
def test_labels_and_sizes_of_every_case(name):
    g = _g()
    c = K.case(name)
    want_l, want_s = K.expected_components(name)
    lab, sz = _label(g, c.vol, c.values)
    print(name, c.vol.shape, "components", len(np.unique(want_l)) - 1, "label mismatches", int((lab != want_l).sum()), "size mismatches", int((sz != want_s).sum()))
    assert lab.dtype == np.int32 and np.array_equal(lab, want_l), name
    assert np.array_equal(sz, want_s), name
    lab2, sz2 = _label(g, c.vol, c.values)                               # a second call is bit-equal
    assert lab2.tobytes() == lab.tobytes() and sz2.tobytes() == sz.tobytes()
    lab0, none = _label(g, c.vol, c.values, want_sizes=False)            # sizes = NULL is accepted and changes nothing
    assert none is None and lab0.tobytes() == lab.tobytes()


@pytest.mark.parametrize("name,k", KEEP_IDS, ids=["%s-%d" % i for i in KEEP_IDS])
def test_keep_of_every_case_and_parameter_set(name, k):
    g = _g()
    c = K.case(name)
    regions, mv, unl = c.params[k]
    want = K.expected_keep(name, k)
    out = _keep(g, c.vol, regions, mv, unl)
    print(name, k, regions, mv, unl, "voxels kept", int((out != 0).sum()), "of", int((c.vol != 0).sum()), "mismatches", int((out != want).sum()))
    assert out.dtype == np.uint8 and out.tobytes() == want.tobytes(), (name, k)
    assert _keep(g, c.vol, regions, mv, unl).tobytes() == out.tobytes()  # a second call is bit-equal


def test_eight_sets_and_a_set_with_label_zero():
    """R = 8, the cap, with repeated sets: every set is read; and a set that holds the value 0 labels the background"""
    g = _g()
    c = K.case("blobs")
    regs8 = K.NESTED * 2 + K.PER_LABEL[:2]
    assert _keep(g, c.vol, regs8, None, "zero").tobytes() == K.keep(c.vol, regs8).tobytes()
    v = K.case("flat").vol
    lab, sz = _label(g, v, (0,))
    want_l, want_s = K.components(K.in_set(v, (0,)))
    assert np.array_equal(lab, want_l) and np.array_equal(sz, want_s)
    # the highest value a set can hold: bit 31 of the mask travels through the binding
    v31 = (np.array(v) == 2).astype(np.uint8) * 31
    lab, sz = _label(g, v31, (31,))
    want_l, want_s = K.components(v31 == 31)
    assert want_l.any() and np.array_equal(lab, want_l) and np.array_equal(sz, want_s)
    assert _keep(g, v31, ((31,), (0, 31)), (0, 2), "zero").tobytes() == K.keep(v31, ((31,), (0, 31)), (0, 2)).tobytes()


def test_a_refused_call_leaves_the_outputs_untouched():
    g = _g()
    dev, L = g.dev(), g.L()
    c = K.case("tie")
    v = torch.from_numpy(np.array(c.vol)).to(dev)
    T = c.vol.size
    ws = torch.full((L.uz_vol_components_workspace(*c.vol.shape) + 16,), 0xA5, dtype=torch.uint8, device=dev)
    lab = torch.full((T,), -7777, dtype=torch.int32, device=dev)
    out = torch.full((T,), 0xA5, dtype=torch.uint8, device=dev)
    sets, mins, neg = (C.c_uint32 * 9)(*[2] * 9), (C.c_int32 * 9)(*[0] * 9), (C.c_int32 * 9)(*[-1] + [0] * 8)
    for kw in (dict(N=0), dict(R=0), dict(R=9), dict(shape=(2, 0, 10)), dict(ws=ws.data_ptr() + 8), dict(ws=None), dict(out=None), dict(mins=neg), dict(out=v.data_ptr() + 1)):
        a = dict(N=1, R=1, shape=c.vol.shape[1:], ws=ws.data_ptr(), out=out.data_ptr(), mins=mins)
        a.update(kw)
        rc = L.uz_vol_keep_components(v.data_ptr(), a["N"], *a["shape"], sets, a["mins"], a["R"], 0, a["out"], a["ws"], g.stream())
        assert rc != 0 and L.uz_last_error().decode().startswith("vol_keep_components:"), kw
    for kw in (dict(N=0), dict(shape=(2, 6, 0)), dict(ws=ws.data_ptr() + 4), dict(lab=None), dict(lab=lab.data_ptr() + 2)):
        a = dict(N=1, shape=c.vol.shape[1:], ws=ws.data_ptr(), lab=lab.data_ptr())
        a.update(kw)
        rc = L.uz_vol_label_components(v.data_ptr(), a["N"], *a["shape"], 2, a["lab"], None, a["ws"], g.stream())
        assert rc != 0 and L.uz_last_error().decode().startswith("vol_label_components:"), kw
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((lab == -7777).all()) and bool((out == 0xA5).all()) and torch.equal(v.cpu(), torch.from_numpy(np.array(c.vol)))


# ================================================================================================ the Python functions
def test_label_components_with_and_without_sizes():
    from unet_zoo_amd import metrics
    g = _g()
    c = K.case("blobs")
    v = torch.from_numpy(np.array(c.vol)).to(g.dev())
    want_l, want_s = K.expected_components("blobs")
    for _ in range(2):                                                   # the second call takes the cached workspace
        lab = metrics.label_components(v, c.values)
        assert isinstance(lab, torch.Tensor) and lab.dtype == torch.int32 and lab.is_cuda and lab.shape == v.shape
        assert np.array_equal(lab.cpu().numpy(), want_l)
    lab, sz = metrics.label_components(v, c.values, return_sizes=True)
    assert np.array_equal(lab.cpu().numpy(), want_l) and sz.dtype == torch.int32 and np.array_equal(sz.cpu().numpy(), want_s)
    assert torch.equal(v.cpu(), torch.from_numpy(np.array(c.vol)))


def test_keep_largest_components_on_predictions_and_tensors_feeds_score_volume():
    from unet_zoo_amd import metrics
    from unet_zoo_amd.models.phiseg import Prediction
    g = _g()
    dev = g.dev()
    # 3-D: the two blob volumes as S = 2 samples, a third built from them as the mean label
    blobs = K.case("blobs").vol
    rows = np.concatenate([blobs, np.maximum(blobs[:1], blobs[1:])], 0)
    soft, mean_soft, entropy, levels = object(), object(), object(), object()
    p3 = Prediction(labels=torch.from_numpy(rows[:2].copy()).to(dev)[:, None], mean_soft=mean_soft, mean_label=torch.from_numpy(rows[2:].copy()).to(dev),
                    entropy=entropy, levels=levels, soft=soft)
    regions = ((1, 2, 3),)                                               # the largest whole tumour; 7 stays with unlisted="keep"
    for unl in ("zero", "keep"):
        want = K.keep(rows, regions, None, unl)
        q3 = metrics.keep_largest_components(p3, regions, unlisted=unl)
        assert type(q3) is Prediction and q3.labels.shape == p3.labels.shape and q3.mean_label.shape == p3.mean_label.shape and q3.labels.is_cuda
        assert q3.soft is soft and q3.mean_soft is mean_soft and q3.entropy is entropy and q3.levels is levels
        got = torch.cat([q3.labels[:, 0], q3.mean_label], 0).cpu().numpy()
        assert got.tobytes() == want.tobytes(), unl
        assert torch.equal(p3.labels.cpu()[:, 0], torch.from_numpy(rows[:2].copy()))                      # the draw itself is untouched
    # the filtered Prediction goes into score_volume unchanged: the counts are those of the twin's filtered volumes
    want = K.keep(rows, K.PER_LABEL)
    q3 = metrics.keep_largest_components(p3)
    ref = torch.from_numpy(blobs[0].copy()).to(dev)
    sc = metrics.score_volume(q3, ref, K.NESTED, hd95=False)
    counts = sc.counts.cpu().numpy()
    for n in range(3):
        for r, reg in enumerate(K.NESTED):
            a, b = K.in_set(want[n], reg), K.in_set(blobs[0], reg)
            assert tuple(int(x) for x in counts[n, r]) == (int((a & b).sum()), int(a.sum()), int(b.sum()), a.size), (n, reg)
    assert not np.array_equal(counts, metrics.score_volume(p3, ref, K.NESTED, hd95=False).counts.cpu().numpy())   # the filter changed what is scored
    # 2-D: S = 2 samples of B = 2 images and the two mean labels, run as volumes of depth 1
    flat = K.case("flat").vol                                            # (2, 1, 33, 67)
    lab2 = np.stack([flat[:, 0], flat[::-1, 0]])                         # (S, B, H, W)
    mean2 = np.maximum(flat[0], flat[1]).repeat(2, 0)                    # (B, H, W)
    p2 = Prediction(labels=torch.from_numpy(lab2.copy()).to(dev), mean_soft=mean_soft, mean_label=torch.from_numpy(mean2.copy()).to(dev), entropy=entropy, levels=levels)
    q2 = metrics.keep_largest_components(p2, K.NESTED, min_voxels=(0, 3, 1))
    want = K.keep(np.concatenate([lab2.reshape(4, 1, 33, 67), mean2.reshape(2, 1, 33, 67)], 0), K.NESTED, (0, 3, 1))
    assert q2.labels.shape == (2, 2, 33, 67) and q2.mean_label.shape == (2, 33, 67) and q2.soft is None and q2.levels is levels
    assert torch.cat([q2.labels.reshape(4, 33, 67), q2.mean_label], 0).cpu().numpy().tobytes() == want.tobytes()
    # a plain tensor, one threshold for every region
    perc = K.case("percolate").vol
    out = metrics.keep_largest_components(torch.from_numpy(np.array(perc)).to(dev), ((1,),), min_voxels=12)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.cpu().numpy().tobytes() == K.keep(perc, ((1,),), 12).tobytes()


def test_keep_on_a_misaligned_sliced_view():
    """a view that is neither contiguous nor aligned: the Python function makes it dense"""
    from unet_zoo_amd import metrics
    g = _g()
    blobs = K.case("blobs").vol
    big = torch.zeros(2, 12, 20, 71, dtype=torch.uint8, device=g.dev())
    big[..., 1:] = torch.from_numpy(np.array(blobs)).to(g.dev())
    view = big[..., 1:]
    assert not view.is_contiguous() and view.data_ptr() % 4 == 1
    out = metrics.keep_largest_components(view, K.NESTED)
    assert out.cpu().numpy().tobytes() == K.expected_keep("blobs", 0).tobytes()
    lab = metrics.label_components(view, (1, 2, 3))
    assert np.array_equal(lab.cpu().numpy(), K.expected_components("blobs")[0])
