"""18- / 26-connectivity, relabelling and hole filling on the device: uz_vol_label_components_ex, uz_vol_keep_components_ex and
uz_vol_fill_holes (csrc/volcomp.hip) through ctypes on the cases of tests/_morph.py against the numpy / scipy twin, then the three
Python functions.  The kernels read no arithmetic mode (everything is an integer); only the end-to-end test runs a network.  Gates:
equality - labels and sizes integer for integer, the filtered and the filled volumes byte for byte, no tolerance anywhere; the _ex
calls at connectivity 1 without relabel byte for byte the old calls; a second call bit-equal; the input untouched; every output and the
workspace between canaries."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _components as K
from tests import _morph as M

pytestmark = pytest.mark.gpu


def _g():
    from tests import _gpu
    return _gpu


def _workspace(g, shape):
    nbytes = g.L().uz_vol_components_workspace(*shape)
    assert nbytes > 0
    raw, ws = g.guarded(nbytes, torch.uint8, 256)
    assert ws.data_ptr() % 16 == 0
    return raw, ws


def _arr(t, values):
    return (t * len(values))(*values)


def _label(g, vol, values, conn, want_sizes=True, old=False):
    """One uz_vol_label_components_ex call (old: uz_vol_label_components), outputs and workspace between canaries -> (labels, sizes or None)"""
    dev, L = g.dev(), g.L()
    v = torch.from_numpy(np.array(vol)).to(dev)
    before = v.clone()
    T = vol.size
    ws_raw, ws = _workspace(g, vol.shape)
    lab_raw, lab = g.guarded(T, torch.int32)
    sz_raw, sz = g.guarded(T, torch.int32)
    tail = (lab.data_ptr(), sz.data_ptr() if want_sizes else None, ws.data_ptr(), g.stream())
    if old:
        rc = L.uz_vol_label_components(v.data_ptr(), *vol.shape, K.region_bits(values), *tail)
    else:
        rc = L.uz_vol_label_components_ex(v.data_ptr(), *vol.shape, K.region_bits(values), conn, *tail)
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(ws_raw, ws) and g.intact(lab_raw, lab) and g.intact(sz_raw, sz) and torch.equal(v, before)
    if not want_sizes:
        assert bool((sz == g.CANARY[torch.int32]).all())
    return lab.cpu().numpy().reshape(vol.shape), sz.cpu().numpy().reshape(vol.shape) if want_sizes else None


def _keep(g, vol, regions, mv, unlisted, conn, relabel, old=False):
    dev, L = g.dev(), g.L()
    v = torch.from_numpy(np.array(vol)).to(dev)
    before = v.clone()
    T, R = vol.size, len(regions)
    ws_raw, ws = _workspace(g, vol.shape)
    out_raw, out = g.guarded(T, torch.uint8)
    sets, mins = _arr(C.c_uint32, [K.region_bits(r) for r in regions]), _arr(C.c_int32, K.min_voxels_list(mv, R))
    rl = _arr(C.c_int32, [-1] * R if relabel is None else [-1 if x is None else x for x in relabel])
    tail = (int(unlisted == "keep"), out.data_ptr(), ws.data_ptr(), g.stream())
    if old:
        rc = L.uz_vol_keep_components(v.data_ptr(), *vol.shape, sets, mins, R, *tail)
    else:
        rc = L.uz_vol_keep_components_ex(v.data_ptr(), *vol.shape, sets, mins, rl, R, conn, *tail)
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(ws_raw, ws) and g.intact(out_raw, out) and torch.equal(v, before)
    return out.cpu().numpy().reshape(vol.shape)


def _fill(g, vol, regions, fv, mx, conn):
    dev, L = g.dev(), g.L()
    v = torch.from_numpy(np.array(vol)).to(dev)
    before = v.clone()
    T, R = vol.size, len(regions)
    ws_raw, ws = _workspace(g, vol.shape)
    out_raw, out = g.guarded(T, torch.uint8)
    sets = _arr(C.c_uint32, [K.region_bits(r) for r in regions])
    fills = _arr(C.c_int32, [int(tuple(r)[0]) for r in regions] if fv is None else M._per_region(fv, R))
    rc = L.uz_vol_fill_holes(v.data_ptr(), *vol.shape, sets, fills, _arr(C.c_int32, M._per_region(mx, R)), R, conn, out.data_ptr(), ws.data_ptr(), g.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(ws_raw, ws) and g.intact(out_raw, out) and torch.equal(v, before)
    return out.cpu().numpy().reshape(vol.shape)


# ================================================================================================ the C entry points
@pytest.mark.parametrize("name", M.NAMES)
def test_labels_and_sizes_of_every_case_at_every_connectivity(name):
    g = _g()
    c = M.case(name)
    for conn in M.CONN:
        want_l, want_s = M.expected_components(name, conn)
        lab, sz = _label(g, c.vol, c.values, conn)
        print(name, c.vol.shape, "c", conn, "components", len(np.unique(want_l)) - 1, "label mismatches", int((lab != want_l).sum()), "size mismatches", int((sz != want_s).sum()))
        assert lab.dtype == np.int32 and np.array_equal(lab, want_l), (name, conn)
        assert np.array_equal(sz, want_s), (name, conn)
        lab2, sz2 = _label(g, c.vol, c.values, conn)                     # a second call is bit-equal
        assert lab2.tobytes() == lab.tobytes() and sz2.tobytes() == sz.tobytes()
        lab0, none = _label(g, c.vol, c.values, conn, want_sizes=False)  # sizes = NULL is accepted and changes nothing
        assert none is None and lab0.tobytes() == lab.tobytes()
        if conn == 1:                                                    # byte for byte the old call
            labo, szo = _label(g, c.vol, c.values, 1, old=True)
            assert labo.tobytes() == lab.tobytes() and szo.tobytes() == sz.tobytes()


@pytest.mark.parametrize("name,k", M.KEEP_IDS, ids=["%s-%d" % i for i in M.KEEP_IDS])
def test_keep_and_relabel_of_every_case_at_every_connectivity(name, k):
    g = _g()
    c = M.case(name)
    regions, mv, unl, rl = c.keeps[k]
    for conn in M.CONN:
        want = M.expected_keep(name, k, conn)
        out = _keep(g, c.vol, regions, mv, unl, conn, rl)
        print(name, k, regions, mv, unl, rl, "c", conn, "voxels changed", int((out != c.vol).sum()), "mismatches", int((out != want).sum()))
        assert out.dtype == np.uint8 and out.tobytes() == want.tobytes(), (name, k, conn)
        assert _keep(g, c.vol, regions, mv, unl, conn, rl).tobytes() == out.tobytes()
        if conn == 1 and rl is None:
            assert _keep(g, c.vol, regions, mv, unl, 1, None, old=True).tobytes() == out.tobytes()


OLD_KEEP_IDS = [(c.name, k) for c in K.cases() for k in range(len(c.params))]


@pytest.mark.parametrize("name,k", OLD_KEEP_IDS, ids=["%s-%d" % i for i in OLD_KEEP_IDS])
def test_keep_ex_at_connectivity_1_without_relabel_is_the_old_call(name, k):
    g = _g()
    c = K.case(name)
    regions, mv, unl = c.params[k]
    old = _keep(g, c.vol, regions, mv, unl, 1, None, old=True)
    assert old.tobytes() == K.expected_keep(name, k).tobytes()
    assert _keep(g, c.vol, regions, mv, unl, 1, None).tobytes() == old.tobytes()
    assert _keep(g, c.vol, regions, mv, unl, 1, [None] * len(regions)).tobytes() == old.tobytes()


@pytest.mark.parametrize("name,k", M.FILL_IDS, ids=["%s-%d" % i for i in M.FILL_IDS])
def test_fill_of_every_case_at_every_connectivity(name, k):
    g = _g()
    c = M.case(name)
    regions, fv, mx = c.fills[k]
    for conn in M.CONN:
        want = M.expected_fill(name, k, conn)
        out = _fill(g, c.vol, regions, fv, mx, conn)
        print(name, k, regions, fv, mx, "c", conn, "voxels filled", int((out != c.vol).sum()), "mismatches", int((out != want).sum()))
        assert out.dtype == np.uint8 and out.tobytes() == want.tobytes(), (name, k, conn)
        assert _fill(g, c.vol, regions, fv, mx, conn).tobytes() == out.tobytes()


def test_eight_sets_and_a_second_stream():
    """R = 8, the cap, with repeated sets: every set, relabel and fill value is read; and the calls on a side stream, bit-equal"""
    g = _g()
    blobs = K.case("blobs").vol
    regs8 = K.NESTED * 2 + K.PER_LABEL[:2]
    rl8 = (None, 9, None, 0, 255, 1, None, 3)
    mv8 = (0, 30, 2, 0, 40, 3, 0, 5)
    for conn in (1, 3):
        assert _keep(g, blobs, regs8, mv8, "keep", conn, rl8).tobytes() == M.keep(blobs, regs8, mv8, "keep", conn, rl8).tobytes()
    sponge = M.case("dense").vol
    regs8 = ((1,), (0, 1), (1, 2), (1,), (1, 3), (0,), (1,), (1, 5))
    fv8, mx8 = (1, 0, 2, 1, 3, 0, 1, 5), (0, 3, 1, 2, 0, 4, 1, 1)
    want = M.fill(sponge, regs8, fv8, mx8, 2)
    assert len(np.unique(want)) == 4 and _fill(g, sponge, regs8, fv8, mx8, 2).tobytes() == want.tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # g.stream() is the current stream: the side stream here
        a = _fill(g, sponge, regs8, fv8, mx8, 2)
        b = _keep(g, blobs, K.NESTED, (0, 30, 2), "zero", 3, (None, 1, 2))
        lab, sz = _label(g, blobs, (1, 2, 3), 2)
    torch.cuda.current_stream().wait_stream(side)
    assert a.tobytes() == want.tobytes() and b.tobytes() == M.keep(blobs, K.NESTED, (0, 30, 2), "zero", 3, (None, 1, 2)).tobytes()
    want_l, want_s = M.components(K.in_set(blobs, (1, 2, 3)), 2)
    assert np.array_equal(lab, want_l) and np.array_equal(sz, want_s)


def test_a_refused_call_leaves_the_outputs_untouched():
    g = _g()
    dev, L = g.dev(), g.L()
    c = K.case("tie")
    v = torch.from_numpy(np.array(c.vol)).to(dev)
    T = c.vol.size
    ws = torch.full((L.uz_vol_components_workspace(*c.vol.shape) + 16,), 0xA5, dtype=torch.uint8, device=dev)
    lab = torch.full((T,), -7777, dtype=torch.int32, device=dev)
    out = torch.full((T,), 0xA5, dtype=torch.uint8, device=dev)
    sets, zeros, neg = _arr(C.c_uint32, [2] * 9), _arr(C.c_int32, [0] * 9), _arr(C.c_int32, [-1] + [0] * 8)
    ones, twos, big = _arr(C.c_int32, [1] * 9), _arr(C.c_int32, [2] * 9), _arr(C.c_int32, [256] + [0] * 8)
    base = dict(N=1, R=1, shape=c.vol.shape[1:], ws=ws.data_ptr(), out=out.data_ptr(), conn=2)
    for kw in (dict(N=0), dict(R=0), dict(R=9), dict(shape=(2, 0, 10)), dict(ws=ws.data_ptr() + 8), dict(ws=None), dict(out=None), dict(mins=neg), dict(out=v.data_ptr() + 1),
               dict(conn=0), dict(conn=4), dict(rl=_arr(C.c_int32, [-2] * 9)), dict(rl=big), dict(rl=None)):
        a = dict(base, mins=zeros, rl=neg)
        a.update(kw)
        rc = L.uz_vol_keep_components_ex(v.data_ptr(), a["N"], *a["shape"], sets, a["mins"], a["rl"], a["R"], a["conn"], 0, a["out"], a["ws"], g.stream())
        assert rc != 0 and L.uz_last_error().decode().startswith("vol_keep_components_ex:"), kw
    for kw in (dict(N=0), dict(R=0), dict(R=9), dict(shape=(2, 6, 0)), dict(ws=ws.data_ptr() + 8), dict(ws=None), dict(out=None), dict(mx=neg), dict(out=v.data_ptr() + 1),
               dict(conn=0), dict(conn=4), dict(fv=twos), dict(fv=neg), dict(fv=None)):
        a = dict(base, fv=ones, mx=zeros)
        a.update(kw)
        rc = L.uz_vol_fill_holes(v.data_ptr(), a["N"], *a["shape"], sets, a["fv"], a["mx"], a["R"], a["conn"], a["out"], a["ws"], g.stream())
        assert rc != 0 and L.uz_last_error().decode().startswith("vol_fill_holes:"), kw
    for kw in (dict(N=0), dict(shape=(2, 6, 0)), dict(ws=ws.data_ptr() + 4), dict(lab=None), dict(lab=lab.data_ptr() + 2), dict(conn=0), dict(conn=4)):
        a = dict(N=1, shape=c.vol.shape[1:], ws=ws.data_ptr(), lab=lab.data_ptr(), conn=3)
        a.update(kw)
        rc = L.uz_vol_label_components_ex(v.data_ptr(), a["N"], *a["shape"], 2, a["conn"], a["lab"], None, a["ws"], g.stream())
        assert rc != 0 and L.uz_last_error().decode().startswith("vol_label_components_ex:"), kw
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((lab == -7777).all()) and bool((out == 0xA5).all()) and torch.equal(v.cpu(), torch.from_numpy(np.array(c.vol)))


# ================================================================================================ the Python functions
def test_python_functions_on_tensors_and_a_misaligned_sliced_view():
    from unet_zoo_amd import metrics
    g = _g()
    dev = g.dev()
    blobs = K.case("blobs").vol
    big = torch.zeros(2, 12, 20, 71, dtype=torch.uint8, device=dev)
    big[..., 1:] = torch.from_numpy(np.array(blobs)).to(dev)
    view = big[..., 1:]                                                  # neither contiguous nor aligned: the functions make it dense
    assert not view.is_contiguous() and view.data_ptr() % 4 == 1
    for conn in (2, 3):
        for _ in range(2):                                               # the second call takes the cached workspace
            lab, sz = metrics.label_components(view, (1, 2, 3), return_sizes=True, connectivity=conn)
            want_l, want_s = M.components(K.in_set(blobs, (1, 2, 3)), conn)
            assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), want_l) and np.array_equal(sz.cpu().numpy(), want_s)
        out = metrics.keep_largest_components(view, K.NESTED, min_voxels=(0, 30, 2), connectivity=conn, relabel=(None, 1, 2))
        assert out.cpu().numpy().tobytes() == M.keep(blobs, K.NESTED, (0, 30, 2), "zero", conn, (None, 1, 2)).tobytes()
    assert metrics.keep_largest_components(view, K.NESTED).cpu().numpy().tobytes() == K.expected_keep("blobs", 0).tobytes()
    # the BraTS rule: a small enhancing component becomes necrosis and stays inside the whole tumour
    out = metrics.keep_largest_components(view, regions=((3,),), min_voxels=20, relabel=(1,), unlisted="keep")
    want = M.keep(blobs, ((3,),), 20, "keep", 1, (1,))
    assert out.cpu().numpy().tobytes() == want.tobytes() and (want != blobs).any() and np.array_equal(K.in_set(want, (1, 2, 3)), K.in_set(blobs, (1, 2, 3)))
    sponge = M.case("dense").vol
    t = torch.from_numpy(np.array(sponge)).to(dev)
    for conn in M.CONN:
        got = metrics.fill_holes(t, ((1,),), connectivity=conn)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == M.expected_fill("dense", 0, conn).tobytes()
    assert metrics.fill_holes(t, ((1,),), max_voxels=1).cpu().numpy().tobytes() == M.expected_fill("dense", 1, 1).tobytes()
    got = metrics.fill_holes(view, K.NESTED, fill=(1, 3, 3), max_voxels=(0, 6, 2), connectivity=2)
    assert got.cpu().numpy().tobytes() == M.fill(blobs, K.NESTED, (1, 3, 3), (0, 6, 2), 2).tobytes()
    assert torch.equal(t.cpu(), torch.from_numpy(np.array(sponge))) and torch.equal(view.cpu(), torch.from_numpy(np.array(blobs)))


def test_predict_keep_fill_score_end_to_end():
    """PHISeg3D.predict -> keep_largest_components(connectivity, relabel) -> fill_holes -> score_volume, and the same on a 2-D Prediction"""
    import oracle
    from tests import _golden as G
    from tests import _nets as N
    from unet_zoo_amd import metrics
    from unet_zoo_amd.models.phiseg import Prediction
    g = _g()
    dev = g.dev()
    arrays, meta = G.load("phiseg3d_small")
    net = N.small_phiseg3d(meta, oracle.deterministic_state_dict(G.spec_of(meta), seed=91))
    torch.manual_seed(5)
    with torch.no_grad():
        pred = net.predict(torch.from_numpy(arrays["patch"]).to(dev), n_samples=4)
    torch.cuda.synchronize()
    nc = int(meta["num_classes"])
    regs = tuple(tuple(range(k, nc)) for k in range(1, nc))              # nested regions of class indices
    rows = torch.cat([pred.labels[:, 0], pred.mean_label], 0).cpu().numpy()
    assert rows.dtype == np.uint8 and rows.shape[0] == 5
    rl = (None,) + tuple(k for k in range(1, nc - 1))                    # a small component of an inner region falls back to the class around it
    mv = (0,) + (4,) * (nc - 2)
    kept = metrics.keep_largest_components(pred, regs, min_voxels=mv, connectivity=3, relabel=rl)
    want_kept = M.keep(rows, regs, mv, "zero", 3, rl)
    assert type(kept) is type(pred) and kept.labels.shape == pred.labels.shape and kept.soft is pred.soft and kept.entropy is pred.entropy
    assert torch.cat([kept.labels[:, 0], kept.mean_label], 0).cpu().numpy().tobytes() == want_kept.tobytes()
    filled = metrics.fill_holes(kept, regs, connectivity=1)
    want = M.fill(want_kept, regs, None, None, 1)
    assert type(filled) is type(pred) and filled.labels.shape == pred.labels.shape and filled.mean_label.shape == pred.mean_label.shape and filled.soft is pred.soft
    assert torch.cat([filled.labels[:, 0], filled.mean_label], 0).cpu().numpy().tobytes() == want.tobytes()
    ref = np.roll(rows[1], 1, axis=2)
    sc = metrics.score_volume(filled, torch.from_numpy(ref.copy()).to(dev), regs, hd95=True)
    counts = sc.counts.cpu().numpy()
    for n in range(5):
        for r, reg in enumerate(regs):
            a, b = K.in_set(want[n], reg), K.in_set(ref, reg)
            assert tuple(int(x) for x in counts[n, r]) == (int((a & b).sum()), int(a.sum()), int(b.sum()), a.size), (n, reg)
    assert np.array_equal(torch.cat([pred.labels[:, 0], pred.mean_label], 0).cpu().numpy(), rows)         # the draw itself is untouched
    # 2-D: S = 2 samples of B = 2 images and the two mean labels, run as volumes of depth 1: an image has holes
    ring = M.case("ring_d1").vol                                         # (2, 1, 14, 18)
    lab2 = np.stack([ring[:, 0], ring[::-1, 0]])                         # (S, B, H, W)
    mean2 = np.stack([ring[0, 0], np.maximum(ring[0, 0], ring[1, 0])])   # (B, H, W)
    p2 = Prediction(labels=torch.from_numpy(lab2.copy()).to(dev), mean_soft=None, mean_label=torch.from_numpy(mean2.copy()).to(dev), entropy=None, levels=None)
    q2 = metrics.fill_holes(p2, ((1,),), max_voxels=100)
    want2 = M.fill(np.concatenate([lab2.reshape(4, 1, 14, 18), mean2.reshape(2, 1, 14, 18)], 0), ((1,),), None, 100)
    assert q2.labels.shape == (2, 2, 14, 18) and q2.mean_label.shape == (2, 14, 18)
    assert torch.cat([q2.labels.reshape(4, 14, 18), q2.mean_label], 0).cpu().numpy().tobytes() == want2.reshape(6, 14, 18).tobytes()
    assert int((want2 != 0).sum()) > int((lab2 != 0).sum()) + int((mean2 != 0).sum())                     # something was filled
