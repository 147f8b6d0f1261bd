"""Binary morphology and lesion-wise scores on the device: uz_vol_morph (csrc/volmorph.hip) and uz_vol_lesion_scores
(csrc/vollesion.hip) through ctypes on the cases of tests/_lesions.py against the numpy / scipy twins, then the Python functions of
metrics.py.  The kernels read no arithmetic mode (everything is an integer up to the final divisions), so one mode suffices.  Gates:
equality - the masks byte for byte, counts and per-lesion tables integer for integer, the scores bit for bit (the finish sums in the
twin's order; a NaN must be a NaN), no tolerance and no exempt share; a second call bit-equal; the inputs untouched; every output and
the workspace between canaries; pointers off their natural alignment by what the contract allows; a second stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _lesions as Z

pytestmark = pytest.mark.gpu


def _g():
    from tests import _gpu
    return _gpu


def _morph(g, vol, values, conn, it, erode, off=0, stream=None):
    """One uz_vol_morph call, the input `off` bytes behind a 16-byte boundary, the output `off` bytes too, both and the workspace between
    canaries -> out numpy"""
    L = g.L()
    T = vol.size
    in_raw, v = g.guarded(T, torch.uint8, 64, fill=0xEE, off=off)
    v.copy_(torch.from_numpy(np.array(vol).reshape(-1)))
    before = in_raw.clone()
    nbytes = L.uz_vol_morph_workspace(*vol.shape)
    assert nbytes > 0
    ws_raw, ws = g.guarded(nbytes, torch.uint8, 256)
    out_raw, out = g.guarded(T, torch.uint8, 64, off=off)
    torch.cuda.synchronize()
    rc = L.uz_vol_morph(v.data_ptr(), *vol.shape, Z.region_bits(values), conn, it, erode, out.data_ptr(), ws.data_ptr(), g.stream() if stream is None else stream)
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(ws_raw, ws) and g.intact(out_raw, out) and torch.equal(in_raw, before)
    return out.cpu().numpy().reshape(vol.shape)


def _lesions(g, c, off=0, stream=None, want_lesions=True, **over):
    """One uz_vol_lesion_scores call; pred and ref `off` bytes behind a 16-byte boundary, the int64 / fp64 outputs `off` elements behind
    one (8-byte alignment is what the contract asks) -> (counts, lesions or None, scores) numpy"""
    L = g.L()
    p = dict(c.params, **over)
    N, D, H, W = c.pred.shape
    R, ML = len(c.pred_regions), p["max_lesions"]
    pr_raw, pr = g.guarded(c.pred.size, torch.uint8, 64, fill=0xEE, off=off)
    rf_raw, rf = g.guarded(c.ref.size, torch.uint8, 64, fill=0xEE, off=off)
    pr.copy_(torch.from_numpy(np.array(c.pred).reshape(-1)))
    rf.copy_(torch.from_numpy(np.array(c.ref).reshape(-1)))
    before = pr_raw.clone(), rf_raw.clone()
    nbytes = L.uz_vol_lesion_scores_workspace(N, R, D, H, W, ML)
    assert nbytes > 0
    ws_raw, ws = g.guarded(nbytes, torch.uint8, 256)
    cn_raw, cn = g.guarded(N * R * 8, torch.int64, off=1 if off else 0)
    le_raw, le = g.guarded(N * R * ML * 3, torch.int64, off=1 if off else 0)
    sc_raw, sc = g.guarded(N * R * 4, torch.float64, off=1 if off else 0)
    ps = (C.c_uint32 * R)(*[Z.region_bits(r) for r in c.pred_regions])
    rs = (C.c_uint32 * R)(*[Z.region_bits(r) for r in c.ref_regions])
    torch.cuda.synchronize()
    rc = L.uz_vol_lesion_scores(pr.data_ptr(), N, ps, rf.data_ptr(), rs, R, D, H, W, p["dilation"], p["min_ref_voxels"], p["min_pred_voxels"], ML, p["max_links"],
                                ws.data_ptr(), cn.data_ptr(), le.data_ptr() if want_lesions else None, sc.data_ptr(), g.stream() if stream is None else stream)
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    assert g.intact(ws_raw, ws) and g.intact(cn_raw, cn) and g.intact(le_raw, le) and g.intact(sc_raw, sc)
    assert torch.equal(pr_raw, before[0]) and torch.equal(rf_raw, before[1])
    if not want_lesions:
        assert bool((le == g.CANARY[torch.int64]).all())
    return (cn.cpu().numpy().reshape(N, R, 8), le.cpu().numpy().reshape(N, R, ML, 3) if want_lesions else None, sc.cpu().numpy().reshape(N, R, 4))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).view(np.uint64).tobytes() == np.ascontiguousarray(b).view(np.uint64).tobytes()


def _canonical_nan(x):
    """the twin's NaN and the kernel's are both the quiet NaN 0x7FF8000000000000"""
    return np.where(np.isnan(x), np.float64(np.nan), x)


# ================================================================================================ uz_vol_morph
@pytest.mark.parametrize("name", Z.MORPH_NAMES)
def test_morph_of_every_case_and_parameter_set(name):
    g = _g()
    c = Z.morph_case(name)
    for conn, it, erode in Z.MORPH_PARAMS:
        want = Z.expected_morph(name, conn, it, erode)
        out = _morph(g, c.vol, c.values, conn, it, erode)
        print(name, c.vol.shape, "connectivity", conn, "iterations", it, "erode", erode, "voxels", int(out.sum()), "mismatches", int((out != want).sum()))
        assert out.dtype == np.uint8 and out.tobytes() == want.tobytes(), (name, conn, it, erode)
    assert _morph(g, c.vol, c.values, 2, 2, 0).tobytes() == _morph(g, c.vol, c.values, 2, 2, 0).tobytes()        # a second call is bit-equal


def test_morph_at_offset_pointers_on_a_second_stream_and_with_the_widest_set():
    g = _g()
    for name in ("w63", "w155", "slab130"):
        c = Z.morph_case(name)
        for off in (1, 7):
            for conn, it, erode in ((2, 2, 0), (3, 1, 1), (1, 3, 1)):
                assert _morph(g, c.vol, c.values, conn, it, erode, off=off).tobytes() == Z.expected_morph(name, conn, it, erode).tobytes(), (name, off, conn, it, erode)
    side = torch.cuda.Stream()
    c = Z.morph_case("sparse155")
    with torch.cuda.stream(side):
        out = _morph(g, c.vol, c.values, 2, 3, 0, stream=side.cuda_stream)
    assert out.tobytes() == Z.expected_morph("sparse155", 2, 3, 0).tobytes()
    # bit 31 of the set travels through the binding; the value 0 can be foreground
    v = (np.array(Z.morph_case("sparse65").vol) == 1).astype(np.uint8) * 31
    assert _morph(g, v, (31,), 2, 1, 0).tobytes() == Z.morph(v, (31,), 2, 1, 0).tobytes() and Z.morph(v, (31,), 2, 1, 0).any()
    assert _morph(g, v, (0, 31), 1, 1, 1).tobytes() == Z.morph(v, (0, 31), 1, 1, 1).tobytes()


def test_a_refused_morph_call_leaves_the_output_untouched():
    g = _g()
    dev, L = g.dev(), g.L()
    c = Z.morph_case("w63")
    v = torch.from_numpy(np.array(c.vol)).to(dev)
    ws = torch.full((L.uz_vol_morph_workspace(*c.vol.shape) + 16,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((c.vol.size,), 0xA5, dtype=torch.uint8, device=dev)
    for kw in (dict(N=0), dict(shape=(4, 0, 63)), dict(conn=0), dict(conn=4), dict(it=-1), dict(erode=2), dict(ws=ws.data_ptr() + 8), dict(ws=None), dict(out=None),
               dict(out=v.data_ptr() + 1)):
        a = dict(N=3, shape=c.vol.shape[1:], conn=1, it=1, erode=0, ws=ws.data_ptr(), out=out.data_ptr())
        a.update(kw)
        rc = L.uz_vol_morph(v.data_ptr(), a["N"], *a["shape"], 2, a["conn"], a["it"], a["erode"], a["out"], a["ws"], g.stream())
        assert rc != 0 and L.uz_last_error().decode().startswith("vol_morph:"), kw
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((out == 0xA5).all()) and torch.equal(v.cpu(), torch.from_numpy(np.array(c.vol)))


# ================================================================================================ uz_vol_lesion_scores
@pytest.mark.parametrize("name", Z.LESION_NAMES)
def test_lesion_scores_of_every_case(name):
    g = _g()
    c = Z.lesion_case(name)
    want_c, want_l, want_s = Z.expected_lesions(name)
    cn, le, sc = _lesions(g, c)
    print(name, c.pred.shape, c.params, "counts", cn.tolist(), "scores", sc.tolist(), "twin", want_s.tolist())
    assert cn.dtype == np.int64 and np.array_equal(cn, want_c), name
    assert np.array_equal(le, want_l), name
    assert np.array_equal(np.isnan(sc), np.isnan(want_s)) and _same_bits(_canonical_nan(sc), _canonical_nan(want_s)), name
    if name in ("speckle_short", "links_short"):                        # overflow rows are NaN, with the counters set
        over = (cn[..., 6] > 0) | (cn[..., 7] > 0)
        assert over.any() and np.isnan(sc[over]).all() and not np.isnan(sc[~over]).any()
    cn2, le2, sc2 = _lesions(g, c)                                        # a second call is bit-equal
    assert cn2.tobytes() == cn.tobytes() and le2.tobytes() == le.tobytes() and sc2.tobytes() == sc.tobytes()
    cn0, none, sc0 = _lesions(g, c, want_lesions=False)                  # lesions = NULL is accepted and changes nothing
    assert none is None and cn0.tobytes() == cn.tobytes() and sc0.tobytes() == sc.tobytes()


def test_lesion_scores_at_offset_pointers_on_a_second_stream_and_with_other_limits():
    g = _g()
    for name in ("nested", "thresholds", "w63"):
        c = Z.lesion_case(name)
        want = Z.expected_lesions(name)
        for off in (1, 5):
            cn, le, sc = _lesions(g, c, off=off)
            assert np.array_equal(cn, want[0]) and np.array_equal(le, want[1]) and _same_bits(sc, want[2]), (name, off)
    side = torch.cuda.Stream()
    c = Z.lesion_case("speckle")
    with torch.cuda.stream(side):
        cn, le, sc = _lesions(g, c, stream=side.cuda_stream)
    want = Z.expected_lesions("speckle")
    assert np.array_equal(cn, want[0]) and np.array_equal(le, want[1]) and _same_bits(sc, want[2])
    # the limits at their ends: dilation 0 and 16, the largest tables, one link
    for over in (dict(dilation=0), dict(dilation=16), dict(max_lesions=4096, max_links=16), dict(max_links=1), dict(min_ref_voxels=0, min_pred_voxels=0)):
        p = dict(c.params, **over)
        want = Z.lesion_scores(c.pred, c.ref, c.pred_regions, c.ref_regions, **p)
        cn, le, sc = _lesions(g, c, **over)
        assert np.array_equal(cn, want[0]) and np.array_equal(le, want[1]), over
        assert np.array_equal(np.isnan(sc), np.isnan(want[2])) and _same_bits(_canonical_nan(sc), _canonical_nan(want[2])), over
    # R = 8, the cap, with repeated sets: every set is read
    c = Z.lesion_case("nested")
    c8 = c._replace(pred_regions=(c.pred_regions * 3)[:8], ref_regions=(c.ref_regions * 3)[:8])
    want = Z.lesion_scores(c8.pred, c8.ref, c8.pred_regions, c8.ref_regions, **c8.params)
    cn, le, sc = _lesions(g, c8)
    assert np.array_equal(cn, want[0]) and np.array_equal(le, want[1]) and _same_bits(sc, want[2])


def test_a_refused_lesion_call_leaves_the_outputs_untouched():
    g = _g()
    dev, L = g.dev(), g.L()
    c = Z.lesion_case("span")
    N, D, H, W = c.pred.shape
    pr, rf = torch.from_numpy(np.array(c.pred)).to(dev), torch.from_numpy(np.array(c.ref)).to(dev)
    ws = torch.full((L.uz_vol_lesion_scores_workspace(N, 1, D, H, W, 4) + 16,), 0xA5, dtype=torch.uint8, device=dev)
    cn = torch.full((N * 8 + 1,), -7777, dtype=torch.int64, device=dev)
    le = torch.full((N * 4 * 3 + 1,), -7777, dtype=torch.int64, device=dev)
    sc = torch.full((N * 4 + 1,), -777.0, dtype=torch.float64, device=dev)
    sets = (C.c_uint32 * 9)(*[2] * 9)
    for kw in (dict(N=0), dict(R=0), dict(R=9), dict(shape=(12, 0, 17)), dict(dil=-1), dict(dil=17), dict(mr=-1), dict(mp=-1), dict(ML=0), dict(ML=4097), dict(links=0),
               dict(links=17), dict(ws=ws.data_ptr() + 8), dict(ws=None), dict(cn=None), dict(sc=None), dict(cn=cn.data_ptr() + 4), dict(le=le.data_ptr() + 4),
               dict(sc=sc.data_ptr() + 4), dict(ps=None), dict(ref=None)):
        a = dict(N=N, R=1, shape=(D, H, W), dil=1, mr=8, mp=0, ML=4, links=2, ws=ws.data_ptr(), cn=cn.data_ptr(), le=le.data_ptr(), sc=sc.data_ptr(), ps=sets, ref=rf.data_ptr())
        a.update(kw)
        rc = L.uz_vol_lesion_scores(pr.data_ptr(), a["N"], a["ps"], a["ref"], sets, a["R"], *a["shape"], a["dil"], a["mr"], a["mp"], a["ML"], a["links"], a["ws"], a["cn"],
                                    a["le"], a["sc"], g.stream())
        assert rc != 0 and L.uz_last_error().decode().startswith("vol_lesion_scores:"), kw
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((cn == -7777).all()) and bool((le == -7777).all()) and bool((sc == -777.0).all())
    assert torch.equal(pr.cpu(), torch.from_numpy(np.array(c.pred))) and torch.equal(rf.cpu(), torch.from_numpy(np.array(c.ref)))


# ================================================================================================ the Python functions
def test_binary_morphology_functions_against_scipy():
    from scipy import ndimage
    from unet_zoo_amd import metrics
    g = _g()
    for name in ("block", "flat65", "sparse65", "w155"):
        c = Z.morph_case(name)
        t = torch.from_numpy(np.array(c.vol)).to(g.dev())
        fg = Z.in_set(c.vol, c.values)
        for conn in Z.CONN:
            for it in (1, 2):
                for _ in range(2):                                       # the second call takes the cached workspace
                    got = metrics.binary_dilation(t, c.values, iterations=it, connectivity=conn)
                assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.is_cuda and got.shape == t.shape
                assert got.cpu().numpy().tobytes() == Z.expected_morph(name, conn, it, 0).tobytes(), (name, conn, it)
                assert metrics.binary_erosion(t, c.values, iterations=it, connectivity=conn).cpu().numpy().tobytes() == Z.expected_morph(name, conn, it, 1).tobytes()
                flat = c.vol.shape[1] == 1
                st = ndimage.generate_binary_structure(2, min(conn, 2)) if flat else ndimage.generate_binary_structure(3, conn)
                opened = metrics.binary_opening(t, c.values, iterations=it, connectivity=conn).cpu().numpy()
                closed = metrics.binary_closing(t, c.values, iterations=it, connectivity=conn).cpu().numpy()
                for n in range(c.vol.shape[0]):
                    m = fg[n, 0] if flat else fg[n]
                    o, cl = (opened[n, 0], closed[n, 0]) if flat else (opened[n], closed[n])
                    assert np.array_equal(o.astype(bool), ndimage.binary_opening(m, structure=st, iterations=it)), (name, conn, it, n)
                    assert np.array_equal(cl.astype(bool), ndimage.binary_closing(m, structure=st, iterations=it)), (name, conn, it, n)
        assert metrics.binary_dilation(t, c.values, iterations=0).cpu().numpy().tobytes() == fg.astype(np.uint8).tobytes()
        assert torch.equal(t.cpu(), torch.from_numpy(np.array(c.vol)))
    # a view that is neither contiguous nor aligned: the Python function makes it dense
    c = Z.morph_case("sparse65")
    big = torch.zeros(2, 4, 6, 66, dtype=torch.uint8, device=g.dev())
    big[..., 1:] = torch.from_numpy(np.array(c.vol)).to(g.dev())
    view = big[..., 1:]
    assert not view.is_contiguous()
    assert metrics.binary_dilation(view, c.values, iterations=2, connectivity=2).cpu().numpy().tobytes() == Z.expected_morph("sparse65", 2, 2, 0).tobytes()


def test_score_lesions_on_tensors_and_on_a_prediction():
    from tests import _golden as G
    from tests import _nets as N
    from unet_zoo_amd import metrics
    g = _g()
    dev = g.dev()
    # tensors: every field against the twin, with and without the per-lesion table
    for name in ("nested", "thresholds", "links_short"):
        c = Z.lesion_case(name)
        want_c, want_l, want_s = Z.expected_lesions(name)
        pr, rf = torch.from_numpy(np.array(c.pred)).to(dev), torch.from_numpy(np.array(c.ref)).to(dev)
        for _ in range(2):                                               # the second call takes the cached workspace
            got = metrics.score_lesions(pr, rf, c.pred_regions, c.ref_regions, return_lesions=True, **c.params)
        assert isinstance(got, metrics.LesionScores) and got.counts.is_cuda and got.lesion_dice.dtype == torch.float64 and got.lesion_dice.shape == want_s.shape[:2]
        assert np.array_equal(got.counts.cpu().numpy(), want_c) and np.array_equal(got.lesions.cpu().numpy(), want_l)
        sc = torch.stack([got.lesion_dice, got.sensitivity, got.precision, got.f1], -1).cpu().numpy()
        assert np.array_equal(np.isnan(sc), np.isnan(want_s)) and _same_bits(_canonical_nan(sc), _canonical_nan(want_s)), name
        assert metrics.score_lesions(pr, rf, c.pred_regions, c.ref_regions, **c.params).lesions is None
    # the Prediction of the small PHISeg3D: its S samples, then the mean label, raw and filtered, against the twin on the tensors copied back.
    # The 1x1 heads' weights are scaled up: as they come, this small network calls every voxel background
    arrays, meta = G.load("phiseg3d_small")
    sd = N.off_identity_state(meta)
    for k in sd:
        if k.startswith("likelihood.s_layer") and k.endswith("weight"):
            sd[k] = sd[k] * 10.0
    net = N.small_phiseg3d(meta, sd)
    torch.manual_seed(5)
    with torch.no_grad():
        pred = net.predict(torch.from_numpy(arrays["patch"]).to(dev), n_samples=4)
    torch.cuda.synchronize()
    nc = int(meta["num_classes"])
    regs = (tuple(range(1, nc)), (0,), (nc - 1,))                        # the foreground, the background, the last class
    rows = torch.cat([pred.labels[:, 0], pred.mean_label], 0).cpu().numpy()
    assert rows.shape[0] == 5 and all(len(np.unique(r)) >= 2 for r in rows)
    ref = np.roll(rows[1], 1, axis=2)
    tr = torch.from_numpy(ref.copy()).to(dev)
    params = dict(dilation=1, min_ref_voxels=3, min_pred_voxels=2, max_lesions=1024, max_links=8)
    got = metrics.score_lesions(pred, tr, regs, return_lesions=True, **params)
    want_c, want_l, want_s = Z.lesion_scores(rows, ref, regs, regs, **params)
    print("prediction rows", rows.shape, "counts", want_c.tolist(), "lesion dice", want_s[..., 0].tolist())
    assert (want_c[:, :2, 0] > 0).all() and (want_c[:, :2, 5] > 0).all() and not want_c[..., 6:].any()       # there is something to score
    assert np.array_equal(got.counts.cpu().numpy(), want_c) and np.array_equal(got.lesions.cpu().numpy(), want_l)
    sc = torch.stack([got.lesion_dice, got.sensitivity, got.precision, got.f1], -1).cpu().numpy()
    assert _same_bits(sc, want_s)
    kept = metrics.keep_largest_components(pred, regs[:1], connectivity=3)
    rows_k = torch.cat([kept.labels[:, 0], kept.mean_label], 0).cpu().numpy()
    got = metrics.score_lesions(kept, tr, regs[:1], **params)
    want_c, _, want_s = Z.lesion_scores(rows_k, ref, regs[:1], regs[:1], **params)
    assert np.array_equal(got.counts.cpu().numpy(), want_c) and (want_c[:, 0, 5] == 1).all()                  # one component per row is left
    assert _same_bits(torch.stack([got.lesion_dice, got.sensitivity, got.precision, got.f1], -1).cpu().numpy(), want_s)
    assert np.array_equal(torch.cat([pred.labels[:, 0], pred.mean_label], 0).cpu().numpy(), rows)              # the draw itself is untouched
