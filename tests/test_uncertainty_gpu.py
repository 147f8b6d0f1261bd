"""Sample uncertainty on the device: uz_vol_uncertainty (csrc/voluncert.hip) through ctypes on every case and content of
tests/_uncertainty.py against the numpy twin, then metrics.score_uncertainty on tensors and on the Predictions of a small PHISeg3D.
The kernels read no arithmetic mode (everything is an integer up to the final divisions), so one mode suffices.  Gates: table, levels
and votes integer for integer, curves and calibration bit for bit (each is one division of exact integers), the areas and the score
within the derived (S + 4) 2^-52 of the exact rational value.  The workspace and every output hold 0xFF before every call and lie
between canaries; a repeated call and a call on a second stream are bit-equal; a refused call writes nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _uncertainty as U

pytestmark = pytest.mark.gpu

GUARD = 256


def _g():
    from tests import _gpu
    return _gpu


def _run(g, smp, dec, ref, preg, rreg, want_votes, off=0, stream=None):
    """One uz_vol_uncertainty call -> dict of numpy results (votes None when not asked for)"""
    L = g.L()
    S, (D, H, W) = smp.shape[0], dec.shape
    R, P = len(preg), dec.size
    sb, sv = g.embed(smp, off)
    db, dv = g.embed(dec, off)
    rb, rv = g.embed(ref, off)
    nbytes = L.uz_vol_uncertainty_workspace(S, R, D, H, W)
    assert nbytes > 0
    sizes = dict(ws=nbytes, table=R * (S + 1) * 4 * 8, levels=R * (S + 1) * 4 * 8, curves=R * (S + 1) * 3 * 8, auc=R * 4 * 8, cal=R * 3 * 8, votes=R * P + 16)
    raw, body = {}, {}
    for k, n in sizes.items():
        raw[k], body[k] = g.guarded(n, torch.uint8, GUARD, 0xFF)
    votes = body["votes"][off:off + R * P]
    psets = (C.c_uint32 * R)(*[U.region_bits(x) for x in preg])
    rsets = (C.c_uint32 * R)(*[U.region_bits(x) for x in rreg])
    st = g.stream() if stream is None else stream.cuda_stream
    rc = L.uz_vol_uncertainty(sv.data_ptr(), S, dv.data_ptr(), psets, rv.data_ptr(), rsets, R, D, H, W, body["ws"].data_ptr(), body["table"].data_ptr(),
                              body["levels"].data_ptr(), body["curves"].data_ptr(), body["auc"].data_ptr(), body["cal"].data_ptr(),
                              votes.data_ptr() if want_votes else None, st)
    torch.cuda.synchronize()
    assert rc == 0, L.uz_last_error()
    for k in sizes:                                                      # nothing outside the buffers
        assert g.intact(raw[k], body[k], 0xFF), k
    assert g.intact(body["votes"], votes, 0xFF)
    if not want_votes:
        assert bool((body["votes"] == 0xFF).all())
    for buf, view, arr in ((sb, sv, smp), (db, dv, dec), (rb, rv, ref)):  # the inputs untouched
        assert view.cpu().numpy().tobytes() == arr.tobytes() and g.intact(buf, view, 0xEE)
    as_np = lambda k, dt, shape: body[k].cpu().numpy().view(dt).reshape(shape).copy()
    return dict(table=as_np("table", np.int64, (R, S + 1, 2, 2)), levels=as_np("levels", np.int64, (R, S + 1, 4)), curves=as_np("curves", np.float64, (R, S + 1, 3)),
                auc=as_np("auc", np.float64, (R, 4)), cal=as_np("cal", np.float64, (R, 3)),
                votes=votes.cpu().numpy().reshape(R, D, H, W).copy() if want_votes else None)


def _check(got, name, what, R, tag):
    v, tab, want = U.expected(name, what, R)
    S = tab.shape[1] - 1
    assert np.array_equal(got["table"], tab), (tag, "table", int((got["table"] != tab).sum()))
    assert np.array_equal(got["levels"], want.levels), (tag, "levels")
    if got["votes"] is not None:
        assert got["votes"].dtype == np.uint8 and got["votes"].tobytes() == v.tobytes(), (tag, "votes", int((got["votes"] != v).sum()))
    assert got["curves"].tobytes() == want.curves.tobytes(), (tag, "curves", float(np.abs(got["curves"] - want.curves).max()))
    assert got["cal"].tobytes() == want.calibration.tobytes(), (tag, "calibration", got["cal"], want.calibration)
    exact = U.exact_auc(want.levels)
    err = max(abs(float(got["auc"][r, k]) - exact[r][k]) for r in range(R) for k in range(4))
    assert err <= U.auc_bound(S), (tag, "auc", float(err), U.auc_bound(S))
    return float(err)


def _same(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


# ================================================================================================ the C entry point
@pytest.mark.parametrize("what", U.CONTENTS)
@pytest.mark.parametrize("name", [c.name for c in U.CASES] + ["stride"])
def test_every_case_and_content_equals_the_twin(name, what):
    g = _g()
    smp, dec, ref, is_index = U.content(name, what)
    worst = 0.0
    for R in U.case(name).R_values:
        preg, rreg = U.region_pair(is_index, R)
        for want_votes in (True, False):
            got = _run(g, smp, dec, ref, preg, rreg, want_votes)
            worst = max(worst, _check(got, name, what, R, (name, what, R, want_votes)))
    print(name, what, smp.shape, "auc error at the most", worst, "of", U.auc_bound(smp.shape[0]))


@pytest.mark.parametrize("off", U.OFFSETS)
@pytest.mark.parametrize("name", U.OFFSET_CASES)
def test_every_pointer_offset_into_a_larger_buffer(name, off):
    g = _g()
    for what in ("random", "blobs_raw", "indices"):
        smp, dec, ref, is_index = U.content(name, what)
        for R in (1, 3, 8):
            preg, rreg = U.region_pair(is_index, R)
            for want_votes in (True, False):
                _check(_run(g, smp, dec, ref, preg, rreg, want_votes, off=off), name, what, R, (name, what, R, want_votes, off))


def test_a_repeated_call_and_a_second_stream_are_bit_equal():
    g = _g()
    side = torch.cuda.Stream()
    for name, what, R in (("mid", "blobs_raw", 3), ("odd_p", "random", 8), ("wg", "random", 3), ("s_max", "random", 8)):
        smp, dec, ref, is_index = U.content(name, what)
        preg, rreg = U.region_pair(is_index, R)
        a = _run(g, smp, dec, ref, preg, rreg, True)
        b = _run(g, smp, dec, ref, preg, rreg, True)
        with torch.cuda.stream(side):
            c = _run(g, smp, dec, ref, preg, rreg, True, stream=side)
        assert _same(a, b) and _same(a, c), (name, what, R)
        _check(c, name, what, R, (name, what, R, "side stream"))


def test_a_refused_call_leaves_the_outputs_untouched():
    g = _g()
    dev, L = g.dev(), g.L()
    S, R, shape = 4, 3, (2, 3, 64)
    P = 2 * 3 * 64
    vol = torch.zeros(S * P + 2 * P, dtype=torch.uint8, device=dev)
    outs = torch.full((65536,), 0xFF, dtype=torch.uint8, device=dev)
    base = outs.data_ptr()
    assert base % 16 == 0
    K = 8192
    sets = (C.c_uint32 * 9)(*[0b10110, 0b10010, 0b10000] * 3)
    for kw in (dict(samples=None), dict(dec=None), dict(ref=None), dict(ps=None), dict(rs=None), dict(ws=None), dict(table=None), dict(levels=None),
               dict(curves=None), dict(auc=None), dict(cal=None), dict(S=0), dict(S=256), dict(R=0), dict(R=9), dict(shape=(2, 0, 64)), dict(shape=(0, 3, 64)),
               dict(shape=(2, 3, 0)), dict(S=2, shape=(1024, 1024, 1024)), dict(ws=base + 8), dict(table=base + K + 4), dict(levels=base + 2 * K + 4),
               dict(curves=base + 3 * K + 2), dict(auc=base + 4 * K + 1), dict(cal=base + 5 * K + 4)):
        a = dict(samples=vol.data_ptr(), S=S, dec=vol.data_ptr() + S * P, ps=sets, ref=vol.data_ptr() + (S + 1) * P, rs=sets, R=R, shape=shape, ws=base,
                 table=base + K, levels=base + 2 * K, curves=base + 3 * K, auc=base + 4 * K, cal=base + 5 * K, votes=base + 6 * K)
        a.update(kw)
        rc = L.uz_vol_uncertainty(a["samples"], a["S"], a["dec"], a["ps"], a["ref"], a["rs"], a["R"], *a["shape"], a["ws"], a["table"], a["levels"], a["curves"],
                                  a["auc"], a["cal"], a["votes"], g.stream())
        assert rc == -1 and L.uz_last_error().decode().startswith("vol_uncertainty:"), kw
    torch.cuda.synchronize()
    assert bool((outs == 0xFF).all()) and not bool(vol.any())


# ================================================================================================ the Python function
def _check_scores(sc, smp, dec, ref, preg, rreg, with_votes):
    from unet_zoo_amd import metrics
    R, S = len(preg), smp.shape[0]
    tab = U.table(smp, dec, ref, preg, rreg)
    want = U.derive(tab)
    assert isinstance(sc, metrics.UncertaintyScores) and all(t.is_cuda for t in sc if t is not None)
    assert sc.table.dtype == torch.int64 and sc.table.shape == (R, S + 1, 2, 2) and np.array_equal(sc.table.cpu().numpy(), tab)
    assert sc.levels.shape == (R, S + 1, 4) and np.array_equal(sc.levels.cpu().numpy(), want.levels)
    for k, t in enumerate((sc.dice, sc.ftp, sc.ftn)):
        assert t.dtype == torch.float64 and t.shape == (R, S + 1) and t.cpu().numpy().tobytes() == np.ascontiguousarray(want.curves[..., k]).tobytes()
    assert sc.dice.data_ptr() + 8 == sc.ftp.data_ptr() == sc.ftn.data_ptr() - 8                  # views of one buffer
    assert sc.calibration.cpu().numpy().tobytes() == want.calibration.tobytes()
    exact = U.exact_auc(want.levels)
    auc = sc.auc.cpu().numpy()
    assert auc.shape == (R, 4) and all(abs(float(auc[r, k]) - exact[r][k]) <= U.auc_bound(S) for r in range(R) for k in range(4))
    if with_votes:
        assert sc.votes.dtype == torch.uint8 and sc.votes.cpu().numpy().tobytes() == U.votes(smp, preg).tobytes()
    else:
        assert sc.votes is None


def test_score_uncertainty_on_tensors_and_views():
    from unet_zoo_amd import metrics
    g = _g()
    dev = g.dev()
    smp, dec, ref, _ = U.content("mid", "blobs_raw")
    ts, td, tr = (torch.from_numpy(np.array(a)).to(dev) for a in (smp, dec, ref))
    for _ in range(2):                                                   # the second call takes the cached workspace
        _check_scores(metrics.score_uncertainty(ts, tr, U.BRATS, decision=td, return_votes=True), smp, dec, ref, U.BRATS, U.BRATS, True)
    _check_scores(metrics.score_uncertainty(ts, tr, U.BRATS, decision=td[None]), smp, dec, ref, U.BRATS, U.BRATS, False)
    # class indices against raw values
    smp, dec, ref, _ = U.content("odd_p", "indices")
    ts, td, tr = (torch.from_numpy(np.array(a)).to(dev) for a in (smp, dec, ref))
    _check_scores(metrics.score_uncertainty(ts, tr, U.INDEX, U.BRATS, decision=td, return_votes=True), smp, dec, ref, U.INDEX, U.BRATS, True)
    # a view that is neither contiguous nor aligned: the function makes it dense
    big = torch.zeros(16, 3, 5, 68, dtype=torch.uint8, device=dev)
    big[..., 1:] = ts
    assert not big[..., 1:].is_contiguous()
    _check_scores(metrics.score_uncertainty(big[..., 1:], tr, U.INDEX, U.BRATS, decision=td), smp, dec, ref, U.INDEX, U.BRATS, False)
    with pytest.raises(ValueError, match="device of pred"):
        metrics.score_uncertainty(ts, tr.cpu(), U.INDEX, decision=td)


def test_predict_then_score_uncertainty_end_to_end():
    """PHISeg3D.predict(n_samples=4) -> score_uncertainty, as it is, filtered by keep_largest_components, and with decision= given"""
    import oracle
    from tests import _golden as G
    from tests import _nets as N
    from unet_zoo_amd import metrics
    g = _g()
    dev = g.dev()
    arrays, meta = G.load("phiseg3d_small")
    net = N.small_phiseg3d(meta, oracle.deterministic_state_dict(G.spec_of(meta), seed=91))
    torch.manual_seed(5)
    with torch.no_grad():
        pred = net.predict(torch.from_numpy(arrays["patch"]).to(dev), n_samples=4)
    torch.cuda.synchronize()
    K = int(meta["num_classes"])
    regs = tuple(tuple(range(k, K)) for k in range(1, K))               # nested regions of class indices: everything, ..., the last class
    smp, dec = pred.labels[:, 0].cpu().numpy(), pred.mean_label[0].cpu().numpy()
    assert smp.shape[0] == 4 and smp.dtype == np.uint8
    ref = np.roll(smp[1], 1, axis=2)                                     # a reference that overlaps the samples without being one
    tr = torch.from_numpy(ref.copy()).to(dev)
    _check_scores(metrics.score_uncertainty(pred, tr, regs, return_votes=True), smp, dec, ref, regs, regs, True)
    filt = metrics.keep_largest_components(pred, regions=regs)
    fs, fd = filt.labels[:, 0].cpu().numpy(), filt.mean_label[0].cpu().numpy()
    _check_scores(metrics.score_uncertainty(filt, tr, regs), fs, fd, ref, regs, regs, False)
    # the filtered mean label as the decision, the samples unfiltered
    _check_scores(metrics.score_uncertainty(pred, tr, regs, decision=filt.mean_label, return_votes=True), smp, fd, ref, regs, regs, True)
    assert np.array_equal(pred.labels[:, 0].cpu().numpy(), smp)          # the draw itself is untouched
