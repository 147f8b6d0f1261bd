"""Sample uncertainty without a GPU: the numpy twin of tests/_uncertainty.py equals a brute-force reference that knows nothing of the
vote table on every case the GPU test runs (the grid-striding one excepted: its content is the same, its size a matter of the device),
every deliberate defect of the twin fails those gates on the case named here, uz_vol_uncertainty_route and the workspace size claim what
the case set says it reaches, a bad call is refused with its reason before anything is launched (the library loads, and refuses,
without a device), score_uncertainty checks its arguments before any device work, and the binding parses the new declarations."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _uncertainty as U


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib(), _ffi


def _gates(got_tab, got, want):
    """the reasons for which (table, Derived) misses the brute-force Brute `want`; empty when it passes"""
    bad = []
    R, S = got_tab.shape[0], got_tab.shape[1] - 1
    bound = U.auc_bound(S)
    for r in range(R):
        if [tuple(int(x) for x in row) for row in got.levels[r]] != want.levels[r]:
            bad.append(("levels", r))
        if int(got_tab[r].sum()) != sum(want.levels[r][S]):
            bad.append(("sum", r))
        for j in range(S + 1):
            if tuple(float(x) for x in got.curves[r, j]) != tuple(float(f) for f in want.curves[r][j]):
                bad.append(("curves", r, j))
        if tuple(float(x) for x in got.calibration[r]) != tuple(float(f) for f in want.calibration[r]):
            bad.append(("calibration", r))
        for k in range(4):
            if not abs(float(got.auc[r, k]) - want.auc[r][k]) <= bound:
                bad.append(("auc", r, k))
    return bad


# ================================================================================================ twin against brute force
@pytest.mark.parametrize("name", [c.name for c in U.CASES])
def test_twin_equals_the_brute_force_reference(name):
    for what in U.CONTENTS:
        smp, dec, ref, is_index = U.content(name, what)
        for R in U.case(name).R_values:
            preg, rreg = U.region_pair(is_index, R)
            v, tab, got = U.expected(name, what, R)
            want = U.brute(smp, dec, ref, preg, rreg)
            assert tab.shape == (R, smp.shape[0] + 1, 2, 2) and all(int(tab[r].sum()) == dec.size for r in range(R))
            assert _gates(tab, got, want) == [], (name, what, R)
            ex = U.exact_auc(got.levels)
            assert all(ex[r][k] == want.auc[r][k] for r in range(R) for k in range(4))
            assert v.shape == (R,) + dec.shape and int(v.max()) <= smp.shape[0]


def test_contents_hold_what_they_claim():
    smp, dec, ref, _ = U.content("odd_p", "background")
    assert not smp.any() and not dec.any() and not ref.any()
    v, tab, _ = U.expected("odd_p", "full", 8)
    assert (v == 16).all() and all(int(tab[r, 16, 1, 1]) == dec.size for r in range(8))
    smp, dec, ref, _ = U.content("mid", "random")
    assert set(np.unique(smp)) == {0, 1, 2, 4, 36, 200} and (dec == 200).any() and (ref == 36).any()
    v, tab, _ = U.expected("odd_p", "half", 3)
    assert tab[2, 8].all() and not np.array_equal(tab[2, 8, 0], tab[2, 8, 1]) and int(tab[2, 8].sum()) == 2 * (3 * 5 * 67) // 3      # c = S / 2 on both sides
    v, tab, _ = U.expected("mid", "contra", 3)
    assert int(tab[0, 5, 0].sum()) > 0 and int(tab[2, 3, 0].sum()) > 0 and int(tab[2, 0, 1].sum()) == 0                            # all five and a bare majority against d = 0
    _, tab, _ = U.expected("mid", "blobs_raw", 3)
    assert all((tab[r].reshape(6, 4).sum(1) > 0).sum() >= 4 for r in range(3))                  # the rim spreads over the vote counts
    assert U.content("mid", "indices")[3] and set(np.unique(U.content("mid", "indices")[0])) == {0, 1, 2, 3}
    assert U.regions(8)[7] == (0, 4) and U.regions(1) == ((1, 2, 4),) and U.regions(3, U.INDEX) == U.INDEX


# which case (name, content, R) notices which defect
NOTICED_BY = {"s_minus_1": ("odd_p", "random", 3), "majority_decision": ("mid", "contra", 3), "pred_sets_for_ref": ("mid", "indices", 3),
              "drop_tail16": ("odd_p", "random", 1), "a_lt_j": ("mid", "blobs_raw", 3), "tie_wrong_side": ("odd_p", "half", 3),
              "wrap_32": ("mid", "random", 3), "ftn_from_tp": ("mid", "blobs_raw", 1), "drop_last_slice": ("wg_p1", "random", 1)}


@pytest.mark.parametrize("defect", U.DEFECTS)
def test_every_defect_fails_the_gates_on_the_named_case(defect):
    assert set(NOTICED_BY) == set(U.DEFECTS)
    name, what, R = NOTICED_BY[defect]
    smp, dec, ref, is_index = U.content(name, what)
    preg, rreg = U.region_pair(is_index, R)
    want = U.brute(smp, dec, ref, preg, rreg)
    tab = U.table(smp, dec, ref, preg, rreg, defects=(defect,))
    bad = _gates(tab, U.derive(tab, defects=(defect,)), want)
    print(defect, name, what, R, bad[:4])
    assert bad, (defect, name, what, R)
    assert _gates(U.expected(name, what, R)[1], U.expected(name, what, R)[2], want) == []


# ================================================================================================ route, workspace, refusals
def _route(L, S, R, D, H, W, align):
    out = (C.c_int * 3)()
    assert L.uz_vol_uncertainty_route(S, R, D, H, W, align, out) == 0, L.uz_last_error()
    return tuple(out)


def test_route_claims_of_the_case_set():
    L, _ = _lib()
    reached = set()
    want_form = {"one": 0, "subwave": 0, "vec": 1, "odd_p": 0, "mid": 0, "s_max": 0, "wg": 1, "wg_m1": 0, "wg_p1": 0}
    for c in U.CASES:
        P = c.D * c.H * c.W
        for R in c.R_values:
            form, wgs, strides = _route(L, c.S, R, c.D, c.H, c.W, 16)
            assert form == want_form[c.name] and strides == 0, (c.name, R)
            assert wgs == (max(1, -(-(P // 16) // 256)) if form else -(-P // 256)), (c.name, wgs)
            reached.add(("wide", "scalar")[1 - form])
    # one workgroup's voxels of the wide form: n fills one, 16 more start the second
    assert _route(L, 2, 1, 1, 1, U.WG_WIDE, 16)[1] == 1 and _route(L, 2, 1, 1, 1, U.WG_WIDE + 16, 16)[1] == 2
    assert _route(L, 2, 1, 1, 1, U.WG_WIDE + 1, 16) == (0, 17, 0)           # odd P: the second row is misaligned, more than one scalar workgroup
    # the offsets: 1 and 15 leave the scalar form, 4 the 4-byte loads where every row allows them
    for name in U.OFFSET_CASES:
        c = U.case(name)
        P = c.D * c.H * c.W
        for off, align in zip(U.OFFSETS, (1, 4, 1)):
            form, wgs, _ = _route(L, c.S, 3, c.D, c.H, c.W, align)
            assert form == (1 if align == 4 and P % 4 == 0 else 0), (name, off)
            assert wgs == (-(-(P // 4) // 256) if form else -(-P // 256))
    assert _route(L, 4, 3, 2, 3, 64, 4)[0] == 1 and _route(L, 4, 3, 2, 3, 64, 8)[0] == 1 and _route(L, 4, 3, 2, 3, 64, 2)[0] == 0
    # grid-striding: STRIDE_P - 37 is the smallest P that does
    c = U.STRIDE
    assert _route(L, 1, 1, 1, 1, c.W, 16) == (1, U.CAP, 1) and _route(L, 1, 1, 1, 1, c.W - 37, 16) == (1, U.CAP, 1)
    assert _route(L, 1, 1, 1, 1, c.W - 38, 16) == (1, U.CAP, 0)
    assert c.W % 16 != 0 and 3 * c.W < 40e6                              # a scalar tail, and a few tens of MB
    reached.add("stride")
    assert reached == {"scalar", "wide", "stride"}
    # S = 1 and one region: rows cannot be misaligned against each other, any P goes wide; a second votes row at odd P cannot
    assert _route(L, 1, 1, 3, 5, 67, 16)[0] == 1 and _route(L, 1, 2, 3, 5, 67, 16)[0] == 0 and _route(L, 2, 1, 3, 5, 67, 16)[0] == 0
    # the BraTS volume: wide, capped, striding
    assert _route(L, 16, 3, 155, 240, 240, 16) == (1, U.CAP, 1)


def test_workspace_sizes_and_refused_sizes():
    L, _ = _lib()
    up16 = lambda b: (b + 15) // 16 * 16
    for S, R, D, H, W in [(1, 1, 1, 1, 1), (16, 3, 3, 5, 67), (255, 8, 2, 3, 37), (16, 3, 155, 240, 240), (16, 3, 128, 128, 128), (255, 8, 1, 1, 8421504), (1, 1, 1, 1, U.STRIDE_P)]:
        P = D * H * W
        assert L.uz_vol_uncertainty_workspace(S, R, D, H, W) == up16(min(U.CAP, -(-P // 256)) * R * (S + 1) * 4 * 4), (S, R, D, H, W)
    assert L.uz_vol_uncertainty_workspace(255, 8, 1, 1, 8421504) == 1024 * 32768       # the largest table: 32 KB a workgroup
    out = (C.c_int * 3)()
    for S, R, D, H, W in [(0, 1, 4, 4, 4), (256, 1, 4, 4, 4), (4, 0, 4, 4, 4), (4, 9, 4, 4, 4), (4, 1, 0, 4, 4), (4, 1, 4, 0, 4), (4, 1, 4, 4, 0), (2, 1, 1024, 1024, 1024),
                          (1, 1, 2048, 1024, 1024), (255, 1, 8421505, 1, 1), (16, 3, 65536, 65536, 65536)]:
        assert L.uz_vol_uncertainty_workspace(S, R, D, H, W) == 0, (S, R, D, H, W)
        assert L.uz_vol_uncertainty_route(S, R, D, H, W, 16, out) != 0 and L.uz_last_error().decode().startswith("vol_uncertainty_route:"), (S, R, D, H, W)
    assert L.uz_vol_uncertainty_workspace(1, 1, 2047, 1024, 1024) > 0 and L.uz_vol_uncertainty_workspace(255, 1, 8421504, 1, 1) > 0      # just below 2^31
    assert L.uz_vol_uncertainty_route(4, 1, 4, 4, 4, 16, None) != 0 and L.uz_vol_uncertainty_route(4, 1, 4, 4, 4, 3, out) != 0


def test_refusals_name_their_reason():
    """Refused before any launch: the device pointers are host memory that is never read or written (the sets are host arrays by contract)."""
    L, _ = _lib()
    host = np.zeros(16384, np.float64)
    ptr = host.ctypes.data
    assert ptr % 16 == 0
    sets = (C.c_uint32 * 9)(*[0b10110, 0b10010, 0b10000] * 3)
    sp = C.addressof(sets)
    K = 8192                                                             # bytes between the buffers

    def call(samples=ptr, S=4, dec=ptr + K, ps=sp, ref=ptr + 2 * K, rs=sp, R=3, shape=(4, 4, 4), ws=ptr + 3 * K, table=ptr + 8 * K, levels=ptr + 9 * K,
             curves=ptr + 10 * K, auc=ptr + 11 * K, cal=ptr + 12 * K, votes=ptr + 13 * K):
        rc = L.uz_vol_uncertainty(samples, S, dec, ps, ref, rs, R, *shape, ws, table, levels, curves, auc, cal, votes, None)
        return rc, L.uz_last_error().decode()

    for kw, reason in [(dict(samples=None), "null"), (dict(dec=None), "null"), (dict(ps=None), "null"), (dict(ref=None), "null"), (dict(rs=None), "null"),
                       (dict(ws=None), "null"), (dict(table=None), "null"), (dict(levels=None), "null"), (dict(curves=None), "null"), (dict(auc=None), "null"),
                       (dict(cal=None), "null"), (dict(S=0), "1 <= S <= 255"), (dict(S=256), "1 <= S <= 255"), (dict(R=0), "1 <= R <= 8"), (dict(R=9), "1 <= R <= 8"),
                       (dict(shape=(0, 4, 4)), "empty axis"), (dict(shape=(4, 0, 4)), "empty axis"), (dict(shape=(4, 4, 0)), "empty axis"),
                       (dict(shape=(1024, 1024, 1024)), "2^31"), (dict(S=2, shape=(1024, 1024, 1024)), "2^31"), (dict(S=255, shape=(8421505, 1, 1)), "2^31"),
                       (dict(ws=ptr + 3 * K + 8), "16-byte"), (dict(table=ptr + 8 * K + 4), "8-byte"), (dict(levels=ptr + 9 * K + 4), "8-byte"),
                       (dict(curves=ptr + 10 * K + 4), "8-byte"), (dict(auc=ptr + 11 * K + 2), "8-byte"), (dict(cal=ptr + 12 * K + 1), "8-byte")]:
        rc, msg = call(**kw)
        assert rc == -1 and reason in msg and msg.startswith("vol_uncertainty:"), (kw.keys(), rc, msg)
    assert not host.any()


# ================================================================================================ the Python function, the binding
def test_argument_errors_of_score_uncertainty():
    from unet_zoo_amd import metrics
    smp = torch.zeros(3, 4, 5, 6, dtype=torch.uint8)
    vol = torch.zeros(4, 5, 6, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        metrics.score_uncertainty(smp.int(), vol, U.BRATS, decision=vol)
    with pytest.raises(TypeError, match="uint8"):
        metrics.score_uncertainty(smp.numpy(), vol, U.BRATS, decision=vol)
    with pytest.raises(ValueError, match=r"not \(S, D, H, W\)"):
        metrics.score_uncertainty(smp[0], vol, U.BRATS, decision=vol)
    with pytest.raises(ValueError, match="decision is required"):
        metrics.score_uncertainty(smp, vol, U.BRATS)
    with pytest.raises(TypeError, match="decision must be a uint8"):
        metrics.score_uncertainty(smp, vol, U.BRATS, decision=vol.float())
    with pytest.raises(TypeError, match="reference must be a uint8"):
        metrics.score_uncertainty(smp, vol.long(), U.BRATS, decision=vol)
    with pytest.raises(ValueError, match="decision .* does not match"):
        metrics.score_uncertainty(smp, vol, U.BRATS, decision=vol[:3])
    with pytest.raises(ValueError, match="reference .* does not match"):
        metrics.score_uncertainty(smp, vol[:, :4], U.BRATS, decision=vol)
    with pytest.raises(ValueError, match="3 regions of pred against 2"):
        metrics.score_uncertainty(smp, vol, U.BRATS, U.BRATS[:2], decision=vol)
    with pytest.raises(ValueError, match="label value 32"):
        metrics.score_uncertainty(smp, vol, ((1, 32),), decision=vol)
    with pytest.raises(ValueError, match="label value -1"):
        metrics.score_uncertainty(smp, vol, U.BRATS, ((1,), (2,), (-1,)), decision=vol)
    with pytest.raises(ValueError, match="on the device"):
        metrics.score_uncertainty(smp, vol, U.BRATS, decision=vol)
    with pytest.raises(ValueError, match="on the device"):
        metrics.score_uncertainty(smp, vol, U.BRATS, decision=vol[None])                       # (1, D, H, W) is taken as one volume
    P = collections.namedtuple("P", "labels mean_label")
    with pytest.raises(TypeError, match="uint8"):
        metrics.score_uncertainty(P(torch.zeros(2, 1, 4, 5, 6), torch.zeros(1, 4, 5, 6, dtype=torch.uint8)), vol, U.BRATS)
    with pytest.raises(ValueError, match="Prediction of one volume expected"):
        metrics.score_uncertainty(P(torch.zeros(2, 2, 4, 5, 6, dtype=torch.uint8), torch.zeros(2, 4, 5, 6, dtype=torch.uint8)), vol, U.BRATS)
    with pytest.raises(ValueError, match="Prediction of one volume expected"):
        metrics.score_uncertainty(P(torch.zeros(2, 3, 5, 6, dtype=torch.uint8), torch.zeros(3, 5, 6, dtype=torch.uint8)), vol, U.BRATS)
    with pytest.raises(ValueError, match="on the device"):
        metrics.score_uncertainty(P(torch.zeros(2, 1, 4, 5, 6, dtype=torch.uint8), torch.zeros(1, 4, 5, 6, dtype=torch.uint8)), vol, U.BRATS)
    assert metrics.UncertaintyScores._fields == ("table", "levels", "dice", "ftp", "ftn", "auc", "calibration", "votes")


def test_binding_parses_the_new_declarations():
    _, ffi = _lib()
    protos = ffi.prototypes()
    vp, i = C.c_void_p, C.c_int
    assert protos["uz_vol_uncertainty_workspace"] == (C.c_size_t, [i] * 5)
    assert protos["uz_vol_uncertainty"] == (i, [vp, i, vp, vp, vp, vp, i, i, i, i] + [vp] * 8)
    assert protos["uz_vol_uncertainty_route"] == (i, [i] * 6 + [vp])
    printable = {C.c_int, C.c_size_t, C.c_void_p, C.c_char_p}           # what a stub generator can print by value, and pointers
    for name in ("uz_vol_uncertainty_workspace", "uz_vol_uncertainty", "uz_vol_uncertainty_route"):
        assert set(protos[name][1]) <= printable and name in ffi.header_symbols()
    # the declarations in front are parsed as before
    assert protos["uz_vol_components_route"] == (i, [i] * 4 + [vp]) and protos["uz_vol_region_scores_workspace"] == (C.c_size_t, [i] * 6)
