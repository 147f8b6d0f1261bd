"""The split-storage dispatch table (tests/_split_routes.py) without a GPU: every case takes the routes it claims and the table
enters all twelve (tile geometry x operand / epilogue form) instances of the forward / data-gradient kernel, the four tile forms of
the weight gradient and chunk loops in 1, 2 and 4 parts; the numpy twin of split storage has split_f16.h's properties; the
structured inputs meet their conditions with no element excluded; every case tells each of the eleven defects that can apply to
it apart by more than 10 gates; and the refusals of the _ex entry points are decided on the host."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _conv_routes as R
from tests import _split_routes as S
from tests.test_conv_routes_gpu import BN_SUM, GATE

IDX = list(enumerate(S.CASES))
IDS = [S.case_id(c) for c in S.CASES]


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib()


# ----------------------------------------------------------------------------- claims
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_case_takes_the_routes_it_claims(case):
    L = _lib()
    with R.dispatch_state(L, case.mode):
        got = S.queries(L, case)
    assert got == case.claims, f"{S.case_id(case)}: claims {case.claims}, the dispatch answers {got}"
    assert case.claims["route"] == 1 and S.key_of(case) in GATE


def test_the_table_enters_every_instance():
    assert len(IDS) == len(set(IDS))
    geos = ("16x16", "16x32-c32", "16x32-c64")
    inst = {S.instance(c) for c in S.CASES if c.direction != "wgrad"}
    assert inst == {(g, f) for g in geos for f in ("XF1", "XF3", "MK2", "MK2-XF1")}, inst
    assert {S.instance(c) for c in S.CASES if c.direction == "fwd" and c.form in ("pk", "seg")} == {(g, "XF1") for g in geos}
    assert {S.instance(c) for c in S.CASES if c.direction == "dgrad" and c.form == "pk"} == {(g, "XF1") for g in geos}
    assert {c.claims["parts"] for c in S.CASES if c.direction == "fwd"} == {1, 2, 4}
    wg = [c for c in S.CASES if c.direction == "wgrad"]
    assert {S.geometry(c) for c in wg} == {"16px-c32", "16px-c64", "32px-c32", "32px-c64"}
    assert {frozenset(c.opt & {"xp", "dp"}) for c in wg} == {frozenset({"xp"}), frozenset({"dp"}), frozenset({"xp", "dp"})}
    # the imported weight-gradient gates were set from sums of at least this many terms (tests/_conv_routes.py)
    for c in wg:
        smallest = min(r.N * r.H * r.W for r in R.CASES if r.gpu and (r.mode, r.direction, r.claims["route"]) == S.key_of(c))
        assert c.N * c.H * c.W >= smallest, S.case_id(c)
    # fold: both epilogues per geometry, misalignment alone, both bn_relu values; aff: both bn_relu values per geometry
    fold = [c for c in S.CASES if c.form == "fold"]
    for g in geos:
        assert {c.W % 4 == 0 and not (c.opt & {"mis-dx", "mis-y"}) for c in fold if S.geometry(c) == g} == {True, False}
        assert any(c.W % 4 == 0 and c.opt & {"mis-dx", "mis-y"} for c in fold if S.geometry(c) == g)
        assert {c.bn_relu for c in S.CASES if c.form == "aff" and S.geometry(c) == g} == {0, 1}
    assert {c.bn_relu for c in fold} == {0, 1}
    for c in S.CASES:
        if c.seg:
            assert c.seg % 16 == 0 and 0 < c.seg < S.contraction(c)[0]
    assert all(any(S.applies(c, n) for c in S.CASES) for n in S.DEFECTS)


# ----------------------------------------------------------------------------- the pack / unpack twin
def test_twin_round_trip_zeros_clamp_and_repack():
    g = np.random.default_rng(5)
    v = (g.standard_normal(200000) * 3).astype(np.float32)
    v[:6] = [0.0, -0.0, 1e-6, -2.5e-7, 2.0 ** -30, -2.0 ** -40]
    amax = np.float32(np.abs(v).max())
    w = S.pack_split(v, amax)
    back = S.unpack_split(w, amax)
    err = np.abs(back.astype(np.float64) - v.astype(np.float64))
    assert float((err - 2.0 ** -22 * np.abs(v.astype(np.float64))).max()) <= 2.0 ** -38 * float(amax)
    # signed zeros: h1 keeps the sign, h2 is +0, the decoded value is +0
    assert w[0] == 0 and w[1] == 0x8000 and back[0] == 0.0 and back[1] == 0.0 and not np.signbit(back[1])
    # re-packing an unpacked value is the identity (on the values: a negative that underflowed to -0 re-packs with h2 = +0)
    assert np.array_equal(S.unpack_split(S.pack_split(back, amax), amax), back)
    # a value above the bound: scaled beyond the fp16 range it is clamped to +-65504, h2 = 0
    s = float(S.split_scale(amax))
    big = np.array([70000.0 / s, -1e30, 65504.0 / s], dtype=np.float32)
    wb = S.pack_split(big, amax)
    h1, h2 = S.halves(wb)
    assert h1.tolist() == [65504.0, -65504.0, 65504.0] and h2.tolist() == [0.0, 0.0, 0.0]
    assert np.isfinite(S.unpack_split(wb, amax)).all()


def test_twin_scale_at_and_beside_a_power_of_two():
    """split_f16.h:25-30: amax in [2^k, 2^(k+1)) has exponent field k + 127, s = 2^(13 - k): amax s in [2^13, 2^14)"""
    for k in (-20, -1, 0, 1, 7):
        at = np.float32(2.0 ** k)
        below, above = np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(np.inf))
        assert float(S.split_scale(at)) == 2.0 ** (13 - k) == float(S.split_scale(above))
        assert float(S.split_scale(below)) == 2.0 ** (14 - k)
        for a in (at, below, above):
            assert 2.0 ** 13 <= float(a) * float(S.split_scale(a)) < 2.0 ** 14
            assert float(S.split_scale(a)) * float(S.split_inv_scale(a)) == 1.0
    # the clamps of the exponent field: zero and huge bounds
    assert float(S.split_scale(np.float32(0))) == 2.0 ** 126 and float(S.split_scale(np.float32(3e38))) == 2.0 ** -114


# ----------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("idx,case", [(i, c) for i, c in IDX if c.form == "fold"], ids=[S.case_id(c) for c in S.CASES if c.form == "fold"])
def test_fold_inputs_keep_the_mask_margin_and_both_signs(idx, case):
    margin, share = S.fold_conditions(case, S.operands(case, idx))
    assert margin >= 2.0 ** -20, f"an element within {margin:.2e} of the ReLU threshold: choose another seed"
    assert share >= 0.25, f"a channel with only {share:.2f} of its elements on one side"


@pytest.mark.parametrize("idx,case", [(i, c) for i, c in IDX if c.seg], ids=[S.case_id(c) for c in S.CASES if c.seg])
def test_segment_bounds_differ_by_sixty_four(idx, case):
    ops = S.operands(case, idx)
    pk = ops.apk
    assert case.ratio in (64.0, 1.0 / 64.0)
    assert float(S.split_scale(pk.amax)) / float(S.split_scale(pk.amax2)) == case.ratio
    x = ops.a
    assert float(x[:, :case.seg].abs().max()) <= float(pk.amax) and float(x[:, case.seg:].abs().max()) <= float(pk.amax2)
    # both segments use their range: no bound more than 4x above its segment's largest value
    assert float(x[:, :case.seg].abs().max()) * 4 > float(pk.amax) or float(x[:, case.seg:].abs().max()) * 4 > float(pk.amax2)
    assert torch.equal(pk.dec.float().double(), pk.dec) and torch.equal(pk.dec32.double(), pk.dec)      # the decoded values are fp32 numbers


# ----------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("idx,case", IDX, ids=IDS)
def test_the_case_tells_every_applicable_defect_apart(idx, case):
    """Each defective evaluation of the fp64 reference leaves the true one by more than 10 gates in at least one gated quantity
    (or is not finite: a NaN canary reached the result), so a kernel with that defect cannot pass the case on the GPU."""
    ops = S.operands(case, idx)
    true = S.evaluate(case, ops)
    for q in true.values():
        assert bool(torch.isfinite(q.ref).all())
    gate = GATE[S.key_of(case)]
    n_applicable = 0
    for n in S.DEFECTS:
        if not S.applies(case, n):
            continue
        n_applicable += 1
        worst = S.moved(true, S.evaluate(case, ops, n), gate, BN_SUM)
        assert worst > 1.0, f"{S.case_id(case)}: defect {n} ({S.DEFECTS[n]}) moves nothing by more than 10 gates (worst {worst:.2e})"
    assert n_applicable > 0


# ----------------------------------------------------------------------------- refusals decided on the host
P = 1 << 20          # a non-null address: no refused call may touch it


def _refused(L, name, rc, launcher=False):
    """launcher: the refusal is worded by the shared launcher the entry point forwards to (conv_split.hip conv_split_impl,
    "conv_split: ..."), which serves several entry points - still on the host, before any HIP call"""
    msg = L.uz_last_error().decode()
    assert rc != 0, f"{name} accepted the call"
    assert name[3:] in msg or (launcher and msg.startswith("conv_split:")), f"{name}: uz_last_error does not name the entry point: {msg!r}"
    return msg


def test_the_refusals_of_the_ex_calls_are_decided_on_the_host():
    L = _lib()
    big = ctypes.c_size_t(1 << 40)
    N, C, H, W = 2, 33, 17, 18                         # Cin = Cout: uz_conv_workspace is the split path's exact need in both directions

    def fwd(x_amax=P, bnp=None, xp=1, a2=None, seg=0, ws=big):
        return L.uz_conv_fwd_ex(P, C, C, P, None, P, C, C, N, H, W, 3, 0, x_amax, P, None, P, ws, None, bnp, xp, a2, seg, None)

    def fwd_bn(save=P, a_amax=P, bnp=None, ws=big):
        return L.uz_conv_fwd_bn_ex(P, C, C, save, 1, P, None, P, C, C, N, H, W, 3, a_amax, P, None, P, ws, None, bnp, None)

    def bwd(acc=0, dyp=0, y=P, save=P, bnp=P, ws=big, dy_amax=P):
        return L.uz_conv_bwd_data_ex(P, C, C, P, P, C, C, N, H, W, 3, acc, dy_amax, P, P, ws, None, dyp, y, C, save, 1, bnp, None)

    def wgrad(xa=P, da=P, db=None, xp=0, dp=0, ws=big, shape=(8, 64, 64, 16, 16)):
        n, ci, co, h, w = shape
        return L.uz_conv_bwd_weight_ex(P, ci, ci, P, co, co, P, db, n, h, w, 3, xa, da, P, ws, xp, None, 0, dp, None, None)

    for mode in (0, 3):                                 # split storage is the two-piece format
        with R.dispatch_state(L, mode):
            assert "split-fp16 path" in _refused(L, "uz_conv_fwd_ex", fwd())
            _refused(L, "uz_conv_fwd_bn_ex", fwd_bn())
            _refused(L, "uz_conv_bwd_data_ex", bwd(y=None, dyp=1))
            _refused(L, "uz_conv_bwd_weight_ex", wgrad(xp=1))
    with R.dispatch_state(L, 1):
        # a shape whose route is not 1 in the default policy (36 tiles < gmin16)
        assert L.uz_conv_route(0, C, C, N, H, W, 3) == 0 and L.uz_conv_route(1, C, C, N, H, W, 3) == 0
        _refused(L, "uz_conv_fwd_ex", fwd())
        _refused(L, "uz_conv_fwd_bn_ex", fwd_bn())
        _refused(L, "uz_conv_bwd_data_ex", bwd())
        assert L.uz_conv_route(2, 64, 64, 8, 16, 24, 3) == 0
        _refused(L, "uz_conv_bwd_weight_ex", wgrad(xp=1, shape=(8, 64, 64, 16, 24)))
        # a split-K shape: no fused statistics forward, no folded reduction backward
        assert L.uz_conv_split_parts(0, 96, 32, 20, 16, 32) == 2 and L.uz_conv_bn_partials(96, 32, 20, 16, 32, 3) == 0
        rc = L.uz_conv_fwd_ex(P, 96, 96, P, None, P, 32, 32, 20, 16, 32, 3, 0, P, P, None, P, big, None, P, 1, None, 0, None)
        assert "uz_conv_bn_partials() == 0" in _refused(L, "uz_conv_fwd_ex", rc)
        assert L.uz_conv_split_parts(1, 32, 96, 20, 16, 32) == 2 and L.uz_conv_bwd_relu_partials(32, 96, 20, 16, 32, 3) == 0
        rc = L.uz_conv_bwd_data_ex(P, 96, 96, P, P, 32, 32, 20, 16, 32, 3, 0, P, P, P, big, None, 0, P, 32, P, 1, P, None)
        assert "unsplit" in _refused(L, "uz_conv_bwd_data_ex", rc)
        rc = L.uz_conv_fwd_bn_ex(P, 96, 96, P, 1, P, None, P, 32, 32, 20, 16, 32, 3, P, P, None, P, big, None, P, None)
        assert "uz_conv_bn_partials() == 0" in _refused(L, "uz_conv_fwd_bn_ex", rc)
    with R.dispatch_state(L, 2):
        assert L.uz_conv_route(0, C, C, N, H, W, 3) == 1 and L.uz_conv_bwd_relu_partials(C, C, N, H, W, 3) > 0
        # x_packed without its bound; the second segment: not on a chunk, beyond the view, without its bound (worded by the shared launcher)
        assert "bound" in _refused(L, "uz_conv_fwd_ex", fwd(x_amax=None), launcher=True)
        assert "multiple of 16" in _refused(L, "uz_conv_fwd_ex", fwd(a2=P, seg=8), launcher=True)
        _refused(L, "uz_conv_fwd_ex", fwd(a2=P, seg=48), launcher=True)
        _refused(L, "uz_conv_fwd_ex", fwd(a2=None, seg=16), launcher=True)
        _refused(L, "uz_conv_bwd_data_ex", bwd(y=None, dyp=1, dy_amax=None), launcher=True)
        # uz_conv_fwd_bn_ex without the activation's bound / the statistics table
        _refused(L, "uz_conv_fwd_bn_ex", fwd_bn(a_amax=None))
        _refused(L, "uz_conv_fwd_bn_ex", fwd_bn(save=None))
        # the fold: accumulating, without the table, without the partial rows
        for kw in (dict(acc=1), dict(save=None), dict(bnp=None)):
            assert "folded BatchNorm reduction" in _refused(L, "uz_conv_bwd_data_ex", bwd(**kw)), kw
        # workspace one byte short (Cin = Cout: the query is the exact need of either direction)
        short = ctypes.c_size_t(L.uz_conv_workspace(C, C, N, H, W, 3) - 1)
        assert "workspace" in _refused(L, "uz_conv_fwd_ex", fwd(ws=short))
        assert "workspace" in _refused(L, "uz_conv_fwd_bn_ex", fwd_bn(ws=short))
        assert "workspace" in _refused(L, "uz_conv_bwd_data_ex", bwd(ws=short))
        assert "workspace" in _refused(L, "uz_conv_bwd_data_ex", bwd(y=None, dyp=1, ws=short))
        # weight gradient: dy_packed with a bias gradient, a packed operand without its bound, workspace one byte short
        assert L.uz_conv_route(2, 64, 64, 8, 16, 16, 3) == 1
        assert "bias gradient" in _refused(L, "uz_conv_bwd_weight_ex", wgrad(dp=1, db=P))
        assert "bound" in _refused(L, "uz_conv_bwd_weight_ex", wgrad(xp=1, xa=None))
        assert "bound" in _refused(L, "uz_conv_bwd_weight_ex", wgrad(dp=1, da=None))
        short = ctypes.c_size_t(L.uz_conv_bwd_weight_workspace(64, 64, 8, 16, 16, 3) - 1)
        assert wgrad(xp=1, ws=short) != 0                  # worded by the dispatch shared with uz_conv_bwd_weight
        msg = L.uz_last_error().decode()
        assert msg.startswith("conv_bwd_weight") and "workspace" in msg, msg
