"""The depth-window dispatch table (tests/_conv3d_routes.py) without a GPU: every case takes the routes it claims, every kernel
family with window-specific code is claimed by a case the GPU tier runs, the cases tell the five addressing defects apart by
more than 100 gates, and the five refusals a window call can meet are decided on the host."""
import ctypes

import pytest
import torch

from tests import _conv3d_routes as V
from tests import _conv_routes as R
from tests.test_conv_routes_gpu import GATE


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib()


def _gate(c, direction):
    key = (c.mode, direction, getattr(c, direction)["route"])
    return V.WINDOW_GATE.get(key, GATE[V.GATE_ALIAS.get(key, key)])


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_case_takes_the_routes_it_claims(case):
    L = _lib()
    with R.dispatch_state(L, case.mode):
        got = V.queries(L, case)
    claims = {d: getattr(case, d) for d in V.directions(case)}
    assert got == claims, f"{V.case_id(case)}: claims {claims}, the dispatch answers {got}"


def test_every_window_specific_kernel_family_has_a_gpu_case():
    ids = [V.case_id(c) for c in V.CASES]
    assert len(ids) == len(set(ids))
    gpu = [c for _, c in V.GPU_CASES]
    assert all(len(V.directions(c)) == 3 for c in gpu)

    def some(pred):
        return any(pred(c) for c in gpu)
    # fp32 MFMA without and with batch tiles (pick_wgeom: planes of <= 16 pixels share a tile between images), per direction
    for d in V.DIRECTIONS:
        assert some(lambda c: getattr(c, d)["route"] == 0 and c.H * c.W > 16 and c.D > 1), d
        assert some(lambda c: getattr(c, d)["route"] == 0 and c.H * c.W <= 16 and c.D > 2), d
    # split kernels with the chunk loop whole and shared out, forward and data gradient
    for d in ("fwd", "dgrad"):
        assert some(lambda c: getattr(c, d)["route"] == 1 and getattr(c, d)["parts"] == 1), d
        assert some(lambda c: getattr(c, d)["route"] == 1 and getattr(c, d)["parts"] > 1), d
    # thin forward and thin weight gradient: a 1-channel volume (Cin = 3)
    assert some(lambda c: c.fwd["route"] == 2 and c.C == 1) and some(lambda c: c.wgrad["route"] == 2 and c.C == 1)
    # split weight gradient on the 32- and the 64-channel tile (chan_tile: both sides <= 32 / one beyond), and W = 16
    assert some(lambda c: c.wgrad["route"] == 1 and max(3 * c.C, c.Cout) <= 32 and c.W % 32 == 0)
    assert some(lambda c: c.wgrad["route"] == 1 and max(3 * c.C, c.Cout) > 32 and c.W % 32 == 0)
    assert some(lambda c: c.wgrad["route"] == 1 and c.W == 16)
    # more than 64 slabs (two-stage reduce in front of the volC write) on both weight-gradient kernels
    assert some(lambda c: c.wgrad["route"] == 0 and c.wgrad["slabs"] > 64 and c.mode == 0)
    assert some(lambda c: c.wgrad["route"] == 1 and c.wgrad["slabs"] > 64)
    # bf16 with the 128-channel tile, and every direction of the bf16 mode on its matrix-pipe route
    assert some(lambda c: c.mode == 3 and c.fwd["route"] == 1 and c.fwd["cot"] == 128)
    for d in V.DIRECTIONS:
        assert some(lambda c: c.mode == 3 and getattr(c, d)["route"] == 1), d


def test_the_window_reference_is_the_conv3d_of_the_materialised_window():
    """The reference the defects are variations of: F.conv3d equals the 2-D convolution of the materialised window with the
    [co][kd][ci] weights - the formulation the kernels implement - to fp64 rounding."""
    idx = next(i for i, c in V.GPU_CASES if (c.mode, c.C, c.D) == (0, 6, 2))
    x, w = V.ref_operands(idx, "fwd")
    D, C = x.shape[:2]
    pad = torch.zeros(D + 2, *x.shape[1:], dtype=x.dtype)
    pad[1:-1] = x
    win = torch.cat([pad[kd:kd + D] for kd in range(3)], 1)
    w2d = w.permute(0, 2, 1, 3, 4).reshape(w.shape[0], 3 * C, 3, 3)
    y = torch.nn.functional.conv2d(win, w2d, None, padding=1)
    assert float((y - V.conv3d("fwd", x, w)).abs().max()) <= 1e-13


PROOFS = [(i, c, d) for i, c, d in V.GPU_RUNS]


@pytest.mark.parametrize("idx,case,direction", PROOFS, ids=[f"{V.case_id(c)}-{d}" for _, c, d in PROOFS])
def test_the_case_tells_every_defect_apart(idx, case, direction):
    """Each defective evaluation of the fp64 reference differs from the true one by more than 100 gates at some element, so a
    kernel with that defect cannot pass the case on the GPU.  (The three cases of 262 144 px or more are proved on their first
    four slices: the window never looks further than one slice, and an fp64 Conv3d of the whole case takes a CPU too long.)"""
    slices = V.PROOF_SLICES if case.D * case.H * case.W >= 262144 else None
    a, b = V.ref_operands(idx, direction, slices)
    true = V.conv3d(direction, a, b)
    den = V.conv3d(direction, a.abs(), b.abs())
    floor = V.floor_of(case, direction, a, b, slices)
    bound = 100.0 * _gate(case, direction) * (den + floor)
    for n in V.defects_of(direction):
        bad = V.DEFECTS[n](direction, a, b)
        if V.defect_is_identity(n, case, direction):
            assert torch.equal(bad, true), f"defect {n} was expected to change nothing here"
            continue
        worst = float(((bad - true).abs() / bound).max())
        assert worst > 1.0, f"{V.case_id(case)} {direction}: defect {n} moves no element by more than 100 gates (worst {worst:.2e})"


# ----------------------------------------------------------------------------- refusals decided on the host
P = 1 << 20          # a non-null address: no refused call may touch it


def _refused(L, name, rc):
    msg = L.uz_last_error().decode() if isinstance(L.uz_last_error(), bytes) else str(L.uz_last_error())
    assert rc != 0, f"{name} accepted the call"
    assert name[3:] in msg, f"{name}: uz_last_error does not name the entry point: {msg!r}"
    return msg


def test_the_refusals_of_a_window_call_are_decided_on_the_host():
    L = _lib()
    big = ctypes.c_size_t(1 << 40)
    with R.dispatch_state(L, 3):
        # uz_conv_fwd_b16 on a window whose chunk loop is shared out (parts 2): no bf16-storage form
        C, Co, D, H, W = 32, 32, 40, 16, 16
        assert L.uz_conv_route(0, 3 * C, Co, D, H, W, 3) == 1 and L.uz_conv_split_parts(0, 3 * C, Co, D, H, W) == 2
        msg = _refused(L, "uz_conv_fwd_b16", L.uz_conv_fwd_b16(P, 3 * C, C, P, None, P, Co, Co, D, H, W, 3, P, big, None, None, 1, 1, None))
        assert "unsplit" in msg
        # uz_conv_bwd_weight_b16 on 16-wide rows (on the matrix-pipe path, but off the bf16-storage loads)
        C, Co, D, H, W = 22, 64, 8, 16, 16
        assert L.uz_conv_route(2, 3 * C, Co, D, H, W, 3) == 1
        _refused(L, "uz_conv_bwd_weight_b16", L.uz_conv_bwd_weight_b16(P, 3 * C, C, P, Co, Co, P, D, H, W, 3, P, big, 1, 1, None, None))
        # uz_conv_bwd_weight_ex with an operand in split storage: two-piece mode only
        C, Co, D, H, W = 11, 32, 8, 128, 128
        assert L.uz_conv_route(2, 3 * C, Co, D, H, W, 3) == 1
        _refused(L, "uz_conv_bwd_weight_ex", L.uz_conv_bwd_weight_ex(P, 3 * C, C, P, Co, Co, P, None, D, H, W, 3, P, P, P, big, 1, None, 0, 0, None, None))
    with R.dispatch_state(L, 2):
        # uz_conv_bwd_weight_b16 outside the single-piece bf16 mode
        C, Co, D, H, W = 11, 40, 3, 8, 32
        assert L.uz_conv_route(2, 3 * C, Co, D, H, W, 3) == 1
        _refused(L, "uz_conv_bwd_weight_b16", L.uz_conv_bwd_weight_b16(P, 3 * C, C, P, Co, Co, P, D, H, W, 3, P, big, 1, 1, None, None))
        # uz_conv_bwd_weight_ex leaving its slabs for the table launch and asked for a bias gradient
        assert L.uz_conv_bwd_weight_slabs(3 * C, Co, D, H, W, 3) > 0
        _refused(L, "uz_conv_bwd_weight_ex", L.uz_conv_bwd_weight_ex(P, 3 * C, C, P, Co, Co, P, P, D, H, W, 3, None, None, P, big, 0, None, 0, 0, P, None))
