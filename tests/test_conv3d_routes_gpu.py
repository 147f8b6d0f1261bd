"""Every GPU case of the depth-window dispatch table (tests/_conv3d_routes.py) through the C ABI, in its own math mode, on the
instance tests/test_conv3d_routes_cpu.py proves it takes - Conv3d(3x3x3, pad 1) as the 2-D kernels with Cin = 3 C view channels
over a CinTot = C channel buffer (include/uz_api.h, volumes section).

Buffers: a window operand lives in one allocation [1 + (D + 2) + 1][C][H][W] whose first and last slice are NaN and whose second
and second-to-last slice are the contract's zero slices; the pointer passed is the first zero slice.  A read outside the D + 2
slices poisons the output.  Outputs go into channel-slice views of wider NaN-filled buffers whose canaries must survive.

Two gates per direction:
  * against the fp64 F.conv3d reference with the elementwise ratio and the GATE of tests/test_conv_routes_gpu.py (same kernels,
    same arithmetic, so no gate of its own; the three (mode, direction, route 0) keys the 2-D table never met take the mode-0
    gate of their direction, GATE_ALIAS - they run the fp32 MFMA kernels on un-rounded operands);
  * bit for bit against the plain 2-D call on the MATERIALISED window x2d[d, kd C + ci] = vol[d - 1 + kd, ci] (CinTot = 3 C).
    The kernels do not know the difference, so an inequality is an addressing defect.
The CPU tier proves that each of the five addressing defects of _conv3d_routes.py moves every case by more than 100 gates."""
import pytest
import torch

from tests import _conv3d_routes as V
from tests import _conv_routes as R
from tests import test_conv_routes_gpu as T

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST = {}
TWIN = {}          # the same ratios of the materialised 2-D twin, where it is held to fp64 itself (weight gradient)


def _g():
    from tests import _gpu
    return _gpu


def _lib():
    from unet_zoo_amd import _ffi
    return _ffi.lib()


def _check(case, direction, what, got, ref, den, floor, worst=WORST):
    """tests/test_conv_routes_gpu._check under the key's gate (GATE_ALIAS; WINDOW_GATE where this table has a gate of its own), the
    worst ratio recorded in this file's own table."""
    key = (case.mode, direction, getattr(case, direction)["route"])
    gk = V.GATE_ALIAS.get(key, key)
    saved, gate = dict(T.WORST), T.GATE[gk]
    T.WORST.pop(gk, None)
    T.GATE[gk] = V.WINDOW_GATE.get(key, gate)
    try:
        T._check(V.as2d(case, direction)._replace(mode=gk[0]), what, got, ref, den, floor)
    finally:
        ratio = T.WORST.get(gk)
        T.GATE[gk] = gate
        T.WORST.clear()
        T.WORST.update(saved)
        if ratio is not None:
            worst[key] = max(worst.get(key, 0.0), ratio)


def _guarded(t, dev, dtype=torch.float32):
    """[D][C][H][W] -> (allocation [NaN, 0, the D slices, 0, NaN], the view a window call is handed: from the first zero slice)."""
    D = t.shape[0]
    buf = torch.full((D + 4, *t.shape[1:]), NAN, device=dev, dtype=dtype)
    buf[1] = 0
    buf[D + 2] = 0
    buf[2:D + 2] = t.to(dev).to(dtype)
    return buf, buf[1:]


def _window(buf, D):
    """The materialised window of a guarded allocation: [D][3 C][H][W] with channel kd C + ci = slice d - 1 + kd, channel ci."""
    return torch.cat([buf[1 + kd:1 + kd + D] for kd in range(3)], 1).contiguous()


def _canaries(buf, c0, c1):
    return bool(torch.isnan(buf[:, :c0]).all()) and bool(torch.isnan(buf[:, c1:]).all())


def _permuted(w, mode, dev):
    """uz_w3d_permute of a [Cout][C][3][3][3] parameter (modes 0, 1) or of a [Cout][3][C][3][3] window-layout gradient (mode 2)."""
    Co, C = (w.shape[0], w.shape[2]) if mode == 2 else w.shape[:2]
    wp = torch.full((Co * C * 27,), NAN, device=dev)
    _g().call("uz_w3d_permute", w, wp, Co, C, mode)
    return wp


def _ws(nbytes, dev):
    return torch.empty(nbytes // 4 + 64, device=dev)


# ----------------------------------------------------------------------------- the three directions
def _fwd(idx, case, L, dev):
    g = _g()
    C, Co, D, H, W = case.C, case.Cout, case.D, case.H, case.W
    x, w = V.operands(idx, "fwd")
    b = V.operands(idx, "bias")
    conv, den, floor = V.reference(idx, "fwd")
    bb = b.double()[None, :, None, None]
    xbuf, xv = _guarded(x, dev)
    x2d = _window(xbuf, D)
    wd, bd = w.to(dev), b.to(dev)
    wp = _permuted(wd, 0, dev)
    wsb = L.uz_conv_workspace(3 * C, Co, D, H, W, 3)
    ws = _ws(wsb, dev)
    npart = case.fwd["bn"]

    def run(xp, ctot, bias, relu, bn):
        ybuf = torch.full((D, Co + 4, H, W), NAN, device=dev)
        part = torch.full((npart * Co * 4,), NAN, device=dev) if bn else None
        if bn:
            g.call("uz_conv_fwd_bnstats", xp, 3 * C, ctot, wp, bias, ybuf[:, 2:], Co, Co + 4, D, H, W, 3, relu, None, None, None, ws, wsb, None, part)
        else:
            g.call("uz_conv_fwd", xp, 3 * C, ctot, wp, bias, ybuf[:, 2:], Co, Co + 4, D, H, W, 3, relu, None, None, None, ws, wsb)
        assert _canaries(ybuf, 2, 2 + Co), "forward wrote outside its output view"
        return ybuf[:, 2:2 + Co], part

    # bias, plain epilogue, with the fused BatchNorm partials where the shape has them
    y, part = run(xv, C, bd, 0, npart > 0)
    _check(case, "fwd", "bias", y, conv + bb, den + bb.abs(), floor)
    if npart > 0:
        y64 = y.cpu().double()
        p = part.view(npart, Co, 4).cpu().double()
        s1, s2 = y64.sum((0, 2, 3)), (y64 * y64).sum((0, 2, 3))
        assert float(((p[:, :, 0].sum(0) - s1).abs() / y64.abs().sum((0, 2, 3))).max()) <= T.BN_SUM
        assert float(((p[:, :, 1].sum(0) - s2).abs() / s2).max()) <= T.BN_SUM
        assert torch.equal(p[:, :, 2].max(0).values, y64.amax((0, 2, 3))) and torch.equal(p[:, :, 3].max(0).values, (-y64).amax((0, 2, 3)))
    y2, part2 = run(x2d, 3 * C, bd, 0, npart > 0)
    assert torch.equal(y, y2), "the window call differs from the 2-D call on the materialised window"
    assert part is None or torch.equal(part, part2), "... in its BatchNorm partials"
    # ReLU epilogue: without the bias in every other case
    if idx % 2:
        y, _ = run(xv, C, None, 1, False)
        _check(case, "fwd", "relu, no bias", y, torch.relu(conv), den, floor)
        y2, _ = run(x2d, 3 * C, None, 1, False)
    else:
        y, _ = run(xv, C, bd, 1, False)
        _check(case, "fwd", "relu", y, torch.relu(conv + bb), den + bb.abs(), floor)
        y2, _ = run(x2d, 3 * C, bd, 1, False)
    assert torch.equal(y, y2), "the window call differs from the 2-D call on the materialised window (ReLU epilogue)"


def _dgrad(idx, case, L, dev):
    g = _g()
    C, Co, D, H, W = case.C, case.Cout, case.D, case.H, case.W
    dy, w = V.operands(idx, "dgrad")
    prev = V.operands(idx, "prev")
    ref, den, floor = V.reference(idx, "dgrad")
    dybuf, dyv = _guarded(dy, dev)
    dy2d = _window(dybuf, D)
    wp = _permuted(w.to(dev), 1, dev)
    wsb = L.uz_conv_workspace(C, 3 * Co, D, H, W, 3)
    ws = _ws(wsb, dev)
    prevd = prev.to(dev)

    def run(dyp, ctot):
        dxbuf = torch.full((D, C + 3, H, W), NAN, device=dev)
        g.call("uz_conv_bwd_data", dyp, 3 * Co, ctot, wp, dxbuf[:, 1:], C, C + 3, D, H, W, 3, 0, None, None, ws, wsb)
        assert _canaries(dxbuf, 1, 1 + C), "data gradient wrote outside its output view"
        over = dxbuf[:, 1:1 + C].clone()
        dxbuf[:, 1:1 + C] = prevd
        g.call("uz_conv_bwd_data", dyp, 3 * Co, ctot, wp, dxbuf[:, 1:], C, C + 3, D, H, W, 3, 1, None, None, ws, wsb)
        assert _canaries(dxbuf, 1, 1 + C)
        return over, dxbuf[:, 1:1 + C]

    over, acc = run(dyv, Co)
    _check(case, "dgrad", "overwrite", over, ref, den, floor)
    _check(case, "dgrad", "accumulate", acc, ref + prev.double(), den + prev.double().abs(), floor)
    over2, acc2 = run(dy2d, 3 * Co)
    assert torch.equal(over, over2) and torch.equal(acc, acc2), "the window call differs from the 2-D call on the materialised dy window"


def _wgrad_operands(idx, case, dev):
    g = _g()
    x, dy = V.operands(idx, "wgrad")
    xbuf, xv = _guarded(x, dev)
    dybuf, dyv = g.view_in(dy, case.Cout + 2, 1)
    return x, dy, xbuf, xv, dybuf, dyv


def _wgrad(idx, case, L, dev):
    g = _g()
    C, Co, D, H, W = case.C, case.Cout, case.D, case.H, case.W
    x, dy, xbuf, xv, dybuf, dyv = _wgrad_operands(idx, case, dev)
    ref, den, floor = V.reference(idx, "wgrad")
    wsb = L.uz_conv_bwd_weight_workspace(3 * C, Co, D, H, W, 3)
    ws = _ws(wsb, dev)
    dw = torch.full((Co, C, 3, 3, 3), NAN, device=dev)
    db = torch.full((Co,), NAN, device=dev)
    g.call("uz_conv_bwd_weight", xv, 3 * C, C, dyv, Co, Co + 2, dw, db, D, H, W, 3, None, None, ws, wsb)
    # the 2-D call on the materialised window leaves [co][kd][ci]; uz_w3d_permute mode 2 brings it to the parameter layout
    x2d = _window(xbuf, D)
    dw2d = torch.full((Co, 3 * C, 3, 3), NAN, device=dev)
    g.call("uz_conv_bwd_weight", x2d, 3 * C, 3 * C, dyv, Co, Co + 2, dw2d, None, D, H, W, 3, None, None, ws, wsb)
    twin = _permuted(dw2d.view(Co, 3, C, 3, 3), 2, dev).view_as(dw)
    same = bool(torch.equal(dw, twin))
    # the twin against fp64 under the same gate: what tells arithmetic (both off alike) from addressing (the window alone)
    _check(case, "wgrad", "weight gradient of the materialised window", twin, ref, den, floor, worst=TWIN)
    _check(case, "wgrad", "weight gradient (Conv3d layout)", dw, ref, den, floor)
    assert same, "the window call differs from the 2-D call on the materialised window"
    dbr = dy.double().sum((0, 2, 3))
    assert float(((db.cpu().double() - dbr).abs() / dy.double().abs().sum((0, 2, 3))).max()) <= 1e-6
    dw2 = torch.full_like(dw, NAN)
    g.call("uz_conv_bwd_weight", xv, 3 * C, C, dyv, Co, Co + 2, dw2, None, D, H, W, 3, None, None, ws, wsb)
    assert torch.equal(dw, dw2), "the weight gradient is not deterministic"


RUN = {"fwd": _fwd, "dgrad": _dgrad, "wgrad": _wgrad}


@pytest.mark.parametrize("idx,case,direction", V.GPU_RUNS, ids=[f"{V.case_id(c)}-{d}" for _, c, d in V.GPU_RUNS])
def test_window_case_against_fp64_and_the_materialised_2d_call(idx, case, direction):
    L, dev = _lib(), _g().dev()
    with R.dispatch_state(L, case.mode):
        assert V.queries(L, case) == {d: getattr(case, d) for d in V.directions(case)}, "the case left its route (tests/test_conv3d_routes_cpu.py)"
        RUN[direction](idx, case, L, dev)


# ----------------------------------------------------------------------------- pack images read from the Conv3d parameter
PACK_CASES = [(i, c) for i, c in V.GPU_CASES if c.fwd["route"] == 1 or c.dgrad["route"] == 1]


@pytest.mark.parametrize("mode", (2, 3), ids=("split", "bf16"))
@pytest.mark.parametrize("idx,case", PACK_CASES, ids=[V.case_id(c) for _, c in PACK_CASES])
def test_pack_images_from_the_conv3d_parameter(idx, case, mode):
    """One uz_conv_pack_weights launch, four rows per layer: forward and data gradient read from the Conv3d parameter (flags bit 1,
    wCi = C) and from the uz_w3d_permute mode-0 / mode-1 outputs (plain rows, wCi = 3 C / C).  The two images of a direction are
    byte-equal, and uz_conv_fwd_packed / uz_conv_bwd_data_packed with the Conv3d-sourced image equal the window call that packs
    its own - in the two-piece mode (NP = 2) and in the bf16 mode (NP = 1), wherever that mode runs the shape on route 1."""
    g, L, dev = _g(), _lib(), _g().dev()
    C, Co, D, H, W = case.C, case.Cout, case.D, case.H, case.W
    with R.dispatch_state(L, mode):
        wd = V.operands(idx, "fwd")[1].to(dev)
        bound = torch.zeros(256, device=dev)
        g.call("uz_absmax", wd, wd.numel(), bound)
        wp0, wp1 = _permuted(wd, 0, dev), _permuted(wd, 1, dev)
        # (w, flags, Mc, Kc, wCi), then the 2-D (Cin, Cout) the size queries take
        spec = [(wd, 2, Co, 3 * C, C, 3 * C, Co), (wd, 3, C, 3 * Co, C, C, 3 * Co),
                (wp0, 0, Co, 3 * C, 3 * C, 3 * C, Co), (wp1, 1, C, 3 * Co, C, C, 3 * Co)]
        imgs, table, rows = [], [], 0
        for wsrc, flags, mc, kc, wci, ci2, co2 in spec:
            img = torch.zeros(L.uz_conv_packed_bytes(ci2, co2, W, flags & 1) + 64, dtype=torch.uint8, device=dev)
            table += [wsrc.data_ptr(), img.data_ptr(), mc, kc, wci, L.uz_conv_pack_cot(ci2, co2, W, flags & 1), flags, rows]
            rows += L.uz_conv_pack_rows(ci2, co2, W, flags & 1)
            imgs.append(img)
        g.call("uz_conv_pack_weights", torch.tensor(table, dtype=torch.int64, device=dev), 4, rows, bound)
        assert bool(imgs[0].any()) and bool(imgs[1].any())
        assert torch.equal(imgs[0], imgs[2]), "forward image read from the Conv3d parameter differs from the permuted weights' image"
        assert torch.equal(imgs[1], imgs[3]), "data-gradient image read from the Conv3d parameter differs from the permuted weights' image"
        ran = 0
        if L.uz_conv_route(0, 3 * C, Co, D, H, W, 3) == 1:
            xbuf, xv = _guarded(V.operands(idx, "fwd")[0], dev)
            wsb = L.uz_conv_workspace(3 * C, Co, D, H, W, 3)
            ws = _ws(wsb, dev)
            y0, y1 = (torch.full((D, Co, H, W), NAN, device=dev) for _ in range(2))
            g.call("uz_conv_fwd", xv, 3 * C, C, wp0, None, y0, Co, Co, D, H, W, 3, 0, None, bound, None, ws, wsb)
            g.call("uz_conv_fwd_packed", xv, 3 * C, C, wd, None, y1, Co, Co, D, H, W, 3, 0, None, bound, None, ws, wsb, imgs[0])
            assert torch.equal(y0, y1) and not bool(torch.isnan(y0).any())
            ran += 1
        if L.uz_conv_route(1, C, 3 * Co, D, H, W, 3) == 1:
            dybuf, dyv = _guarded(V.operands(idx, "dgrad")[0], dev)
            wsb = L.uz_conv_workspace(C, 3 * Co, D, H, W, 3)
            ws = _ws(wsb, dev)
            d0, d1 = (torch.full((D, C, H, W), NAN, device=dev) for _ in range(2))
            g.call("uz_conv_bwd_data", dyv, 3 * Co, Co, wp1, d0, C, C, D, H, W, 3, 0, None, bound, ws, wsb)
            g.call("uz_conv_bwd_data_packed", dyv, 3 * Co, Co, wd, d1, C, C, D, H, W, 3, 0, None, bound, ws, wsb, imgs[1])
            assert torch.equal(d0, d1) and not bool(torch.isnan(d0).any())
            ran += 1
        assert ran > 0 or mode == 3, "mode 2 runs every such shape on the split kernels"


# ----------------------------------------------------------------------------- slabs left for the table launch
TABLE_CASES = [(i, c) for i, c in V.GPU_CASES if c.wgrad["slabs"] > 64 and c.mode in (0, 2)] + \
              [(i, c) for i, c in V.GPU_CASES if (c.mode, c.C, c.Cout, c.W) == (2, 11, 40, 32)]


@pytest.mark.parametrize("idx,case", TABLE_CASES, ids=[V.case_id(c) for _, c in TABLE_CASES])
def test_window_slabs_reduced_by_the_table_launch(idx, case):
    """uz_conv_bwd_weight_ex(slabs_out) + uz_wgrad_reduce_table with volC = C: the two cases with more than 64 slabs (two-stage
    order) and a split case on the 64-channel tile.  Bit-equal to the call's own reduction, and checked against fp64."""
    g, L, dev = _g(), _lib(), _g().dev()
    C, Co, D, H, W = case.C, case.Cout, case.D, case.H, case.W
    assert len(TABLE_CASES) == 3
    with R.dispatch_state(L, case.mode):
        S = L.uz_conv_bwd_weight_slabs(3 * C, Co, D, H, W, 3)
        assert S == case.wgrad["slabs"] and L.uz_conv_route(2, 3 * C, Co, D, H, W, 3) == case.wgrad["route"]
        x, dy, xbuf, xv, dybuf, dyv = _wgrad_operands(idx, case, dev)
        wsb = L.uz_conv_bwd_weight_workspace(3 * C, Co, D, H, W, 3)
        ws = _ws(wsb, dev)
        dw0 = torch.full((Co, C, 3, 3, 3), NAN, device=dev)
        g.call("uz_conv_bwd_weight", xv, 3 * C, C, dyv, Co, Co + 2, dw0, None, D, H, W, 3, None, None, ws, wsb)
        slabs = torch.full((S * 9 * Co * 3 * C,), NAN, device=dev)
        dw1 = torch.full_like(dw0, NAN)
        g.call("uz_conv_bwd_weight_ex", xv, 3 * C, C, dyv, Co, Co + 2, dw1, None, D, H, W, 3, None, None, ws, wsb, 0, None, 0, 0, slabs)
        assert bool(torch.isnan(dw1).all()), "the call with slabs_out wrote dw"
        table = torch.tensor([slabs.data_ptr(), dw1.data_ptr(), S, Co, 3 * C, 9, 0, C], dtype=torch.int64, device=dev)
        g.call("uz_wgrad_reduce_table", table, 1, L.uz_wgrad_reduce_blocks(3 * C, Co, 3))
        assert torch.equal(dw0, dw1), "the table launch differs from the call's own reduction"
        ref, den, floor = V.reference(idx, "wgrad")
        _check(case, "wgrad", "table reduction", dw1, ref, den, floor)


# ----------------------------------------------------------------------------- bf16 storage on a window
B16_CASES = [(i, c) for i, c in V.GPU_CASES if c.mode == 3]


def _rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


@pytest.mark.parametrize("idx,case", B16_CASES, ids=[V.case_id(c) for _, c in B16_CASES])
def test_bf16_storage_on_a_window(idx, case):
    """The *_b16 convolutions on a depth window, as equalities (tests/test_b16_storage_gpu.py): the oracle is the fp32-storage window
    call on the same bf16-representable values.  A bf16-stored input gives the same bits, a bf16-stored output their rounding."""
    g, L, dev = _g(), _lib(), _g().dev()
    C, Co, D, H, W = case.C, case.Cout, case.D, case.H, case.W
    bf = torch.bfloat16
    ran = 0
    with R.dispatch_state(L, 3):
        assert V.queries(L, case) == {d: getattr(case, d) for d in V.directions(case)}
        if case.fwd["route"] == 1:
            ran += 1
            npart = case.fwd["bn"]
            assert npart > 0 and case.fwd["parts"] == 1
            x, w = V.operands(idx, "fwd")
            x = _rb(x)
            bd = V.operands(idx, "bias").to(dev)
            wp = _permuted(w.to(dev), 0, dev)
            b32, v32 = _guarded(x, dev)
            b16, v16 = _guarded(x, dev, bf)
            wsb = L.uz_conv_workspace(3 * C, Co, D, H, W, 3)
            ws = _ws(wsb, dev)
            y_ref = torch.full((D, Co + 4, H, W), NAN, device=dev)
            p_ref = torch.full((npart * Co * 4,), NAN, device=dev)
            g.call("uz_conv_fwd_bnstats", v32, 3 * C, C, wp, bd, y_ref[:, 2:], Co, Co + 4, D, H, W, 3, 0, None, None, None, ws, wsb, None, p_ref)
            y_a, p_a = torch.full_like(y_ref, NAN), torch.full_like(p_ref, NAN)
            g.call("uz_conv_fwd_b16", v16, 3 * C, C, wp, bd, y_a[:, 2:], Co, Co + 4, D, H, W, 3, ws, wsb, None, p_a, 1, 0)
            assert _canaries(y_a, 2, 2 + Co) and not bool(torch.isnan(y_ref[:, 2:2 + Co]).any())
            assert torch.equal(y_a[:, 2:2 + Co], y_ref[:, 2:2 + Co]) and torch.equal(p_a, p_ref)
            y_b = torch.full((D, Co + 4, H, W), NAN, device=dev, dtype=bf)
            p_b = torch.full_like(p_ref, NAN)
            g.call("uz_conv_fwd_b16", v16, 3 * C, C, wp, bd, y_b[:, 2:], Co, Co + 4, D, H, W, 3, ws, wsb, None, p_b, 1, 1)
            assert _canaries(y_b, 2, 2 + Co)
            assert torch.equal(y_b[:, 2:2 + Co], y_ref[:, 2:2 + Co].to(bf))
            pb = p_b.view(npart, Co, 4).double().cpu()               # the statistics are those of the STORED values
            ys = y_b[:, 2:2 + Co].float().double().cpu()
            assert float(((pb[:, :, 0].sum(0) - ys.sum((0, 2, 3))).abs() / ys.abs().sum((0, 2, 3))).max()) <= T.BN_SUM
            assert float(((pb[:, :, 1].sum(0) - (ys * ys).sum((0, 2, 3))).abs() / (ys * ys).sum((0, 2, 3))).max()) <= T.BN_SUM
            assert torch.equal(pb[:, :, 2].max(0).values, ys.amax((0, 2, 3))) and torch.equal(pb[:, :, 3].max(0).values, (-ys).amax((0, 2, 3)))
            y_c = torch.full_like(y_b, NAN)                          # bf16 output from the fp32 volume
            g.call("uz_conv_fwd_b16", v32, 3 * C, C, wp, bd, y_c[:, 2:], Co, Co + 4, D, H, W, 3, ws, wsb, None, None, 0, 1)
            assert torch.equal(y_c[:, 2:2 + Co], y_b[:, 2:2 + Co])
        if case.wgrad["route"] == 1:
            ran += 1
            x, dy = V.operands(idx, "wgrad")
            x, dy = _rb(x), _rb(dy)
            xb32, x32 = _guarded(x, dev)
            xb16, x16 = _guarded(x, dev, bf)
            dyb32, dy32 = g.view_in(dy, Co + 3, 0)
            dyb16 = dyb32.to(bf)
            dy16 = dyb16[:, 0:]
            wsb = L.uz_conv_bwd_weight_workspace(3 * C, Co, D, H, W, 3)
            ws = _ws(wsb, dev)
            dw_ref = torch.full((Co, C, 3, 3, 3), NAN, device=dev)
            g.call("uz_conv_bwd_weight", x32, 3 * C, C, dy32, Co, Co + 3, dw_ref, None, D, H, W, 3, None, None, ws, wsb)
            assert not bool(torch.isnan(dw_ref).any())
            same = {}
            for xb, db in ((0, 0), (1, 0), (0, 1), (1, 1)):
                dw = torch.full_like(dw_ref, NAN)
                g.call("uz_conv_bwd_weight_b16", x16 if xb else x32, 3 * C, C, dy16 if db else dy32, Co, Co + 3, dw, D, H, W, 3, ws, wsb, xb, db, None)
                same[(xb, db)] = bool(torch.equal(dw, dw_ref))
            assert all(same.values()), same
        if case.dgrad["route"] == 1:
            ran += 1
            assert case.dgrad["parts"] == 1
            dy, w = V.operands(idx, "dgrad")
            dy = _rb(dy)
            wp = _permuted(w.to(dev), 1, dev)
            b32, v32 = _guarded(dy, dev)
            b16, v16 = _guarded(dy, dev, bf)
            wsb = L.uz_conv_workspace(C, 3 * Co, D, H, W, 3)
            ws = _ws(wsb, dev)
            dx_ref = torch.full((D, C + 3, H, W), NAN, device=dev)
            g.call("uz_conv_bwd_data", v32, 3 * Co, Co, wp, dx_ref[:, 1:], C, C + 3, D, H, W, 3, 0, None, None, ws, wsb)
            ref = dx_ref[:, 1:1 + C]
            assert not bool(torch.isnan(ref).any())
            dx_a = torch.full_like(dx_ref, NAN)                      # bf16 dy window, fp32 dx: the same bits
            g.call("uz_conv_bwd_data_b16", v16, 3 * Co, Co, wp, dx_a[:, 1:], C, C + 3, D, H, W, 3, 0, ws, wsb, None, 1, 0)
            assert _canaries(dx_a, 1, 1 + C) and torch.equal(dx_a[:, 1:1 + C], ref)
            dx_b = torch.full((D, C + 3, H, W), NAN, device=dev, dtype=bf)
            g.call("uz_conv_bwd_data_b16", v16, 3 * Co, Co, wp, dx_b[:, 1:], C, C + 3, D, H, W, 3, 0, ws, wsb, None, 1, 1)
            assert _canaries(dx_b, 1, 1 + C) and torch.equal(dx_b[:, 1:1 + C], ref.to(bf))
            base = _rb(V.operands(idx, "prev")).to(dev)
            dx_b[:, 1:1 + C] = base.to(bf)                           # accumulate onto a bf16 tensor: round(stored + new)
            g.call("uz_conv_bwd_data_b16", v16, 3 * Co, Co, wp, dx_b[:, 1:], C, C + 3, D, H, W, 3, 1, ws, wsb, None, 1, 1)
            assert _canaries(dx_b, 1, 1 + C) and torch.equal(dx_b[:, 1:1 + C], (ref + base).to(bf))
    assert ran > 0


def test_zz_report_worst_ratios(capsys):
    """Lists the worst elementwise ratio per (math mode, direction, route) seen by the window cases above (run with them)."""
    with capsys.disabled():
        print("\ndepth windows: worst elementwise |got - ref64| / (|a| conv |b| + floor) per (mode, direction, route):")
        for k in sorted(WORST):
            gk = V.GATE_ALIAS.get(k, k)
            gate = V.WINDOW_GATE.get(k, T.GATE[gk])
            twin = f", 2-D twin {TWIN[k]:.3e}" if k in TWIN else ""
            print(f"  {k}: {WORST[k]:.3e}  (gate {gate:.1e}{', of this table' if k in V.WINDOW_GATE else '' if gk == k else f', that of {gk}'}{twin})")
