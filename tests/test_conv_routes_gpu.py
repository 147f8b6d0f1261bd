"""fp64 parity of every case of the convolution dispatch table (tests/_conv_routes.py), each run through the C ABI in its own math
mode on the instance tests/test_conv_routes_cpu.py proves it takes.

Inputs are structured: one channel at 2^-12 of the others, a block of rows offset by +3 against zero-mean weights (the outputs
cancel there), non-negative (post-ReLU) activations in every other case, input and output in channel-slice views of wider buffers
with NaN canaries on both sides.

Gate: elementwise, per output element e
    ratio(e) = |got - ref64| / (den(e) + floor),   den = (|a| conv |b|)(e) [+ |bias| + |accumulated value|],
the fp64 magnitude of the same sum, so that cancelling outputs, border pixels with fewer taps and a channel at 2^-12 are held to the
same relative standard as the rest.  floor = 2^-39 max|a| max|b| T (T terms per output) is split_f16.h's absolute error of an
operand below 2^-17 of its tensor bound, summed over the T products.  The worst ratio of a case must stay under GATE[(mode,
direction, route)].  Derivation (split_f16.h): a split operand v s = h1 + h2 + r with |r| <= 2^-22 |v s|; of a product the kernels
keep a1 b1 + a1 b2 + a2 b1 and drop a2 b2 <= 2^-22 |ab|, so with the two residuals a product is off by at most 3 * 2^-22 |ab| =
7.2e-7 |ab|, and the fp32 accumulation adds at most one rounding of 2^-24 of the running magnitude per addition level.  The
single-piece bf16 mode is compared with the fp64 sum of the RNE-bf16 operands: bf16 x bf16 products are exact in fp32, so only the
fp32 accumulation remains.  The fp32 MFMA kernels have the accumulation term alone.  Those bounds are worst cases over K terms;
the errors are sums of signed roundings, and the constants below are set from the MI355X (worst observed ratio of the table per
key, recorded beside each) at no more than 4x that value.  In modes 0, 1 and 2 the tensor-max relative error against fp64 must
also stay <= 2e-6 (tools/wgrad_forms_check.py's gate)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _conv_routes as R

pytestmark = pytest.mark.gpu

# worst elementwise ratio allowed per (math mode, direction, route); observed worst on the MI355X in the comment
GATE = {
    (0, "fwd", 0): 1e-6,          # 3.7e-7
    (0, "dgrad", 0): 1e-6,        # 3.4e-7
    (0, "wgrad", 0): 4e-7,        # 1.5e-7
    (1, "fwd", 0): 1e-6,          # 4.2e-7
    (1, "fwd", 1): 1.2e-6,        # 4.0e-7
    (1, "fwd", 2): 1e-6,          # 4.5e-7
    (1, "dgrad", 0): 1e-6,        # 4.3e-7
    (1, "dgrad", 1): 1.2e-6,      # 3.9e-7
    (1, "wgrad", 0): 2e-7,        # 7.0e-8
    (1, "wgrad", 1): 1.5e-7,      # 4.1e-8
    (1, "wgrad", 2): 1.5e-8,      # 4.7e-9
    (2, "fwd", 1): 1e-6,          # 3.4e-7
    (2, "dgrad", 1): 1e-6,        # 3.8e-7
    (2, "wgrad", 1): 3e-8,        # 1.1e-8
    (3, "fwd", 1): 5e-7,          # 1.5e-7
    (3, "dgrad", 0): 1e-6,        # 3.4e-7
    (3, "dgrad", 1): 5e-7,        # 1.4e-7
    (3, "wgrad", 1): 1.2e-7,      # 3.5e-8
}
TENSOR_MAX = 2e-6
BN_SUM = 1e-6          # fused BatchNorm partial sums / sums of squares against fp64 sums of the stored y, relative to sum |y| / sum y^2
WORST = {}


def _g():
    from tests import _gpu
    return _gpu


def _act(shape, seed, nonneg):
    g = _g()
    t = g.rnd(*shape, seed=seed)
    H = shape[2]
    r0 = H // 4
    t[:, :, r0:r0 + max(1, H // 4)] += 3.0          # an offset block of rows
    if shape[1] > 1:
        t[:, 1] *= 2.0 ** -12                        # a quiet channel
    return torch.relu(t) if nonneg else t


def _bf16(t):
    return t.to(torch.bfloat16).float()


def _check(case, what, got, ref, den, floor):
    """Elementwise ratio (recorded per key) and, in modes 0..2, the tensor-max relative error."""
    got = got.detach().cpu().double()
    ratio = float(((got - ref).abs() / (den + floor)).max())
    key = (case.mode, case.direction, case.claims["route"])
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= GATE[key], f"{R.case_id(case)} {what}: worst elementwise ratio {ratio:.3e} > {GATE[key]:.1e}"
    if case.mode != 3:
        rel = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
        assert rel <= TENSOR_MAX, f"{R.case_id(case)} {what}: tensor-max relative error {rel:.3e}"


def _canaries(buf, c0, c1):
    return bool(torch.isnan(buf[:, :c0]).all()) and bool(torch.isnan(buf[:, c1:]).all())


def _fwd(case, idx, L, dev):
    g = _g()
    N, Cin, Cout, H, W, ks = case.N, case.Cin, case.Cout, case.H, case.W, case.ks
    pad = ks // 2
    x = _act((N, Cin, H, W), 100 + idx, idx % 2 == 1)
    w = g.rnd(Cout, Cin, ks, ks, seed=200 + idx, scale=1.0 / math.sqrt(Cin * ks * ks))
    w[0] -= w[0].mean()                              # output channel 0 cancels on the offset block
    b = g.rnd(Cout, seed=300 + idx)
    xr, wr = (_bf16(x), _bf16(w)) if case.mode == 3 and case.claims["route"] == 1 else (x, w)
    conv = F.conv2d(xr.double(), wr.double(), None, padding=pad)
    den = F.conv2d(xr.double().abs(), wr.double().abs(), None, padding=pad)
    floor = 2.0 ** -39 * float(xr.abs().max()) * float(wr.abs().max()) * Cin * ks * ks
    ref, den_b = conv + b.double()[None, :, None, None], den + b.double().abs()[None, :, None, None]

    xbuf, xv = g.view_in(x, Cin + 5, 3)
    wd, bd = w.to(dev), b.to(dev)
    wsb = L.uz_conv_workspace(Cin, Cout, N, H, W, ks)
    ws = torch.empty(wsb // 4 + 16, device=dev)
    ybuf = torch.full((N, Cout + 4, H, W), float("nan"), device=dev)
    npart = case.claims["bn"]
    if npart > 0:                                    # plain epilogue with the fused BatchNorm partials
        part = torch.full((npart * Cout * 4,), float("nan"), device=dev)
        g.call("uz_conv_fwd_bnstats", xv, Cin, Cin + 5, wd, bd, ybuf[:, 2:], Cout, Cout + 4, N, H, W, ks, 0, None, None, None, ws, wsb, None, part)
    else:
        g.call("uz_conv_fwd", xv, Cin, Cin + 5, wd, bd, ybuf[:, 2:], Cout, Cout + 4, N, H, W, ks, 0, None, None, None, ws, wsb)
    assert _canaries(ybuf, 2, 2 + Cout), "forward wrote outside its output view"
    y = ybuf[:, 2:2 + Cout]
    _check(case, "bias", y, ref, den_b, floor)
    if npart > 0:
        y64 = y.cpu().double()
        p = part.view(npart, Cout, 4).cpu().double()
        s1, s2 = y64.sum((0, 2, 3)), (y64 * y64).sum((0, 2, 3))
        assert float(((p[:, :, 0].sum(0) - s1).abs() / y64.abs().sum((0, 2, 3))).max()) <= BN_SUM
        assert float(((p[:, :, 1].sum(0) - s2).abs() / s2).max()) <= BN_SUM
        assert torch.equal(p[:, :, 2].max(0).values, y64.amax((0, 2, 3))) and torch.equal(p[:, :, 3].max(0).values, (-y64).amax((0, 2, 3)))
    # second launch: no bias, ReLU epilogue, into a plain tensor (into the view again with the bias in every other case)
    if idx % 2:
        y2 = torch.full((N, Cout, H, W), float("nan"), device=dev)
        g.call("uz_conv_fwd", xv, Cin, Cin + 5, wd, None, y2, Cout, Cout, N, H, W, ks, 1, None, None, None, ws, wsb)
        _check(case, "relu, no bias", y2, torch.relu(conv), den, floor)
    else:
        g.call("uz_conv_fwd", xv, Cin, Cin + 5, wd, bd, ybuf[:, 2:], Cout, Cout + 4, N, H, W, ks, 1, None, None, None, ws, wsb)
        assert _canaries(ybuf, 2, 2 + Cout)
        _check(case, "relu", ybuf[:, 2:2 + Cout], torch.relu(ref), den_b, floor)


def _dgrad(case, idx, L, dev):
    g = _g()
    N, Cin, Cout, H, W, ks = case.N, case.Cin, case.Cout, case.H, case.W, case.ks
    pad = ks // 2
    dy = _act((N, Cout, H, W), 400 + idx, idx % 2 == 1)
    w = g.rnd(Cout, Cin, ks, ks, seed=500 + idx, scale=1.0 / math.sqrt(Cout * ks * ks))
    w[:, 0] -= w[:, 0].mean()                        # input channel 0 of the gradient cancels on the offset block
    prev = g.rnd(N, Cin, H, W, seed=600 + idx)
    dyr, wr = (_bf16(dy), _bf16(w)) if case.mode == 3 and case.claims["route"] == 1 else (dy, w)
    ref = F.conv_transpose2d(dyr.double(), wr.double(), None, padding=pad)
    den = F.conv_transpose2d(dyr.double().abs(), wr.double().abs(), None, padding=pad)
    floor = 2.0 ** -39 * float(dyr.abs().max()) * float(wr.abs().max()) * Cout * ks * ks

    dybuf, dyv = g.view_in(dy, Cout + 3, 2)
    wd = w.to(dev)
    wsb = L.uz_conv_workspace(Cin, Cout, N, H, W, ks)
    ws = torch.empty(wsb // 4 + 16, device=dev)
    dxbuf = torch.full((N, Cin + 3, H, W), float("nan"), device=dev)
    g.call("uz_conv_bwd_data", dyv, Cout, Cout + 3, wd, dxbuf[:, 1:], Cin, Cin + 3, N, H, W, ks, 0, None, None, ws, wsb)
    assert _canaries(dxbuf, 1, 1 + Cin), "data gradient wrote outside its output view"
    _check(case, "overwrite", dxbuf[:, 1:1 + Cin], ref, den, floor)
    dxbuf[:, 1:1 + Cin] = prev.to(dev)
    g.call("uz_conv_bwd_data", dyv, Cout, Cout + 3, wd, dxbuf[:, 1:], Cin, Cin + 3, N, H, W, ks, 1, None, None, ws, wsb)
    assert _canaries(dxbuf, 1, 1 + Cin)
    _check(case, "accumulate", dxbuf[:, 1:1 + Cin], ref + prev.double(), den + prev.double().abs(), floor)


def _wgrad(case, idx, L, dev, x=None, xv=None, CinTot=None, bitwise=True):
    g = _g()
    N, Cin, Cout, H, W, ks = case.N, case.Cin, case.Cout, case.H, case.W, case.ks
    pad = ks // 2
    if x is None:
        x = _act((N, Cin, H, W), 700 + idx, idx % 2 == 1)
        xbuf, xv = g.view_in(x, Cin + 5, 3)
        CinTot = Cin + 5
    dy = g.rnd(N, Cout, H, W, seed=800 + idx)
    if Cout > 1:
        dy[:, Cout - 1] *= 2.0 ** -12
    xr, dyr = (_bf16(x), _bf16(dy)) if case.mode == 3 and case.claims["route"] == 1 else (x, dy)
    wshape = (Cout, Cin, ks, ks)
    ref = torch.nn.grad.conv2d_weight(xr.double(), wshape, dyr.double(), padding=pad)
    den = torch.nn.grad.conv2d_weight(xr.double().abs(), wshape, dyr.double().abs(), padding=pad)
    floor = 2.0 ** -39 * float(xr.abs().max()) * float(dyr.abs().max()) * N * H * W

    dybuf, dyv = g.view_in(dy, Cout + 2, 1)
    wsb = L.uz_conv_bwd_weight_workspace(Cin, Cout, N, H, W, ks)
    ws = torch.empty(wsb // 4 + 16, device=dev)
    dw = torch.full(wshape, float("nan"), device=dev)
    db = torch.full((Cout,), float("nan"), device=dev)
    g.call("uz_conv_bwd_weight", xv, Cin, CinTot, dyv, Cout, Cout + 2, dw, db, N, H, W, ks, None, None, ws, wsb)
    _check(case, "weight gradient", dw, ref, den, floor)
    dbr = dy.double().sum((0, 2, 3))                 # the bias gradient reads dy in fp32 in every mode
    assert float(((db.cpu().double() - dbr).abs() / dy.double().abs().sum((0, 2, 3))).max()) <= 1e-6
    if bitwise:
        dw2 = torch.full(wshape, float("nan"), device=dev)
        g.call("uz_conv_bwd_weight", xv, Cin, CinTot, dyv, Cout, Cout + 2, dw2, None, N, H, W, ks, None, None, ws, wsb)
        assert torch.equal(dw, dw2), "the weight gradient is not deterministic"


def _with_mode(mode, fn):
    from unet_zoo_amd import _ffi
    L = _ffi.lib()
    with R.dispatch_state(L, mode):
        fn(L)


GPU_CASES = [(i, c) for i, c in enumerate(R.CASES) if c.gpu]


@pytest.mark.parametrize("idx,case", GPU_CASES, ids=[R.case_id(c) for _, c in GPU_CASES])
def test_route_case_against_fp64(idx, case):
    dev = _g().dev()

    def run(L):
        assert R.queries(L, case) == case.claims, "the case left its route (tests/test_conv_routes_cpu.py)"
        {"fwd": _fwd, "dgrad": _dgrad, "wgrad": _wgrad}[case.direction](case, idx, L, dev)
    _with_mode(case.mode, run)


def test_weight_gradient_of_a_view_into_a_buffer_of_two_to_the_thirty_elements():
    """The `huge` branch of the weight-gradient dispatch (conv_wgrad.hip: a buffer of >= 2^30 elements leaves the 32-bit-offset
    kernels for the generic one with 64-bit pointers): an 8-channel view at the far end of a 2^30-element input buffer, the
    reference over the view alone."""
    if torch.cuda.mem_get_info()[0] < 16 * 2 ** 30:
        pytest.skip("needs 16 GiB of free device memory")
    g = _g()
    dev = g.dev()
    N, Cin, Cout, H, W = 2, 8, 16, 4, 8               # 8 x 4 tiles with two images per tile: the generic tiled kernel, not a fast one
    CinTot = 2 ** 30 // (N * H * W) + 16
    case = R.R("wgrad", 1, N, Cin, Cout, H, W, 3, route=0, slabs=None)
    x = _act((N, Cin, H, W), 900, False)
    xbuf = torch.full((N, CinTot, H, W), float("nan"), device=dev)
    c0 = CinTot - Cin - 3
    xbuf[:, c0:c0 + Cin] = x.to(dev)

    def run(L):
        assert L.uz_conv_route(2, Cin, Cout, N, H, W, 3) == 0
        _wgrad(case, 900, L, dev, x=x, xv=xbuf[:, c0:], CinTot=CinTot)
    _with_mode(1, run)
    del xbuf
    torch.cuda.empty_cache()


def test_zz_report_worst_ratios(capsys):
    """Lists the worst elementwise ratio per (math mode, direction, route) seen by the cases above (run with them)."""
    with capsys.disabled():
        print("\nworst elementwise |got - ref64| / (|a| conv |b| + floor) per (mode, direction, route):")
        for k in sorted(WORST):
            print(f"  {k}: {WORST[k]:.3e}  (gate {GATE[k]:.1e})")
