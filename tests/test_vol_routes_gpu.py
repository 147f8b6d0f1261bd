"""Every case of the volume dispatch table (tests/_vol_routes.py) through the C ABI against an fp64 evaluation of the same operation
on the same fp32 operands: F.avg_pool3d(ceil_mode=True), trilinear interpolation with align_corners=True along the depth (in-plane
scale 1: the identity), nearest interpolation, autograd for the backward passes.  Every operand is a channel-slice view of a volume
[D][C + 2][H][W] inside a NaN-filled allocation (tests/_views.py): everything outside a view must keep its bits.

Gates are those of tests/test_phiseg3d.py::test_avgpool3d_trilinear_nearest_vs_torch, absolute bounds on max |got - ref| as there:
pooling 1e-6 (2e-6 where the call accumulates into prior contents), depth interpolation 2e-6 forward and 1e-5 backward, nearest
forward exact, nearest backward 1e-5 on the thread kernel.  The wave kernel of the nearest backward sums 64 and more children per
element; its gate there was 1e-5 PER CHILD, loose enough to hide a dropped child.  Here it is 4 x the error of torch's own fp32
CPU backward against the same fp64 reference on the same input, both relative to max(1, max |ref|)
(tests/_vol_routes.py NEAREST_WAVE_TORCH32, recomputed by tests/test_vol_routes_cpu.py; the kernel's butterfly order
differs from torch's sequential one, hence the factor - the one tests/test_stream_routes_gpu.py uses), plus one fp32 rounding
(2^-24) where the call accumulates into prior contents.  The permutations and conversions are exact."""
import pytest
import torch

from tests import _vol_routes as R

pytestmark = pytest.mark.gpu

GATE = dict(pool=1e-6, pool_accumulate=2e-6, lerp_fwd=2e-6, lerp_bwd=1e-5, nearest_bwd=1e-5)          # absolute: max |got - ref|
B16_ROUND = 2.0 ** -8


def _g():
    from tests import _gpu
    return _gpu


def _v():
    from tests import _views
    return _views


_rnd = R.rnd          # the operands nearest_torch32_error measured the wave gate on


def _rb(t):
    return t.to(torch.bfloat16).float()


def _nan(*shape):
    return torch.full(shape, float("nan"))


def _close(got, ref, gate, what, b16=False, relative=False):
    """max |got - ref| <= gate; relative: of max(1, max |ref|) (the wave kernel's gate is measured that way)."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if b16:                                          # one bf16 rounding of the stored element on top
        assert bool(((got - ref).abs() <= ref.abs() * B16_ROUND + gate).all()), what
        return
    err = float((got - ref).abs().max()) / (max(1.0, float(ref.abs().max())) if relative else 1.0)
    print(f"{what}: {'relative' if relative else 'absolute'} error {err:.3e} (gate {gate:g})")
    assert err <= gate, f"{what}: error {err:.3e} exceeds {gate:g}"      # (NaN fails too)


_ref_fn, _grad = R.ref_fn, R.grad


def _align(v):
    p = v.ptr.data_ptr()
    return 16 if p % 16 == 0 else 8 if p % 8 == 0 else 4


def _check_route(c, src, dst):
    assert R.queries(_g().L(), c) == c.claims, "the case left its route (tests/test_vol_routes_cpu.py)"
    assert (_align(src), _align(dst)) == R.alignments(c)


GPU_CASES = [c for c in R.CASES if c.gpu]


@pytest.mark.parametrize("case", GPU_CASES, ids=R.case_id)
def test_case_against_fp64(case):
    c, g, V = case, _g(), _v()
    C, D, H, W = c.C, c.D, c.H, c.W
    b16 = c.op == "lerp_b16"
    dt = torch.bfloat16 if b16 else torch.float32
    fn = _ref_fn(c)
    x = _rnd(D, C, H, W, seed=1)
    x = _rb(x) if b16 else x
    ref = fn(x.double())
    dy = _rnd(*ref.shape, seed=2)
    dy = _rb(dy) if b16 else dy
    prev = _rnd(D, C, H, W, seed=3)
    prev = _rb(prev) if b16 else prev
    gref = _grad(fn, x, dy)
    # ---- forward
    xv, yv = V.View(x, c.off[0], c0=R.C0, dtype=dt), V.View(_nan(*ref.shape), c.off[1], c0=R.C0, dtype=dt)
    _check_route(c, xv, yv)
    if c.op == "pool":
        g.call("uz_avgpool3d_fwd", xv.ptr, C, xv.ctot, yv.ptr, yv.ctot, D, H, W)
        _close(yv.get(), ref, GATE["pool"], "avgpool3d_fwd")
    elif c.op == "lerp":
        g.call("uz_depth_lerp2x_fwd", xv.ptr, C, xv.ctot, yv.ptr, yv.ctot, D, H, W)
        _close(yv.get(), ref, GATE["lerp_fwd"], "depth_lerp2x_fwd")
    elif b16:
        g.call("uz_depth_lerp2x_fwd_b16", xv.ptr, C, xv.ctot, yv.ptr, yv.ctot, D, H, W, 1, 1)
        _close(yv.get(), ref, GATE["lerp_fwd"], "depth_lerp2x_fwd_b16", b16=True)
    else:
        g.call("uz_nearest3d_fwd", xv.ptr, C, xv.ctot, yv.ptr, yv.ctot, D, H, W, c.f, c.fz)
        assert torch.equal(yv.get(), ref.float()), "nearest3d_fwd is not exact"
    assert xv.untouched() and yv.outside_untouched()
    del yv
    # ---- backward, overwriting and accumulating
    dyv = V.View(dy, c.off[1], c0=R.C0, dtype=dt)
    wave = c.op == "nearest" and c.claims["bwd"][0] == R.WAVE
    for accumulate in (0, 1):
        dxv = V.View(prev if accumulate else _nan(D, C, H, W), c.off[0], c0=R.C0, dtype=dt)
        want = gref + prev.double() if accumulate else gref
        what = f"{c.op} backward accumulate={accumulate}"
        if c.op == "pool":
            g.call("uz_avgpool3d_bwd", dyv.ptr, C, dyv.ctot, dxv.ptr, dxv.ctot, D, H, W, accumulate)
            _close(dxv.get(), want, GATE["pool_accumulate" if accumulate else "pool"], what)
        elif c.op == "lerp":
            g.call("uz_depth_lerp2x_bwd", dyv.ptr, C, dyv.ctot, dxv.ptr, dxv.ctot, D, H, W, accumulate)
            _close(dxv.get(), want, GATE["lerp_bwd"], what)
        elif b16:
            g.call("uz_depth_lerp2x_bwd_b16", dyv.ptr, C, dyv.ctot, dxv.ptr, dxv.ctot, D, H, W, accumulate, 1, 1)
            _close(dxv.get(), want, GATE["lerp_bwd"], what, b16=True)
        else:
            g.call("uz_nearest3d_bwd", dyv.ptr, C, dyv.ctot, dxv.ptr, dxv.ctot, D, H, W, c.f, c.fz, accumulate)
            gate = GATE["nearest_bwd"]
            if wave:
                gate = 4 * R.NEAREST_WAVE_TORCH32[(c.f, c.fz)] + (2.0 ** -24 if accumulate else 0.0)
            _close(dxv.get(), want, gate, what + (" (wave kernel)" if wave else ""), relative=wave)
        assert dxv.outside_untouched()
    assert dyv.untouched()


@pytest.mark.parametrize("mode", R.PERMUTE_MODES)
@pytest.mark.parametrize("Cout,Cin,groups", R.PERMUTE_CASES)
def test_weight_permutation_is_exact(Cout, Cin, groups, mode):
    g, V = _g(), _v()
    assert R.query(g.L(), 10, Cout, Cin, 1, 1, 1, 1, 16, 16) == (R.SCALAR, groups)
    n = Cout * Cin * 27
    src = torch.arange(n, dtype=torch.float32) - 0.5 * n                                   # every element distinct and exact in fp32
    if mode == 0:                                                                           # [co][ci][kd][9] -> [co][kd][ci][9]
        ref = src.view(Cout, Cin, 3, 9).permute(0, 2, 1, 3)
    elif mode == 1:                                                                         # -> [j][co][ci][9], kd = 2 - j
        ref = src.view(Cout, Cin, 3, 9).flip(2).permute(2, 0, 1, 3)
    else:                                                                                   # [co][kd][ci][9] -> [co][ci][kd][9]
        ref = src.view(Cout, 3, Cin, 9).permute(0, 2, 1, 3)
    sv, dv = V.Flat((n,), 4, src), V.Flat((n,), 4)
    g.call("uz_w3d_permute", sv.ptr, dv.ptr, Cout, Cin, mode)
    assert torch.equal(dv.get(), ref.reshape(-1)) and dv.outside_untouched() and sv.untouched()


def _cvt_input(n):
    """Normal values, and in front the cases of round-to-nearest-even: ties towards an even and an odd upper half, just below and above
    a tie, a carry into the exponent, overflow to infinity, subnormals, signed zeros and infinities."""
    x = _rnd(n, seed=1) * 3
    bits = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFF8000, 0x7F7F8000, 0x7F7F7FFF, 0x00008000, 0x00018000, 0x00000001,
            0x00000000, 0x7F800000]
    bits = bits + [b | 0x80000000 for b in bits]
    sp = torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    return x


@pytest.mark.parametrize("n,groups", R.CVT_CASES)
def test_conversions_round_to_nearest_even_bit_for_bit(n, groups):
    g, V = _g(), _v()
    if n:
        assert R.query(g.L(), 11, n, 1, 1, 1, 1, 1, 16, 16) == (R.SCALAR, groups)
    x = _cvt_input(n)
    want = x.to(torch.bfloat16)
    sv, hv = V.Flat((n,), 4, x), V.Flat((n,), 8, dtype=torch.bfloat16)
    ptr = (lambda t: t.ptr) if n else (lambda t: t.flat)          # (an empty view has no address: n = 0 gets the allocation, and must not touch it)
    g.call("uz_cvt_f32_to_b16", ptr(sv), ptr(hv), n)
    assert torch.equal(hv.ptr.view(torch.int16).cpu(), want.view(torch.int16)) and hv.outside_untouched() and sv.untouched()
    back = V.Flat((n,), 4)
    g.call("uz_cvt_b16_to_f32", ptr(hv), ptr(back), n)
    assert torch.equal(back.ptr.view(torch.int32).cpu(), want.float().view(torch.int32)) and back.outside_untouched()
