"""Every case of the heads dispatch table (tests/_head_routes.py) through the C ABI against an fp64 evaluation of the same operation
on the same fp32 operands (F.conv2d / F.conv_transpose2d in double, softplus / exp and the sample in double).  Every tensor operand
is a view inside a NaN-filled allocation (tests/_views.py): everything outside a view must keep its bits.

Gates (tests/test_ops_gpu.py's, relative to the largest reference magnitude): 2e-5 for the values and gradients of a 1x1 head - the
large-sum weight gradients included, which flush fp32 into fp64 every 32 steps (measured values print under -s); for the latent
heads 2e-6 for the forward and the data gradient and 1e-5 for the weight and bias gradients.  A bf16-stored data gradient is held
to one bf16 rounding (2^-8 of the element) on top.  Weight gradients and the channel-parallel forward run twice and must repeat
their bits; the sequential latent forward equals the separate ops (uz_conv_fwd x 2 + uz_latent_sample_fwd) bit for bit; accumulate
= 1 equals the prior contents plus the gradient; a refused call returns an error and leaves its outputs' NaNs in place.  The
output counts the streaming kernels do not cover run the fp32 MFMA kernels (dispatch_state(L, 0))."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _conv_routes as CR
from tests import _head_routes as R

pytestmark = pytest.mark.gpu

C1_GATE = 2e-5
LAT_FWD_GATE, LAT_DGRAD_GATE, LAT_WGRAD_GATE = 2e-6, 2e-6, 1e-5


def _g():
    from tests import _gpu
    return _gpu


def _v():
    from tests import _views
    return _views


def _rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def _rb(t):
    return t.to(torch.bfloat16).float()


def _err(got, ref, what, gate):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    print(f"{what}: error {err:.3e} of max |ref| (gate {gate:g})")
    assert err <= gate, f"{what}: error {err:.3e} of max |ref| exceeds {gate:g}"      # (NaN fails too)


def _operands(c):
    return _operands_of(R.case_id(c))


@functools.lru_cache(maxsize=2)
def _operands_of(cid):
    """fp32 CPU operands of a case, shared by its three directions (weights of variance 1 / Cin: outputs of unit scale)."""
    c = next(k for k in R.CASES if R.case_id(k) == cid)
    N, Cin, Co, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    x = _rnd(N, Cin, H, W, seed=1)
    if c.kind == "c1_b16":
        x = _rb(x)
    o = dict(x=x, prev=_rnd(N, Cin, H, W, seed=9))
    if c.kind == "lat":
        o.update(wa=_rnd(Co, Cin, 1, 1, seed=2, scale=Cin ** -0.5), wb=_rnd(Co, Cin, 1, 1, seed=3, scale=Cin ** -0.5), ba=_rnd(Co, seed=4), bb=_rnd(Co, seed=5),
                 eps=_rnd(N, Co, H, W, seed=6), dya=_rnd(N, Co, H, W, seed=7), dyb=_rnd(N, Co, H, W, seed=8))
    else:
        o.update(w=_rnd(Co, Cin, 1, 1, seed=2, scale=Cin ** -0.5), b=_rnd(Co, seed=3), dy=_rnd(N, Co, H, W, seed=4))
    return o


def _cases(direction, kinds):
    cs = [c for c in R.CASES if c.kind in kinds and direction in c.claims]
    return pytest.mark.parametrize("case", cs, ids=[R.case_id(c) for c in cs])


def _wide(c, t):
    """The many-channel operand of a case as the table places it (module docstring of tests/_head_routes.py)."""
    if c.kind == "c1_b16":
        return _v().View(t, R.B16_LEAD + c.off[0], c0=0, dtype=torch.bfloat16)
    return _v().View(t, c.off[0], c0=R.C0)


def _nan(*shape):
    return torch.full(shape, float("nan"))


def _check_route(c, direction, *views):
    """The case still launches what it claims, and the views are aligned as the table told the query."""
    assert R.queries(_g().L(), c)[direction] == c.claims[direction], "the case left its route (tests/test_head_routes_cpu.py)"
    assert all(v.aligned() for v in views) == R.aligned(c)


def _mfma(c, direction):
    return c.claims[direction][0] == R.MFMA


def _Mode(on):
    """dispatch_state(L, 0) around a case the MFMA kernels run; nothing for the streaming kernels, which do not read the math mode."""
    return CR.dispatch_state(_g().L(), 0) if on else contextlib.nullcontext()


# ------------------------------------------------------------------------------ the 1x1 heads
@_cases("fwd", ("c1", "c1_b16"))
def test_head_forward_against_fp64(case):
    c, g, V = case, _g(), _v()
    N, Cin, Co, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    o = _operands(c)
    bias = o["b"] if R.opt(c, "bias", 1) else None
    ref = F.conv2d(o["x"].double(), o["w"].double(), bias.double() if bias is not None else None)
    xv, yv = _wide(c, o["x"]), V.View(_nan(N, Co, H, W), c.off[1], c0=R.C0)
    _check_route(c, "fwd", xv, yv)
    wd, bd = o["w"].to(g.dev()), bias.to(g.dev()) if bias is not None else None
    if c.kind == "c1_b16":
        g.call("uz_conv1x1_fwd_b16", xv.ptr, Cin, xv.ctot, wd, bd, yv.ptr, Co, yv.ctot, N, H, W, 1)
    else:
        wsb = g.L().uz_conv_workspace(Cin, Co, N, H, W, 1)
        ws = torch.empty(wsb // 4 + 16, device=g.dev())
        with _Mode(_mfma(c, "fwd")):
            g.call("uz_conv_fwd", xv.ptr, Cin, xv.ctot, wd, bd, yv.ptr, Co, yv.ctot, N, H, W, 1, 0, None, None, None, ws, wsb)
    _err(yv.get(), ref, "forward", C1_GATE)
    assert xv.untouched() and yv.outside_untouched()


@_cases("dgrad", ("c1", "c1_b16"))
def test_head_data_gradient_against_fp64(case):
    c, g, V = case, _g(), _v()
    N, Cin, Co, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    o = _operands(c)
    b16 = c.kind == "c1_b16"
    prev = _rb(o["prev"]) if b16 else o["prev"]
    gref = F.conv_transpose2d(o["dy"].double(), o["w"].double())
    dyv = V.View(o["dy"], c.off[1], c0=R.C0)
    wd = o["w"].to(g.dev())
    wsb = g.L().uz_conv_workspace(Cin, Co, N, H, W, 1)
    ws = torch.empty(wsb // 4 + 16, device=g.dev())
    for accumulate in (0, 1):
        dxv = _wide(c, prev if accumulate else _nan(N, Cin, H, W))
        _check_route(c, "dgrad", dyv, dxv)
        if b16:
            g.call("uz_conv1x1_bwd_data_b16", dyv.ptr, Co, dyv.ctot, wd, dxv.ptr, Cin, dxv.ctot, N, H, W, accumulate, 1)
        else:
            with _Mode(_mfma(c, "dgrad")):
                g.call("uz_conv_bwd_data", dyv.ptr, Co, dyv.ctot, wd, dxv.ptr, Cin, dxv.ctot, N, H, W, 1, accumulate, None, None, ws, wsb)
        ref = gref + prev.double() if accumulate else gref
        if b16:                                      # one bf16 rounding of the stored element on top of the fp32 gate
            got = dxv.get().double()
            assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -8 + C1_GATE * float(ref.abs().max())).all())
        else:
            _err(dxv.get(), ref, f"data gradient accumulate={accumulate}", C1_GATE)
        assert dxv.outside_untouched()
    assert dyv.untouched()


@_cases("wgrad", ("c1", "c1_b16"))
def test_head_weight_gradient_against_fp64(case):
    c, g, V = case, _g(), _v()
    N, Cin, Co, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    o = _operands(c)
    ref = torch.einsum("nohw,nchw->oc", o["dy"].double(), o["x"].double()).view(Co, Cin, 1, 1)
    dbref = o["dy"].double().sum((0, 2, 3))
    xv, dyv = _wide(c, o["x"]), V.View(o["dy"], c.off[1], c0=R.C0)
    _check_route(c, "wgrad", xv, dyv)
    wsb = g.L().uz_conv_bwd_weight_workspace(Cin, Co, N, H, W, 1)
    ws = torch.empty(wsb // 4 + 16, device=g.dev())
    want_db = R.opt(c, "db", 1)
    runs = []
    for _ in range(2):
        dw, db = V.Flat((Co, Cin, 1, 1), R.GUARD), V.Flat((Co,), R.GUARD)
        dbp = db.ptr if want_db else None
        if c.kind == "c1_b16":
            g.call("uz_conv1x1_bwd_weight_b16", xv.ptr, Cin, xv.ctot, dyv.ptr, Co, dyv.ctot, dw.ptr, dbp, N, H, W, ws, wsb, 1)
        else:
            with _Mode(_mfma(c, "wgrad")):
                g.call("uz_conv_bwd_weight", xv.ptr, Cin, xv.ctot, dyv.ptr, Co, dyv.ctot, dw.ptr, dbp, N, H, W, 1, None, None, ws, wsb)
        assert dw.outside_untouched() and db.outside_untouched()
        assert want_db or db.untouched()
        runs.append((dw.get(), db.get()))
    _err(runs[0][0], ref, f"weight gradient of {N * H * W} pixels", C1_GATE)
    if want_db:
        _err(runs[0][1], dbref, "bias gradient", C1_GATE)
    assert torch.equal(runs[0][0], runs[1][0]), "the weight gradient does not repeat its bits"
    assert not want_db or torch.equal(runs[0][1], runs[1][1])
    assert xv.untouched() and dyv.untouched()


def test_an_uncovered_head_leaves_its_weight_gradient_slabs():
    """5 outputs at ks = 1: uz_conv_bwd_weight_slabs now answers the MFMA kernels' slab count, so the slabs_out form of the call is
    accepted (it was refused while the query said 'no slabs'), and the slabs add up to the weight gradient."""
    g, V = _g(), _v()
    N, Cin, Co, H, W = 2, 38, 5, 16, 16
    x, dy = _rnd(N, Cin, H, W, seed=1), _rnd(N, Co, H, W, seed=2)
    ref = torch.einsum("nohw,nchw->oc", dy.double(), x.double())
    xv, dyv = V.View(x, 0), V.View(dy, 0)
    L = g.L()
    with CR.dispatch_state(L, 0):
        S = L.uz_conv_bwd_weight_slabs(Cin, Co, N, H, W, 1)
        assert S >= 1
        wsb = L.uz_conv_bwd_weight_workspace(Cin, Co, N, H, W, 1)
        ws = torch.empty(wsb // 4 + 16, device=g.dev())
        slabs = V.Flat((S, Co, Cin), R.GUARD)
        g.call("uz_conv_bwd_weight_ex", xv.ptr, Cin, xv.ctot, dyv.ptr, Co, dyv.ctot, None, None, N, H, W, 1, None, None, ws, wsb,
               0, None, 0, 0, slabs.ptr)
    assert slabs.outside_untouched()
    _err(slabs.get().double().sum(0), ref, f"sum of {S} slabs", C1_GATE)


# ------------------------------------------------------------------------------ the latent heads
def _lat_params(c, o, dev):
    bias = R.opt(c, "bias", 1)
    return (o["wa"].to(dev), o["wb"].to(dev), o["ba"].to(dev) if bias else None, o["bb"].to(dev) if bias else None)


def _lat_reference(c, o):
    bias = R.opt(c, "bias", 1)
    mu = F.conv2d(o["x"].double(), o["wa"].double(), o["ba"].double() if bias else None)
    pre = F.conv2d(o["x"].double(), o["wb"].double(), o["bb"].double() if bias else None)
    sigma = torch.exp(pre) if R.opt(c, "act", 0) else F.softplus(pre)
    return mu, pre, sigma, mu + sigma * o["eps"].double()


def _lat_forward(c, o, hv):
    """One uz_latent_heads_fwd call of the case into fresh NaN-filled outputs."""
    g, V = _g(), _v()
    N, Cin, Lc, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    wa, wb, ba, bb = _lat_params(c, o, g.dev())
    with_z = R.opt(c, "z", 1)
    off = R.GUARD + c.off[1]
    outs = [V.Flat((N, Lc, H, W), off) for _ in range(4)]          # mu, pre_sigma, sigma, z
    eps = V.Flat((N, Lc, H, W), off, o["eps"])
    g.call("uz_latent_heads_fwd", hv.ptr, Cin, hv.ctot, wa, ba, wb, bb, eps.ptr if with_z else None, outs[0].ptr, outs[1].ptr, outs[2].ptr,
           outs[3].ptr if with_z else None, Lc, N, H, W, R.opt(c, "act", 0))
    assert all(t.outside_untouched() for t in outs) and eps.untouched() and (with_z or outs[3].untouched())
    return outs, eps


@_cases("fwd", ("lat",))
def test_latent_heads_forward_against_fp64(case, monkeypatch):
    c, g = case, _g()
    N, Cin, Lc, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    monkeypatch.delenv("UZ_HEADS_PAR", raising=False)
    o = _operands(c)
    refs = _lat_reference(c, o)
    with_z, act = R.opt(c, "z", 1), R.opt(c, "act", 0)
    hv = _wide(c, o["x"])
    outs, eps = _lat_forward(c, o, hv)
    _check_route(c, "fwd", hv, *(outs if with_z else outs[:3]), *([eps] if with_z else []))
    for name, t, ref in list(zip(("mu", "pre_sigma", "sigma", "z"), outs, refs))[:4 if with_z else 3]:
        _err(t.get(), ref, name, LAT_FWD_GATE)
    if c.claims["fwd"][0] == R.PAR:                                  # the fixed binary tree over channel groups repeats its bits
        again, _ = _lat_forward(c, o, hv)
        assert all(torch.equal(a.get(), b.get()) for a, b in list(zip(outs, again))[:4 if with_z else 3])
    # the sequential form equals the ops it replaces bit for bit
    monkeypatch.setenv("UZ_HEADS_PAR", "0")
    seq, _ = _lat_forward(c, o, hv)
    wa, wb, ba, bb = _lat_params(c, o, g.dev())
    d = g.dev()
    mu0, pre0, sg0, z0 = (torch.full((N, Lc, H, W), float("nan"), device=d) for _ in range(4))
    wsb = g.L().uz_conv_workspace(Cin, Lc, N, H, W, 1)
    ws = torch.empty(wsb // 4 + 16, device=d)
    g.call("uz_conv_fwd", hv.ptr, Cin, hv.ctot, wa, ba, mu0, Lc, Lc, N, H, W, 1, 0, None, None, None, ws, wsb)
    g.call("uz_conv_fwd", hv.ptr, Cin, hv.ctot, wb, bb, pre0, Lc, Lc, N, H, W, 1, 0, None, None, None, ws, wsb)
    g.call("uz_latent_sample_fwd", mu0 if with_z else None, pre0, o["eps"].to(d) if with_z else None, sg0, z0 if with_z else None, mu0.numel(), act)
    for name, a, b in list(zip(("mu", "pre_sigma", "sigma", "z"), seq, (mu0, pre0, sg0, z0)))[:4 if with_z else 3]:
        assert torch.equal(a.get(), b.cpu()), f"{name}: the fused sequential forward differs from the separate ops"
    assert hv.untouched()


@_cases("dgrad", ("lat",))
def test_latent_heads_data_gradient_against_fp64(case):
    c, g, V = case, _g(), _v()
    N, Cin, Lc, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    o = _operands(c)
    gref = F.conv_transpose2d(o["dya"].double(), o["wa"].double()) + F.conv_transpose2d(o["dyb"].double(), o["wb"].double())
    off = R.GUARD + c.off[1]
    dya, dyb = V.Flat((N, Lc, H, W), off, o["dya"]), V.Flat((N, Lc, H, W), off, o["dyb"])
    wa, wb = o["wa"].to(g.dev()), o["wb"].to(g.dev())
    for accumulate in (0, 1):
        dhv = _wide(c, o["prev"] if accumulate else _nan(N, Cin, H, W))
        _check_route(c, "dgrad", dya, dyb, dhv)
        g.call("uz_latent_heads_bwd_data", dya.ptr, dyb.ptr, Lc, wa, wb, dhv.ptr, Cin, dhv.ctot, N, H, W, accumulate)
        _err(dhv.get(), gref + o["prev"].double() if accumulate else gref, f"data gradient accumulate={accumulate}", LAT_DGRAD_GATE)
        assert dhv.outside_untouched()
    assert dya.untouched() and dyb.untouched()


@_cases("wgrad", ("lat",))
def test_latent_heads_weight_gradient_against_fp64(case):
    c, g, V = case, _g(), _v()
    N, Cin, Lc, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    o = _operands(c)
    refs = [torch.einsum("nohw,nchw->oc", o[k].double(), o["x"].double()).view(Lc, Cin, 1, 1) for k in ("dya", "dyb")]
    dbrefs = [o[k].double().sum((0, 2, 3)) for k in ("dya", "dyb")]
    off = R.GUARD + c.off[1]
    hv, dya, dyb = _wide(c, o["x"]), V.Flat((N, Lc, H, W), off, o["dya"]), V.Flat((N, Lc, H, W), off, o["dyb"])
    _check_route(c, "wgrad", hv, dya, dyb)
    wsb = g.L().uz_latent_heads_bwd_weight_workspace(Cin, Lc, N, H, W)
    ws = torch.empty(wsb // 8 + 8, dtype=torch.float64, device=g.dev())
    want_db = R.opt(c, "db", 1)
    runs = []
    for _ in range(2):
        dws, dbs = [V.Flat((Lc, Cin, 1, 1), R.GUARD) for _ in range(2)], [V.Flat((Lc,), R.GUARD) for _ in range(2)]
        g.call("uz_latent_heads_bwd_weight", hv.ptr, Cin, hv.ctot, dya.ptr, dyb.ptr, Lc, dws[0].ptr, dbs[0].ptr if want_db else None,
               dws[1].ptr, dbs[1].ptr if want_db else None, N, H, W, ws, wsb)
        assert all(t.outside_untouched() for t in dws + dbs) and (want_db or all(t.untouched() for t in dbs))
        runs.append([t.get() for t in dws + dbs])
    for i, head in enumerate("ab"):
        _err(runs[0][i], refs[i], f"weight gradient of head {head}", LAT_WGRAD_GATE)
        if want_db:
            _err(runs[0][2 + i], dbrefs[i], f"bias gradient of head {head}", LAT_WGRAD_GATE)
    for a, b in list(zip(runs[0], runs[1]))[:4 if want_db else 2]:
        assert torch.equal(a, b), "the weight gradient does not repeat its bits"
    assert hv.untouched() and dya.untouched() and dyb.untouched()


# ------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kind,N,Cin,Co,H,W", R.REFUSED)
def test_a_refused_call_returns_an_error_and_writes_nothing(kind, N, Cin, Co, H, W):
    g, V = _g(), _v()
    d = g.dev()
    Lo = max(Co, 1)                                                  # (L = 0: the operands still need a shape)
    ws = V.Flat((4096,), R.GUARD, dtype=torch.float64)
    w = _rnd(Lo, Cin, 1, 1, seed=2).to(d)
    if kind == "lat":
        hv = V.View(_rnd(N, Cin, H, W, seed=1), 0)
        t = [V.Flat((N, Lo, H, W), R.GUARD) for _ in range(4)]
        eps = V.Flat((N, Lo, H, W), R.GUARD, _rnd(N, Lo, H, W, seed=3))
        assert V.rc("uz_latent_heads_fwd", hv.ptr, Cin, hv.ctot, w, None, w, None, eps.ptr, t[0].ptr, t[1].ptr, t[2].ptr, t[3].ptr, Co, N, H, W, 0) != 0
        assert all(x.untouched() for x in t)
        dhv = V.View(_nan(N, Cin, H, W), 0)
        assert V.rc("uz_latent_heads_bwd_data", eps.ptr, eps.ptr, Co, w, w, dhv.ptr, Cin, dhv.ctot, N, H, W, 0) != 0
        assert dhv.untouched()
        dw = [V.Flat((Lo, Cin), R.GUARD) for _ in range(2)]
        assert V.rc("uz_latent_heads_bwd_weight", hv.ptr, Cin, hv.ctot, eps.ptr, eps.ptr, Co, dw[0].ptr, None, dw[1].ptr, None, N, H, W, ws.ptr, 8 * 4096) != 0
        assert all(x.untouched() for x in dw) and ws.untouched()
    else:
        xv = V.View(_rb(_rnd(N, Cin, H, W, seed=1)), R.B16_LEAD, c0=0, dtype=torch.bfloat16)
        yv = V.View(_nan(N, Co, H, W), 0)
        assert V.rc("uz_conv1x1_fwd_b16", xv.ptr, Cin, xv.ctot, w, None, yv.ptr, Co, yv.ctot, N, H, W, 1) != 0
        assert yv.untouched()
        dyv = V.View(_rnd(N, Co, H, W, seed=4), 0)
        dxv = V.View(_nan(N, Cin, H, W), R.B16_LEAD, c0=0, dtype=torch.bfloat16)
        assert V.rc("uz_conv1x1_bwd_data_b16", dyv.ptr, Co, dyv.ctot, w, dxv.ptr, Cin, dxv.ctot, N, H, W, 0, 1) != 0
        assert dxv.untouched()
        dw = V.Flat((Co, Cin), R.GUARD)
        assert V.rc("uz_conv1x1_bwd_weight_b16", xv.ptr, Cin, xv.ctot, dyv.ptr, Co, dyv.ctot, dw.ptr, None, N, H, W, ws.ptr, 8 * 4096, 1) != 0
        assert dw.untouched() and ws.untouched()
    assert g.L().uz_last_error()
