"""Every case of the streaming dispatch table (tests/_stream_routes.py) through the C ABI against an fp64 evaluation of the same
operation on the same fp32 inputs (torch.nn.functional in double, autograd for the backward passes; the reference's own
formulas for KL, residual CE and Adam).  Operands of the resampling ops and of uz_add_views are channel-slice views inside
NaN-filled allocations: everything outside a view must keep its bits.  Gates are the ones tests/test_ops_gpu.py states for each
op, taken relative to max(1, max |ref|); nearest_fwd, bcast_fwd and the argmax labels are exact."""
import pytest
import torch
import torch.nn.functional as F

from tests import _stream_routes as R

pytestmark = pytest.mark.gpu

GATE = dict(pool=1e-6, bilinear_fwd=2e-6, bilinear_bwd=1e-5, nearest_bwd=1e-4, kl=1e-5, kl_grad=2e-5, ce=1e-5, ce_grad=2e-6,
            adam=1e-6, norms=1e-6, norms_bwd=1e-5, softmax=1e-6)
# align_corners=True on wide planes: the source coordinate scale * o is an fp32 product of magnitude ~ W, so its fraction - the
# interpolation weight - carries ~ W 2^-23 of error against fp64 whatever computes it.  These three cases miss 2e-6 by that rounding
# alone; their gate is 4 x the error of torch's own fp32 CPU op against the same fp64 reference on the same input (measured
# 5.488e-06 at 4 x 128, 8.807e-06 at 4 x 132, 5.463e-06 at 33 x 66; align_corners=False, scale 0.5 exactly: 9e-08, gate unchanged).
BILINEAR_FWD_AC_GATE = {(4, 128): 4 * 5.488e-06, (4, 132): 4 * 8.807e-06, (33, 66): 4 * 5.463e-06}


def _g():
    from tests import _gpu
    return _gpu


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).float()


def _close(got, ref, gate, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.numel() == 0:
        return
    err = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    print(f"{what}: error {err:.3e} (gate {gate:g})")
    assert err <= gate, f"{what}: error {err:.3e} of max(1, max |ref|) exceeds {gate:g}"      # (NaN fails too)


class View:
    """An NCHW tensor as channels [C0, C0 + C) of a buffer of C + 2 channels that starts `off` floats into a NaN-filled allocation."""

    def __init__(self, t, off, align=None):
        g = _g()
        n, c, h, w = t.shape
        size = n * (c + 2) * h * w
        self.flat = torch.full((size + 4,), float("nan"), device=g.dev())
        self.body = self.flat[off:off + size].view(n, c + 2, h, w)
        self.body[:, R.C0:R.C0 + c] = t.to(g.dev())
        self.c, self.ctot = c, c + 2
        self.ptr = self.body[:, R.C0:]
        inside = torch.zeros(size + 4, dtype=torch.bool, device=g.dev())
        inside[off:off + size].view(n, c + 2, h, w)[:, R.C0:R.C0 + c] = True
        self.outside = ~inside
        self.before = self.flat.clone()
        assert self.flat.data_ptr() % 16 == 0
        if align is not None:                      # the table's alignment claim is what the dispatch will see
            p = self.ptr.data_ptr()
            assert (16 if p % 16 == 0 else 8 if p % 8 == 0 else 4) == align, (p % 16, align)

    def get(self):
        return self.body[:, R.C0:R.C0 + self.c].cpu()

    def outside_untouched(self):
        return torch.equal(self.flat.view(torch.int32)[self.outside], self.before.view(torch.int32)[self.outside])

    def untouched(self):
        return torch.equal(self.flat.view(torch.int32), self.before.view(torch.int32))


def _pool_ref(x):
    return F.avg_pool2d(x, 2, 2, 0, ceil_mode=True)


def _bil_ref(x, ac):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=bool(ac))


def _grad(fn, x, dy):
    xd = x.double().requires_grad_(True)
    fn(xd).backward(dy.double())
    return xd.grad


def _run_fwd(c, name, ref_fn, gate, extra):
    g = _g()
    al = R.alignments(c)
    x = _rnd(c.N, c.C, c.H, c.W, seed=1)
    ref = ref_fn(x.double())
    xv = View(x, c.off[0], al[0])
    yv = View(torch.full(ref.shape, float("nan")), c.off[1], al[1])
    g.call(name, xv.ptr, c.C, xv.ctot, yv.ptr, yv.ctot, c.N, c.H, c.W, *extra, None, None)
    _close(yv.get(), ref, gate, f"{name} {c.H} x {c.W} {extra}")
    assert xv.untouched() and yv.outside_untouched()


def _run_bwd(c, name, ref_fn, gate, extra):
    g = _g()
    al = R.alignments(c)
    x = _rnd(c.N, c.C, c.H, c.W, seed=1)
    dy = _rnd(*ref_fn(x).shape, seed=2)
    gref = _grad(ref_fn, x, dy)
    prev = _rnd(c.N, c.C, c.H, c.W, seed=3)
    dyv = View(dy, c.off[0], al[0])
    for accumulate in (0, 1):
        dxv = View(prev if accumulate else torch.full(x.shape, float("nan")), c.off[1], al[1])
        g.call(name, dyv.ptr, c.C, dyv.ctot, dxv.ptr, dxv.ctot, c.N, c.H, c.W, *extra, accumulate)
        _close(dxv.get(), gref + prev.double() if accumulate else gref, gate, f"{name} accumulate={accumulate}")
        assert dxv.outside_untouched()
    assert dyv.untouched()


def _run_bwd_relu(c, kind, name, ref_fn, gate, extra):
    """The *_bwd_relu forms against autograd of relu -> op: masked gradient, one partial row per workgroup column and image
    (uz_resample_bwd_relu_rows), their fp64 sums = the bias gradient, and the published bound of |dx|."""
    g = _g()
    al = R.alignments(c)
    dev = g.dev()
    rows = g.L().uz_resample_bwd_relu_rows(kind, c.C, c.N, c.H, c.W)
    assert rows == c.claims["rows"]
    pre = _rnd(c.N, c.C, c.H, c.W, seed=1)
    a = torch.relu(pre)
    dy = _rnd(*ref_fn(a).shape, seed=2)
    prev = _rnd(c.N, c.C, c.H, c.W, seed=3)
    mask = (a > 0).double()
    gref = _grad(ref_fn, a, dy) * mask
    dyv, av = View(dy, c.off[0], al[0]), View(a, c.off[2], al[2])
    for accumulate in (0, 1):
        ref = gref + prev.double() * mask if accumulate else gref
        dxv = View(prev if accumulate else torch.full(pre.shape, float("nan")), c.off[1], al[1])
        part = torch.full(((rows + 2) * c.C,), float("nan"), dtype=torch.float64, device=dev)      # two guard rows
        slot = torch.zeros(256, device=dev)
        g.call(name, dyv.ptr, c.C, dyv.ctot, dxv.ptr, dxv.ctot, c.N, c.H, c.W, *extra, accumulate, av.ptr, av.ctot, part, slot)
        _close(dxv.get(), ref, gate, f"{name} accumulate={accumulate}")
        assert dxv.outside_untouched()
        p, guard = part.cpu()[:rows * c.C], part.cpu()[rows * c.C:]
        assert not bool(torch.isnan(p).any()), "a partial row was left unwritten"
        assert bool(torch.isnan(guard).all()), "a partial row was written past uz_resample_bwd_relu_rows"
        db = p.view(rows, c.C).sum(0)
        assert float((db - ref.sum((0, 2, 3))).abs().max()) <= 1e-5 * float(ref.abs().sum((0, 2, 3)).max())
        amax = float(ref.abs().max())
        assert amax * (1 - 1e-5) <= float(slot.max()) <= amax * 1.001
    assert dyv.untouched() and av.untouched()


def _run_nearest(c):
    g = _g()
    f = c.f

    def ref_fn(t):
        return F.interpolate(t, size=[c.H * f, c.W * f], mode="nearest")
    x = _rnd(c.N, c.C, c.H, c.W, seed=1)
    yr = ref_fn(x)
    xv = View(x, c.off[1])
    yv = View(torch.full(yr.shape, float("nan")), c.off[0])
    g.call("uz_nearest_fwd", xv.ptr, c.C, xv.ctot, yv.ptr, yv.ctot, c.N, c.H, c.W, f)
    assert torch.equal(yv.get(), yr) and yv.outside_untouched() and xv.untouched()
    del yv
    _run_bwd(c, "uz_nearest_bwd", ref_fn, GATE["nearest_bwd"], (f,))


def _run_add_views(c):
    g = _g()
    al = R.alignments(c)
    a, b, prev = (_rnd(c.N, c.C, c.H, c.W, seed=s) for s in (1, 2, 3))
    av = View(a, c.off[0], al[0])
    bv = View(b, c.off[2], al[2]) if c.opt.get("b", 1) else None
    small = c.C * c.H * c.W < 4096
    combos = [(al_, acc) for al_ in (1.0, -0.625) for acc in (0, 1)] if small else [(-0.625, 1)]
    for with_b in ([1, 0] if (bv is not None and small) else [int(bv is not None)]):
        for alpha, accumulate in combos:
            yv = View(prev if accumulate else torch.full(a.shape, float("nan")), c.off[1], al[1])
            use_b = bv if with_b else None
            g.call("uz_add_views", av.ptr, av.ctot, use_b.ptr if use_b else None, use_b.ctot if use_b else 0, yv.ptr, yv.ctot,
                   c.C, c.N, c.H, c.W, alpha, accumulate, None, None, None)
            ref = a.double() + (alpha * b.double() if use_b else 0) + (prev.double() if accumulate else 0)
            _close(yv.get(), ref, GATE["pool"], f"add_views b={with_b} alpha={alpha} accumulate={accumulate}")
            assert yv.outside_untouched()
    assert av.untouched() and (bv is None or bv.untouched())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_against_fp64(case):
    c = case
    if c.op == "avgpool_fwd":
        _run_fwd(c, "uz_avgpool2_fwd", _pool_ref, GATE["pool"], ())
    elif c.op == "avgpool_bwd":
        _run_bwd(c, "uz_avgpool2_bwd", _pool_ref, GATE["pool"], ())
    elif c.op == "avgpool_bwd_relu":
        _run_bwd_relu(c, 0, "uz_avgpool2_bwd_relu", _pool_ref, GATE["pool"], ())
    elif c.op == "nearest":
        _run_nearest(c)
    elif c.op == "add_views":
        _run_add_views(c)
    else:
        for ac in (1, 0):
            if c.op == "bilinear_fwd":
                gate = BILINEAR_FWD_AC_GATE.get((c.H, c.W), GATE["bilinear_fwd"]) if ac else GATE["bilinear_fwd"]
                _run_fwd(c, "uz_bilinear2x_fwd", lambda t: _bil_ref(t, ac), gate, (ac,))
            elif c.op == "bilinear_bwd":
                _run_bwd(c, "uz_bilinear2x_bwd", lambda t: _bil_ref(t, ac), GATE["bilinear_bwd"], (ac,))
            else:
                assert c.op == "bilinear_bwd_relu"
                _run_bwd_relu(c, 1, "uz_bilinear2x_bwd_relu", lambda t: _bil_ref(t, ac), GATE["bilinear_bwd"], (ac,))


@pytest.mark.parametrize("ac", [1, 0])
def test_float4_and_pair_band_kernels_agree_bit_for_bit_in_one_process(ac):
    """The same dy placed 16-byte aligned and 8-byte-only aligned selects the float4 and the pair kernel (tests/_stream_routes.py,
    4 x 32 with dy shifted by 2 floats): the two serve the same call by alignment alone, so their results must be equal bits.
    Several bands and the whole-plane walk included."""
    g = _g()
    for N, C, H, W in [(2, 3, 4, 32), (2, 3, 33, 64), (1, 2048, 20, 32)]:
        dy, prev = _rnd(N, C, 2 * H, 2 * W, seed=5), _rnd(N, C, H, W, seed=6)
        outs = []
        for off in (0, 2):
            dyv = View(dy, off, 16 if off == 0 else 8)
            for accumulate in (0, 1):
                dxv = View(prev if accumulate else torch.full(prev.shape, float("nan")), 0)
                g.call("uz_bilinear2x_bwd", dyv.ptr, C, dyv.ctot, dxv.ptr, dxv.ctot, N, H, W, ac, accumulate)
                outs.append(dxv.get())
        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])


# ------------------------------------------------------------------------------ spatial mean / broadcast
@pytest.mark.parametrize("H,W", R.MEAN_HW)
def test_spatial_mean(H, W):
    g = _g()
    N, C = 2, 3
    x = _rnd(N, C, H, W, seed=1)

    def ref_fn(t):
        return torch.mean(torch.mean(t, dim=2, keepdim=True), dim=3, keepdim=True)
    xv = View(x, 0)
    y = torch.full((N, C), float("nan"), device=g.dev())
    g.call("uz_spatial_mean_fwd", xv.ptr, C, xv.ctot, y, N, H, W)
    _close(y, ref_fn(x.double()).reshape(N, C), GATE["pool"], "spatial_mean_fwd")
    assert xv.untouched()
    dy, prev = _rnd(N, C, 1, 1, seed=2), _rnd(N, C, H, W, seed=3)
    gref = _grad(ref_fn, x, dy)
    dyd = dy.reshape(N, C).to(g.dev())
    for accumulate in (0, 1):
        dxv = View(prev if accumulate else torch.full(x.shape, float("nan")), 0)
        g.call("uz_spatial_mean_bwd", dyd, C, dxv.ptr, dxv.ctot, N, H, W, accumulate)
        _close(dxv.get(), gref + prev.double() if accumulate else gref, GATE["pool"], f"spatial_mean_bwd accumulate={accumulate}")
        assert dxv.outside_untouched()


@pytest.mark.parametrize("L", R.BCAST_L)
@pytest.mark.parametrize("H,W", R.BCAST_HW)
def test_bcast_channels(H, W, L):
    g = _g()
    N = 2
    z = _rnd(N, L, seed=1)
    yv = View(torch.full((N, L, H, W), float("nan")), 0)
    g.call("uz_bcast_channels_fwd", z.to(g.dev()), L, yv.ptr, yv.ctot, N, H, W)
    assert torch.equal(yv.get(), z[:, :, None, None].expand(N, L, H, W)) and yv.outside_untouched()
    dy = _rnd(N, L, H, W, seed=2)
    dyv = View(dy, 0)
    dz = torch.full((N, L), float("nan"), device=g.dev())
    g.call("uz_bcast_channels_bwd", dyv.ptr, dyv.ctot, L, dz, N, H, W)
    _close(dz, dy.double().sum((2, 3)), GATE["pool"], "bcast_channels_bwd")
    assert dyv.untouched()


# ------------------------------------------------------------------------------ KL
def _kl_inputs(N, per):
    """sigma = softplus(normal) + 0.1: every log argument is well away from the 1e-10 guard."""
    mu0, mu1 = _rnd(N, per, seed=1), _rnd(N, per, seed=2)
    s0, s1 = F.softplus(_rnd(N, per, seed=3)) + 0.1, F.softplus(_rnd(N, per, seed=4)) + 0.1
    return mu0, s0, mu1, s1


def _kl_ref(mu0, sigma0, mu1, sigma1):
    """KL_two_gauss_with_diag_cov of the reference model, literally, on whatever dtype it is given."""
    sigma0_fs = torch.mul(torch.flatten(sigma0, start_dim=1), torch.flatten(sigma0, start_dim=1))
    sigma1_fs = torch.mul(torch.flatten(sigma1, start_dim=1), torch.flatten(sigma0, start_dim=1))
    logsigma0_fs = torch.log(sigma0_fs + 1e-10)
    logsigma1_fs = torch.log(sigma1_fs + 1e-10)
    mu0_f = torch.flatten(mu0, start_dim=1)
    mu1_f = torch.flatten(mu1, start_dim=1)
    return torch.mean(0.5 * torch.sum(torch.div(sigma0_fs + torch.mul((mu1_f - mu0_f), (mu1_f - mu0_f)), sigma1_fs + 1e-10)
                                      + logsigma1_fs - logsigma0_fs - 1, dim=1))


@pytest.mark.parametrize("N,per,parts", R.KL_CASES)
def test_kl_fwd_ws(N, per, parts):
    g = _g()
    t = _kl_inputs(N, per)
    ref = 4.0 * float(_kl_ref(*[a.double() for a in t]))
    td = [a.to(g.dev()) for a in t]
    ws = torch.full((72,), float("nan"), dtype=torch.float64, device=g.dev())          # the 512 bytes the header asks for, and a guard
    for workspace in (ws, None):                                                          # no workspace: the single-workgroup kernel, same sum
        out = torch.full((1,), float("nan"), device=g.dev())
        g.call("uz_kl_fwd_ws", *td, N, per, 4.0, out, workspace)
        assert abs(float(out) - ref) <= GATE["kl"] * max(1.0, abs(ref)), (float(out), ref)
    assert int((~torch.isnan(ws[:64])).sum()) == (parts if parts > 1 else 0)             # exactly `parts` partials were written
    assert bool(torch.isnan(ws[64:]).all())


@pytest.mark.parametrize("N,per", R.KL_BWD_CASES)
def test_kl_bwd(N, per):
    g = _g()
    t = _kl_inputs(N, per)
    leaves = [a.double().requires_grad_(True) for a in t]
    (0.37 * 4.0 * _kl_ref(*leaves)).backward()
    refs = [x.grad for x in leaves]
    td = [a.to(g.dev()) for a in t]
    scale = torch.tensor([0.37], device=g.dev())
    for missing in (None, 0, 1, 2, 3):                                                     # each output pointer null in turn
        outs = [None if i == missing else torch.full((N, per), float("nan"), device=g.dev()) for i in range(4)]
        g.call("uz_kl_bwd", *td, N, per, 4.0, scale, *outs)
        for i, (o, r) in enumerate(zip(outs, refs)):
            if o is not None:
                _close(o, r, GATE["kl_grad"], f"kl_bwd output {i} (null: {missing})")
    outs = [torch.full((N, per), float("nan"), device=g.dev()) for _ in range(4)]
    g.call("uz_kl_bwd", *td, N, per, 4.0, None, *outs)                                     # no loss_scale: scale 1
    for i, (o, r) in enumerate(zip(outs, refs)):
        _close(o, r / 0.37, GATE["kl_grad"], f"kl_bwd output {i} unscaled")


# ------------------------------------------------------------------------------ residual CE / accumulate + softmax + argmax
def _ce_setup(K, L, H, W, N=3):
    s = [_rnd(N, K, H, W, seed=10 + l) for l in range(L)]
    tgt = torch.randint(0, K, (N, 1, H, W), generator=torch.Generator().manual_seed(3))
    if N * H * W >= K:
        tgt.view(-1)[:K] = torch.arange(K)                                                  # every class is used
    return s, tgt


def _ce_levels(s, tgt):
    """Per-level cross entropy of the residual sums taken from the last level down (residual_multinoulli_loss), mean over the
    batch of the per-image sums."""
    N, K = s[0].shape[:2]
    out, acc = [None] * len(s), None
    for l in reversed(range(len(s))):
        acc = s[l] if acc is None else acc + s[l]
        ce = F.cross_entropy(acc.reshape(N, K, -1), tgt.reshape(N, -1).long(), reduction="none")
        out[l] = torch.mean(torch.sum(ce, dim=1))
    return out


@pytest.mark.parametrize("H,W", R.CE_HW)
@pytest.mark.parametrize("K,L", R.CE_KL)
def test_residual_ce(K, L, H, W):
    g = _g()
    N = 3
    s, tgt = _ce_setup(K, L, H, W)
    leaves = [t.double().requires_grad_(True) for t in s]
    lv = _ce_levels(leaves, tgt)
    (0.37 * sum(lv)).backward()
    lv = [v.detach() for v in lv]
    sd = [t.to(g.dev()) for t in s]
    tab = torch.tensor([t.data_ptr() for t in sd], dtype=torch.int64, device=g.dev())
    ws = torch.empty(g.L().uz_ce_workspace(N, H, W, L) // 8, dtype=torch.float64, device=g.dev())
    out = torch.full((8,), float("nan"), device=g.dev())
    td = tgt.float().to(g.dev())
    g.call("uz_residual_ce_fwd", tab, L, K, td, N, H, W, out, ws)
    for l in range(L):
        assert abs(float(out[l]) - float(lv[l])) <= GATE["ce"] * max(1.0, abs(float(lv[l]))), (l, float(out[l]), float(lv[l]))
    assert bool(torch.isnan(out[L:]).all())
    ds = [torch.full_like(t, float("nan")) for t in sd]
    gtab = torch.tensor([t.data_ptr() for t in ds], dtype=torch.int64, device=g.dev())
    scale = torch.tensor([0.37], device=g.dev())
    g.call("uz_residual_ce_bwd", tab, gtab, L, K, td, N, H, W, scale)
    for l in range(L):
        _close(ds[l], leaves[l].grad, GATE["ce_grad"], f"residual_ce_bwd level {l}")


@pytest.mark.parametrize("H,W", R.CE_HW)
@pytest.mark.parametrize("K,L", R.CE_KL)
def test_accumulate_softmax_argmax(K, L, H, W):
    g = _g()
    N = 3
    s, _ = _ce_setup(K, L, H, W)
    acc32 = s[-1].clone()
    for i in range(L - 1):
        acc32 += s[i]                                                                       # accumulate_output's order, fp32
    acc = s[-1].double()
    for i in range(L - 1):
        acc = acc + s[i].double()
    sd = [t.to(g.dev()) for t in s]
    tab = torch.tensor([t.data_ptr() for t in sd], dtype=torch.int64, device=g.dev())
    a, so = (torch.full((N, K, H, W), float("nan"), device=g.dev()) for _ in range(2))
    lab = torch.full((N, H, W), 255, dtype=torch.uint8, device=g.dev())
    g.call("uz_accumulate_softmax_argmax", tab, L, K, N, H, W, a, so, lab)
    assert torch.equal(a.cpu(), acc32)
    _close(so, F.softmax(acc, dim=1), GATE["softmax"], "softmax")
    # exact: the label is the first strict maximum of the very probabilities the call stores, as torch.argmax takes it
    assert torch.equal(lab.cpu().long(), torch.argmax(so.cpu(), dim=1))
    # and those are gated at 1e-6: the label is torch.argmax of the fp64 softmax wherever the two largest probabilities are
    # further apart than twice that gate (exact ties: the test below)
    p = F.softmax(acc, dim=1)
    chosen = p.gather(1, lab.cpu().long().unsqueeze(1)).squeeze(1)
    assert int(lab.max()) < K and bool((p.max(dim=1).values - chosen <= 2 * GATE["softmax"]).all())


def test_argmax_ties_take_the_first_maximal_class():
    """Small integers: the level sums are exact and many pixels hold exact ties between two, three or all classes."""
    g = _g()
    N, K, L, H, W = 3, 4, 3, 9, 29
    gen = torch.Generator().manual_seed(7)
    s = [torch.randint(-1, 2, (N, K, H, W), generator=gen).float() for _ in range(L)]
    acc = s[0] + s[1] + s[2]
    ties = (acc == acc.max(dim=1, keepdim=True).values).sum(1)
    assert int((ties == 2).sum()) > 0 and int((ties == 3).sum()) > 0 and int((ties == 4).sum()) > 0
    sd = [t.to(g.dev()) for t in s]
    tab = torch.tensor([t.data_ptr() for t in sd], dtype=torch.int64, device=g.dev())
    lab = torch.full((N, H, W), 255, dtype=torch.uint8, device=g.dev())
    so = torch.empty(N, K, H, W, device=g.dev())
    g.call("uz_accumulate_softmax_argmax", tab, L, K, N, H, W, None, so, lab)
    assert torch.equal(lab.cpu().long(), torch.argmax(acc.double(), dim=1))
    _close(so, F.softmax(acc.double(), dim=1), GATE["softmax"], "softmax")


# ------------------------------------------------------------------------------ Adam, latent sample, axpy, scale
@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("n", R.VEC_N)
def test_adam(n, wd):
    """A double restatement of torch.optim.Adam's update (L2 weight decay, lerp of the first moment, sqrt(v) / sqrt(bc2) + eps),
    with the gradient scaled by grad_scale first; three steps from zero moments at step 1 and from given moments at step 1000."""
    g = _g()
    lr, b1, b2, eps, gs = 1e-3, 0.9, 0.999, 1e-8, 0.5
    for start in (1, 1000):
        p0 = _rnd(n, seed=1)
        m0 = torch.zeros(n) if start == 1 else 0.1 * _rnd(n, seed=2)
        v0 = torch.zeros(n) if start == 1 else 0.01 * _rnd(n, seed=3) ** 2
        grads = [_rnd(n, seed=10 + i) for i in range(3)]
        p, m, v = p0.double(), m0.double(), v0.double()
        pd, md, vd = p0.to(g.dev()), m0.to(g.dev()), v0.to(g.dev())
        for i, gr in enumerate(grads):
            step = start + i
            gi = gr.double() * gs + wd * p
            m = m + (gi - m) * (1 - b1)
            v = v * b2 + (1 - b2) * gi * gi
            bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
            p = p - (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))
            g.call("uz_adam_step", pd, gr.to(g.dev()), md, vd, n, step, lr, b1, b2, eps, wd, gs)
        _close(pd, p, GATE["adam"], f"adam params from step {start}")
        _close(md, m, GATE["adam"], "adam exp_avg")
        _close(vd, v, GATE["adam"], "adam exp_avg_sq")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("n", R.VEC_N)
def test_latent_sample(n, act):
    """pre_sigma on both sides of softplus' threshold of 20 (19.9, 20.0, 20.1, 25).  The gates of tests/test_ops_gpu.py (1e-6; 2e-5
    for dpre_sigma), here per element: relative to max(1, |ref|), or for a sum of two terms to max(1, the magnitude its fp32
    addition rounds at)."""
    g = _g()
    mu, pre, eps = _rnd(n, seed=1), _rnd(n, seed=2) * 3, _rnd(n, seed=3)
    special = torch.tensor([20.0, 19.9, 20.1, 25.0])
    pre[:min(n, 4)] = special[:min(n, 4)]
    dmu, dsig, dz = _rnd(n, seed=4), _rnd(n, seed=5), _rnd(n, seed=6)
    mr, pr = mu.double().requires_grad_(True), pre.double().requires_grad_(True)
    sr = torch.exp(pr) if act else F.softplus(pr)
    zr = mr + sr * eps.double()
    (zr * dz.double() + mr * dmu.double() + sr * dsig.double()).sum().backward()
    dev = g.dev()
    sig, z = torch.full((n,), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev)
    g.call("uz_latent_sample_fwd", mu.to(dev), pre.to(dev), eps.to(dev), sig, z, n, act)
    sr, zr = sr.detach(), zr.detach()
    assert bool(((sig.cpu().double() - sr).abs() <= 1e-6 * sr.clamp(min=1.0)).all())
    zmag = mu.double().abs() + (sr * eps.double()).abs()                                        # the magnitude the fp32 sum rounds at
    assert bool(((z.cpu().double() - zr).abs() <= 1e-6 * zmag.clamp(min=1.0)).all())
    a, b = torch.full((n,), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev)
    g.call("uz_latent_sample_bwd", dmu.to(dev), dsig.to(dev), dz.to(dev), eps.to(dev), sig, a, b, n, act)
    assert bool(((a.cpu().double() - mr.grad).abs() <= 1e-6 * mr.grad.abs().clamp(min=1.0)).all())
    dsdp = sr if act else torch.sigmoid(pre.double())
    mag = dsdp * (dsig.double().abs() + (dz.double() * eps.double()).abs())
    assert bool(((b.cpu().double() - pr.grad).abs() <= 2e-5 * mag.clamp(min=1.0)).all())
    sig2 = torch.full((n,), float("nan"), device=dev)
    g.call("uz_latent_sample_fwd", None, pre.to(dev), None, sig2, None, n, act)                 # the prior's draw is discarded: z null
    assert torch.equal(sig2, sig)


@pytest.mark.parametrize("n", R.VEC_N)
def test_axpy_and_scale(n):
    g = _g()
    x, y = _rnd(n, seed=1), _rnd(n, seed=2)
    buf = torch.full((n + 2,), float("nan"), device=g.dev())
    buf[1:1 + n] = y.to(g.dev())
    g.call("uz_axpy", buf[1:], x.to(g.dev()), -0.625, n)
    _close(buf[1:1 + n], y.double() - 0.625 * x.double(), GATE["adam"], "axpy")
    g.call("uz_scale", buf[1:], 1.7, n)
    _close(buf[1:1 + n], (y.double() - 0.625 * x.double()) * float(torch.tensor(1.7)), GATE["adam"], "scale")
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1]))                              # nothing written past either end


# ------------------------------------------------------------------------------ l2 norms
def _norm_layout():
    """(offset, count) pairs: every count of the table at every residue of the offset mod 4, one float of gap between tensors."""
    oc, pos = [], 0
    for r in range(4):
        for cnt in R.NORM_COUNTS:
            pos += 1
            while pos % 4 != r:
                pos += 1
            oc.append((pos, cnt))
            pos += cnt
    return oc, pos + 4


@pytest.mark.parametrize("gshift", [0, 1])
def test_l2_norms_and_backward(gshift):
    """The head / float4 body / tail split for the four alignment classes of a tensor's offset, counts shorter than the head, and
    the backward into a gradient buffer of the same alignment class (float4 body) and one shifted by a float (scalar)."""
    g = _g()
    oc, total = _norm_layout()
    flat = _rnd(total, seed=1)
    ref = torch.stack([flat[o:o + c].double().square().sum().sqrt() for o, c in oc])
    fd = flat.to(g.dev())
    assert fd.data_ptr() % 16 == 0
    ocd = torch.tensor([v for p in oc for v in p], dtype=torch.int64, device=g.dev())
    out = torch.full((len(oc),), float("nan"), device=g.dev())
    g.call("uz_l2_norms", fd, ocd, len(oc), out)
    assert bool(((out.cpu().double() - ref).abs() <= GATE["norms"] * ref.clamp(min=1.0)).all()), (out.cpu().double() - ref).abs().max()
    g0 = _rnd(total, seed=2)
    gbuf = torch.full((total + 8,), float("nan"), device=g.dev())
    gbuf[gshift:gshift + total] = g0.to(g.dev())
    gview = gbuf[gshift:]
    assert gview.data_ptr() % 16 == 4 * gshift
    scale = torch.tensor([0.37], device=g.dev())
    g.call("uz_l2_norms_bwd", fd, ocd, len(oc), out, scale, gview)
    gref = g0.double().clone()
    for (o, c), nr in zip(oc, ref):
        if c and float(nr) > 0:
            gref[o:o + c] += 0.37 * flat[o:o + c].double() / nr
    _close(gbuf[gshift:gshift + total], gref, GATE["norms_bwd"], "l2_norms_bwd")
    touched = torch.zeros(total, dtype=torch.bool)
    for o, c in oc:
        touched[o:o + c] = True
    assert torch.equal(gbuf[gshift:gshift + total].cpu()[~touched], g0[~touched])                # the gaps between tensors keep their bits
    assert bool(torch.isnan(gbuf[:gshift]).all()) and bool(torch.isnan(gbuf[gshift + total:]).all())
