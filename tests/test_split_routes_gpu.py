"""fp64 parity of every case of the split-storage dispatch table (tests/_split_routes.py): the operand and epilogue forms a training
step hands the split-fp16 kernels - input in split storage, a concat buffer with two scale segments, the producer's BatchNorm
applied while staging, the BatchNorm-backward reduction folded into the data gradient's epilogue - each run through the C ABI in
its own math mode on the kernel instance tests/test_split_routes_cpu.py proves it takes, at K tails, channel overhangs, ragged
tiles, H < 16, W % 4 != 0, misaligned views and chunk loops in 1, 2 and 4 parts.  (These are the two-piece fp16 forms; the storage
forms of the single-piece bf16 mode are tested in tests/test_b16_storage_gpu.py.)

Every packed input is packed ON THE HOST by the numpy twin of split_f16.h; the twin is tied to the device once per case
(uz_pack_split of the case's fp32 operand equals the twin's words bit for bit, uz_unpack_split of the twin's words equals the twin's
decode bit for bit).  Inputs and outputs are channel-slice views of NaN-filled wider buffers.

Gates (imported from tests/test_conv_routes_gpu.py, same elementwise ratio |got - ref64| / (den + floor) and the same floor):
  * packed forms: GATE[(mode, direction, 1)].  The fp64 reference is taken over the DECODED operand, which the packed words represent
    exactly, so the kernel's error is the plain route's minus one operand's residual and the existing gate bounds it.
  * uz_conv_fwd_bn_ex: GATE + 2^-24.  The kernel forms the operand a = max(fmaf(y, alpha, beta'), 0) in fp32, the reference in fp64
    from the same fp32 table: fmaf rounds the exact alpha y + beta' once, |a32 - a64| <= 2^-24 |a64|, so every product and with it the
    sum moves by at most 2^-24 of den: 6e-8 in the ratio, added to the key's gate.
  * the fold: the stored dz by the key's gate (exactly 0 where the fp64 mask is 0: the inputs keep every element 2^-20 away from the
    threshold, where the fp32 fmaf has the fp64 sign); the partial rows summed in fp64 against sums of the STORED dz within BN_SUM of
    sum |dz| and sum |dz x_hat|; max |dz| bit-equal to the stored tensor's; max |x_hat| bit-equal to the fp32 restatement
    (y - mean) * rstd (two fp32 operations: nothing to contract).
  * weight-gradient cases keep N H W at or above the smallest case of their key in tests/_conv_routes.py, so the imported gate applies.
In modes 1 and 2 the tensor-max relative error must also stay <= TENSOR_MAX.  No gate is set from what these tests observe."""
import pytest
import torch

from tests import _conv_routes as R
from tests import _split_routes as S
from tests.test_conv_routes_gpu import BN_SUM, GATE, TENSOR_MAX

pytestmark = pytest.mark.gpu

AFF_EXTRA = 2.0 ** -24
WORST = {}


def _g():
    from tests import _gpu
    return _gpu


def _slot(v):
    t = torch.zeros(256, device=_g().dev())
    t[0] = float(v)
    return t


def _nan(*shape):
    return torch.full(shape, float("nan"), device=_g().dev())


def _view(t, lead, misaligned=False):
    """t (CPU, NCHW) as channels [lead, lead + C) of a NaN-filled buffer with S.TAIL channels behind -> (flat raw buffer, buffer as
    NCHW, view from channel lead on).  misaligned: the buffer starts 4 bytes behind a 16-byte boundary."""
    n, c, h, w = t.shape
    ctot = lead + c + S.TAIL
    numel = n * ctot * h * w
    raw = _nan(numel + 8)
    assert raw.data_ptr() % 16 == 0
    off = 1 if misaligned else 4
    buf = raw[off:off + numel].view(n, ctot, h, w)
    buf[:, lead:lead + c] = t.to(raw.device)
    return raw, buf, buf[:, lead:]


def _intact(raw, buf, lead, c):
    """NaN canaries on both sides of the view's channels and around the buffer"""
    off = (buf.data_ptr() - raw.data_ptr()) // 4
    return (bool(torch.isnan(buf[:, :lead]).all()) and bool(torch.isnan(buf[:, lead + c:]).all())
            and bool(torch.isnan(raw[:off]).all()) and bool(torch.isnan(raw[off + buf.numel():]).all()))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check(case, what, got, q, extra=0.0):
    got = got.detach().cpu().double()
    ratio = float(((got - q.ref).abs() / (q.den + q.floor)).max())
    gate = GATE[S.key_of(case)] + extra
    key = (case.form, case.mode, case.direction, S.geometry(case))
    WORST[key] = max(WORST.get(key, (0.0, gate))[0], ratio), gate
    print(f"  {S.case_id(case)} {what}: ratio {ratio:.3e} (gate {gate:.2e})")
    assert ratio <= gate, f"{S.case_id(case)} {what}: worst elementwise ratio {ratio:.3e} > {gate:.2e}"
    rel = float((got - q.ref).abs().max() / q.ref.abs().max().clamp_min(1e-300))
    assert rel <= TENSOR_MAX, f"{S.case_id(case)} {what}: tensor-max relative error {rel:.3e}"


def _twin(case, ops):
    """the host twin against the device, on the case's fp32 operand with the bounds the case packs it with"""
    g = _g()
    pk = ops.apk if ops.apk is not None else S.Packed(ops.a, float(ops.a.abs().max()))
    spans = [(0, pk.seg, pk.amax), (pk.seg, ops.a.shape[1], pk.amax2)] if pk.seg else [(0, ops.a.shape[1], pk.amax)]
    for lo, hi, amax in spans:
        x = ops.a[:, lo:hi].contiguous().to(g.dev())
        words = pk.words[:, lo:hi].contiguous().to(g.dev())
        out, back = torch.empty_like(x), torch.empty_like(x)
        g.call("uz_pack_split", x, out, x.numel(), _slot(amax))
        g.call("uz_unpack_split", words, back, x.numel(), _slot(amax))
        assert torch.equal(_bits(out), _bits(words)), f"{S.case_id(case)}: uz_pack_split differs from the host twin"
        assert torch.equal(_bits(back), _bits(pk.dec32[:, lo:hi])), f"{S.case_id(case)}: uz_unpack_split differs from the host twin"


def _fwd_partials(case, part, npart, y):
    """tests/test_conv_routes_gpu.py _fwd: the fused statistics are those of the stored y"""
    Cout = case.Cout
    assert not bool(torch.isnan(part[:npart * Cout * 4]).any()) and bool(torch.isnan(part[npart * Cout * 4:]).all())
    y64 = y.cpu().double()
    p = part[:npart * Cout * 4].view(npart, Cout, 4).cpu().double()
    s1, s2 = y64.sum((0, 2, 3)), (y64 * y64).sum((0, 2, 3))
    assert float(((p[:, :, 0].sum(0) - s1).abs() / y64.abs().sum((0, 2, 3))).max()) <= BN_SUM
    assert float(((p[:, :, 1].sum(0) - s2).abs() / s2).max()) <= BN_SUM
    assert torch.equal(p[:, :, 2].max(0).values, y64.amax((0, 2, 3))) and torch.equal(p[:, :, 3].max(0).values, (-y64).amax((0, 2, 3)))


def _fwd(case, idx, ops, L, dev):
    g = _g()
    c = case
    N, Cin, Cout, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    exp = S.evaluate(c, ops)
    aff = c.form == "aff"
    xraw, xbuf, xv = _view(ops.a if aff else ops.apk.words, c.xoff)
    CinTot, CoutTot = xbuf.shape[1], c.yoff + Cout + S.TAIL
    yraw, ybuf, yv = _view(torch.full((N, Cout, H, W), float("nan")), c.yoff)
    wd, bd = ops.w.to(dev), ops.bias.to(dev)
    wsb = L.uz_conv_workspace(Cin, Cout, N, H, W, 3)
    ws = torch.empty(wsb // 4 + 16, device=dev)
    npart = c.claims["bn"] if "bnpart" in c.opt else 0
    part = _nan(npart * Cout * 4 + 64) if npart else None
    y = ybuf[:, c.yoff:c.yoff + Cout]
    if aff:
        save, slot = ops.extra["save"].to(dev), _slot(ops.extra["a_amax"])

        def run(bias, bnp):
            g.call("uz_conv_fwd_bn_ex", xv, Cin, CinTot, save, c.bn_relu, wd, bias, yv, Cout, CoutTot, N, H, W, 3, slot, None, None, ws, wsb, None, bnp)
    else:
        s1, s2 = _slot(ops.apk.amax), (_slot(ops.apk.amax2) if c.seg else None)

        def run(bias, bnp, relu=0):
            g.call("uz_conv_fwd_ex", xv, Cin, CinTot, wd, bias, yv, Cout, CoutTot, N, H, W, 3, relu, s1, None, None, ws, wsb, None, bnp, 1, s2, c.seg)
    run(bd, part)
    assert _intact(yraw, ybuf, c.yoff, Cout), "the forward wrote outside its output view"
    assert _intact(xraw, xbuf, c.xoff, Cin)
    _check(c, "bias", y, exp["y"], AFF_EXTRA if aff else 0.0)
    if npart:
        _fwd_partials(c, part, npart, y)
    # second launch: no bias (packed forms: with the ReLU epilogue)
    if aff:
        run(None, None)
        _check(c, "no bias", y, exp["conv"], AFF_EXTRA)
    else:
        run(None, None, relu=1)
        q = exp["conv"]
        _check(c, "relu, no bias", y, S.Q(torch.relu(q.ref), q.den, q.floor, "gate"))
    assert _intact(yraw, ybuf, c.yoff, Cout)


def _dgrad(case, idx, ops, L, dev):
    g = _g()
    c = case
    N, Cin, Cout, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    exp = S.evaluate(c, ops)
    packed = ops.apk is not None
    dyraw, dybuf, dyv = _view(ops.apk.words if packed else ops.a, c.xoff)
    CoutTot, CinTot = dybuf.shape[1], c.yoff + Cin + S.TAIL
    dxraw, dxbuf, dxv = _view(torch.full((N, Cin, H, W), float("nan")), c.yoff, "mis-dx" in c.opt)
    wd = ops.w.to(dev)
    wsb = L.uz_conv_workspace(Cin, Cout, N, H, W, 3)
    ws = torch.empty(wsb // 4 + 16, device=dev)
    slot = _slot(ops.apk.amax if packed else ops.a.abs().max())
    dx = dxbuf[:, c.yoff:c.yoff + Cin]
    if c.form != "fold":
        g.call("uz_conv_bwd_data_ex", dyv, Cout, CoutTot, wd, dxv, Cin, CinTot, N, H, W, 3, 0, slot, None, ws, wsb, None, 1, None, 0, None, 0, None)
        assert _intact(dxraw, dxbuf, c.yoff, Cin), "the data gradient wrote outside its output view"
        _check(c, "overwrite", dx, exp["dx"])
        dx.copy_(ops.extra["prev"].to(dev))
        g.call("uz_conv_bwd_data_ex", dyv, Cout, CoutTot, wd, dxv, Cin, CinTot, N, H, W, 3, 1, slot, None, ws, wsb, None, 1, None, 0, None, 0, None)
        assert _intact(dxraw, dxbuf, c.yoff, Cin)
        _check(c, "accumulate", dx, exp["dx_acc"])
        return
    rows = c.claims["relu"]
    yraw, ybuf, yv = _view(ops.extra["y"], c.yoff + 2, "mis-y" in c.opt)
    yCtot = ybuf.shape[1]
    assert yCtot > Cin
    save = ops.extra["save"].to(dev)
    part = _nan(rows * Cin * 4 + 64)
    g.call("uz_conv_bwd_data_ex", dyv, Cout, CoutTot, wd, dxv, Cin, CinTot, N, H, W, 3, 0, slot, None, ws, wsb, None, int(packed), yv, yCtot, save, c.bn_relu, part)
    assert _intact(dxraw, dxbuf, c.yoff, Cin), "the folded data gradient wrote outside its output view"
    assert _intact(yraw, ybuf, c.yoff + 2, Cin) and _intact(dyraw, dybuf, c.xoff, Cout)
    _check(c, "dz", dx, exp["dz"])
    dz = dx.cpu()
    assert bool((dz[exp["mask"].ref == 0] == 0).all()), "dz is not exactly 0 behind the ReLU mask"
    assert not bool(torch.isnan(part[:rows * Cin * 4]).any()), "a partial row was not written"
    assert bool(torch.isnan(part[rows * Cin * 4:]).all()), "the fold wrote behind its partial rows"
    p = part[:rows * Cin * 4].view(rows, Cin, 4).cpu()
    dz64, y64 = dz.double(), ops.extra["y"].double()
    mean, rstd = (ops.extra["save"][i * Cin:(i + 1) * Cin].double()[None, :, None, None] for i in (0, 1))
    dzx = dz64 * ((y64 - mean) * rstd)
    e1 = float(((p[:, :, 0].double().sum(0) - dz64.sum((0, 2, 3))).abs() / dz64.abs().sum((0, 2, 3)).clamp_min(1e-300)).max())
    e2 = float(((p[:, :, 1].double().sum(0) - dzx.sum((0, 2, 3))).abs() / dzx.abs().sum((0, 2, 3)).clamp_min(1e-300)).max())
    print(f"  {S.case_id(c)} partial sums: sum dz {e1:.3e}, sum dz x_hat {e2:.3e} (gate {BN_SUM:.1e})")
    assert e1 <= BN_SUM and e2 <= BN_SUM
    assert torch.equal(p[:, :, 2].max(0).values, dz.abs().amax((0, 2, 3))), "max |dz| is not that of the stored dz"
    assert torch.equal(p[:, :, 3].max(0).values.double(), exp["max_xhat"].ref), "max |x_hat| is not the fp32 (y - mean) * rstd"


def _wgrad(case, idx, ops, L, dev):
    g = _g()
    c = case
    N, Cin, Cout, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    exp = S.evaluate(c, ops)
    xpk, dpk = ops.apk, ops.extra["bpk"]
    xraw, xbuf, xv = _view(xpk.words if xpk is not None else ops.a, c.xoff)
    dyraw, dybuf, dyv = _view(dpk.words if dpk is not None else ops.b, c.yoff)
    CinTot, CoutTot = xbuf.shape[1], dybuf.shape[1]
    assert CinTot > Cin and CoutTot > Cout
    xs = _slot(xpk.amax if xpk is not None else ops.a.abs().max())
    xs2 = _slot(xpk.amax2) if c.seg else None
    ds = _slot(dpk.amax if dpk is not None else ops.b.abs().max())
    wsb = L.uz_conv_bwd_weight_workspace(Cin, Cout, N, H, W, 3)
    ws = torch.empty(wsb // 4 + 16, device=dev)
    n = Cout * Cin * 9
    args = (xv, Cin, CinTot, dyv, Cout, CoutTot)
    tail = (N, H, W, 3, xs, ds, ws, wsb, int(xpk is not None), xs2, c.seg, int(dpk is not None))
    raw, dw = g.guarded(n, torch.float32, fill=float("nan"))
    g.call("uz_conv_bwd_weight_ex", *args, dw, None, *tail, None)
    assert bool(torch.isnan(raw[:64]).all()) and bool(torch.isnan(raw[64 + n:]).all()), "the weight gradient wrote outside dw"
    _check(c, "weight gradient", dw.view(Cout, Cin, 3, 3), exp["dw"])
    dw2 = _nan(n)
    g.call("uz_conv_bwd_weight_ex", *args, dw2, None, *tail, None)
    assert torch.equal(dw, dw2), "the weight gradient is not deterministic"
    if "slabs" in c.opt:
        Sn = c.claims["slabs"]
        slabs, dw3 = _nan(Sn * n + 64), _nan(n)
        g.call("uz_conv_bwd_weight_ex", *args, dw3, None, *tail, slabs)
        assert bool(torch.isnan(dw3).all()) and bool(torch.isnan(slabs[Sn * n:]).all())
        table = torch.tensor([slabs.data_ptr(), dw3.data_ptr(), Sn, Cout, Cin, 9, 0, 0], dtype=torch.int64, device=dev)
        g.call("uz_wgrad_reduce_table", table, 1, L.uz_wgrad_reduce_blocks(Cin, Cout, 3))
        assert torch.equal(dw, dw3), "slabs_out + uz_wgrad_reduce_table differs from the in-call reduction"


GPU_CASES = list(enumerate(S.CASES))


@pytest.mark.parametrize("idx,case", GPU_CASES, ids=[S.case_id(c) for c in S.CASES])
def test_split_case_against_fp64(idx, case):
    from unet_zoo_amd import _ffi
    L = _ffi.lib()
    dev = _g().dev()
    process_mode = L.uz_get_conv_math()
    installed = True
    if process_mode in (0, 3):                           # forced for the process: can the case's mode be installed at all?
        installed = L.uz_set_conv_math(case.mode) == 0
        L.uz_set_conv_math(process_mode)
    if not installed:
        pytest.skip(f"UZ_CONV_MATH forces math mode {process_mode} and mode {case.mode} cannot be installed: split storage is the two-piece fp16 format")
    with R.dispatch_state(L, case.mode):
        assert S.queries(L, case) == case.claims, "the case left its route (tests/test_split_routes_cpu.py)"
        ops = S.operands(case, idx)
        _twin(case, ops)
        {"fwd": _fwd, "dgrad": _dgrad, "wgrad": _wgrad}[case.direction](case, idx, ops, L, dev)


def test_zz_report_worst_ratios(capsys):
    """Lists the worst elementwise ratio per (form, math mode, direction, geometry) seen by the cases above (run with them)."""
    with capsys.disabled():
        print("\nworst elementwise |got - ref64| / (den + floor) per (form, mode, direction, geometry):")
        for k in sorted(WORST):
            print(f"  {k}: {WORST[k][0]:.3e}  (gate {WORST[k][1]:.2e})")
