"""Every case of the BatchNorm dispatch table (tests/_bn_routes.py) through the C ABI against fp64 tensor arithmetic on the same fp32
operands (_bn_routes.reference): training forward (a, save_mean_rstd, running statistics, the bound slot), backward (dy, dgamma,
dbeta, dbias) from the save the forward wrote, eval forward, a second run that must repeat the first bit for bit, and the folded
inputs synthesised on the host - convolution partials forward (_pre, _ex with the 4 C table, _phase 1 + 2) and backward (with
dbias_partials), split-K slabs on the small path, split storage - so that no convolution's tiling decides what is tested.  Every
tensor operand is a channel-slice view in a NaN-filled allocation; everything outside a view must keep its bits.

Gates are those of tests/test_ops_gpu.py::test_bn_relu_fwd_bwd (a 2e-5, 3e-5 with statistics from partials; running mean 1e-6,
variance 1e-5; dy 3e-5 max(1, max |dy|); dgamma, dbeta 1e-4 relative; dbias, analytically zero, 1e-3 max(1, sqrt(sum |dA|))) and
relerr(save) <= 2e-6 of ::test_conv_with_fused_bn_statistics; bf16 storage: tests/test_b16_storage_gpu.py (see _b16_close).  The
ReLU knife edge is handled by the reference (dA zeroed within 1e-4 of the edge; _bn_routes docstring), never by leaving elements out."""
import ctypes

import pytest
import torch

from tests import _bn_routes as R

pytestmark = pytest.mark.gpu

FP32 = [c for c in R.CASES if not c.b16 and not c.o("refused")]
TRAIN = [(c, relu) for c in FP32 if c.training for relu in ((1,) if c.o("big") else (1, 0))]
EVAL = [(c, relu) for c in FP32 if not c.training for relu in (1, 0)]
B16 = [c for c in R.CASES if c.b16]
NAN = float("nan")


def _g():
    from tests import _gpu
    return _gpu


def _id(p):
    return R.case_id(p[0]) + f"-relu{p[1]}"


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class View:
    """An NCHW tensor (a CPU tensor, or a shape: then the view itself is NaN too) as channels [c0, c0 + C) of a wider buffer that
    starts `off` elements into a NaN-filled allocation.  fp32: c0 = 1 of C + 2 channels; bf16: c0 = 2 of C + 3 (16-byte alignment
    of a 2-byte view needs an even number of H W % 4 == 0 planes in front of it)."""

    def __init__(self, t, off=0, dtype=torch.float32):
        self.shape = tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(t)
        n, c, h, w = self.shape
        self.c0 = R.C0 if dtype == torch.float32 else 2
        self.ctot, self.off = c + self.c0 + 1, off
        self.flat = torch.full((off + n * self.ctot * h * w + 4,), NAN, device=_g().dev(), dtype=dtype)
        if isinstance(t, torch.Tensor):
            self.inner().copy_(t.to(_g().dev()))
        self.ptr = self._body(self.flat)[:, self.c0:]
        self.before = self.flat.clone()

    def _body(self, flat):
        n, c, h, w = self.shape
        return flat[self.off:self.off + n * self.ctot * h * w].view(n, self.ctot, h, w)

    def inner(self, flat=None):
        return self._body(self.flat if flat is None else flat)[:, self.c0:self.c0 + self.shape[1]]

    def get(self):
        return self.inner().float().cpu()

    def aligned(self):
        return self.ptr.data_ptr() % 16 == 0

    def outside_kept(self):
        """Every element of the allocation outside the view has the bits it had when the view was made."""
        now, was = self.flat.clone(), self.before.clone()
        self.inner(now).zero_()
        self.inner(was).zero_()
        return bool(torch.equal(_bits(now), _bits(was)))

    def untouched(self):
        return bool(torch.equal(_bits(self.flat), _bits(self.before)))


def _dev(t):
    return None if t is None else t.to(_g().dev())


def _ws(c, extra=16):
    g = _g()
    return torch.empty(g.L().uz_bn_workspace(c.C, c.N, c.H, c.W) // 4 + extra, device=g.dev())


def _slot():
    return torch.zeros(256, device=_g().dev())


def _err(got, ref):
    return float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max())


def _rel(got, ref):
    return _err(got, ref) / (float(ref.abs().max()) + 1e-12)


def _gate(what, err, gate):
    print(f"{what}: {err:.3e} (gate {gate:.3g})")
    assert err <= gate, f"{what}: {err:.3e} exceeds {gate:.3g}"        # (NaN fails too)


def _check_forward(tag, ref, a, save, rm, rv, slot, gate_a=2e-5):
    C = ref["mean"].numel()
    _gate(f"{tag} a", _err(a, ref["a"]), gate_a)
    _gate(f"{tag} save", _rel(save[:2 * C], torch.cat([ref["mean"], ref["rstd"]])), 2e-6)
    if rm is not None:
        _gate(f"{tag} running mean", _err(rm, ref["rm"]), 1e-6)
        _gate(f"{tag} running var", _err(rv, ref["rv"]), 1e-5)
    if slot is not None:
        top, amax = float(ref["a"].abs().max()), float(slot.max())
        print(f"{tag} bound slot {amax:.6g}, max |a| {top:.6g}")
        assert top * (1 - 1e-5) <= amax <= top * 1.001


def _check_backward(tag, ref, dy, dgm, dbt, dbias):
    _gate(f"{tag} dy", _err(dy, ref["dy"]), 3e-5 * max(1.0, float(ref["dy"].abs().max())))
    _gate(f"{tag} dgamma", _rel(dgm, ref["dgamma"]), 1e-4)
    _gate(f"{tag} dbeta", _rel(dbt, ref["dbeta"]), 1e-4)
    if dbias is not None:
        _gate(f"{tag} dbias", float(dbias.abs().max()), 1e-3 * max(1.0, float(ref["da"].abs().sum()) ** 0.5))


def _train_once(c, relu, op, ref, ws):
    """One training forward and the backward from the save it wrote; every operand a view in a NaN-filled allocation."""
    g = _g()
    d = g.dev()
    y, a = View(op["y"], c.off), View(op["y"].shape, c.off)
    da, dy = View(ref["da"], c.off), View(op["y"].shape, c.off)
    for v in (y, a, da, dy):
        assert v.aligned() == R.aligned(c)           # the route the table claims is the one these pointers take
    gm, bt, rm, rv = (_dev(op[k]) for k in ("gamma", "beta", "rm", "rv"))
    save, slot = torch.full((2 * c.C,), NAN, device=d), _slot()
    g.call("uz_bn_relu_fwd", y.ptr, c.C, y.ctot, gm, bt, rm, rv, save, a.ptr, a.ctot, c.N, c.H, c.W, R.EPS, R.MOMENTUM, 1, relu, slot, ws)
    dgm, dbt, dbias = (torch.full((c.C,), NAN, device=d) for _ in range(3))
    g.call("uz_bn_relu_bwd", da.ptr, da.ctot, y.ptr, c.C, y.ctot, gm, bt, save, dy.ptr, dy.ctot, dgm, dbt, dbias, c.N, c.H, c.W, relu, None, ws)
    assert y.untouched() and da.untouched() and a.outside_kept() and dy.outside_kept()
    return dict(a=a.get(), save=save.cpu(), rm=None if rm is None else rm.cpu(), rv=None if rv is None else rv.cpu(), slot=slot.cpu(),
                dy=dy.get(), dgamma=dgm.cpu(), dbeta=dbt.cpu(), dbias=dbias.cpu())


@pytest.mark.parametrize("case,relu", TRAIN, ids=[_id(p) for p in TRAIN])
def test_training_forward_and_backward(case, relu):
    c, op, ref = case, R.operands(case), R.reference(case, relu)
    ws = _ws(c)
    out = _train_once(c, relu, op, ref, ws)
    _check_forward(R.case_id(c), ref, out["a"], out["save"], out["rm"], out["rv"], out["slot"])
    _check_backward(R.case_id(c), ref, out["dy"], out["dgamma"], out["dbeta"], out["dbias"])
    # "bitwise reproducible; no atomics" (csrc/bn.hip): an identical second run repeats every output bit for bit
    again = _train_once(c, relu, op, ref, ws)
    for k, v in out.items():
        if v is not None:
            assert torch.equal(_bits(v), _bits(again[k])), f"{R.case_id(c)}: {k} differs between two identical runs"
    if op["rm"] is None:
        return
    # eval mode from given running statistics (at a mid size: the large apply pass alone)
    g = _g()
    y, a = View(op["y"], c.off), View(op["y"].shape, c.off)
    g.call("uz_bn_relu_fwd", y.ptr, c.C, y.ctot, _dev(op["gamma"]), _dev(op["beta"]), _dev(op["rm"]), _dev(op["rv"]), None, a.ptr, a.ctot,
           c.N, c.H, c.W, R.EPS, R.MOMENTUM, 0, relu, None, ws)
    _gate(f"{R.case_id(c)} eval a", _err(a.get(), ref["a_eval"]), 2e-5)
    assert y.untouched() and a.outside_kept()


@pytest.mark.parametrize("case,relu", EVAL, ids=[_id(p) for p in EVAL])
def test_eval_forward_at_a_mid_size(case, relu):
    g = _g()
    c, op, ref = case, R.operands(case), R.reference(case, relu)
    y, a = View(op["y"], c.off), View(op["y"].shape, c.off)
    rm, rv, slot = _dev(op["rm"]), _dev(op["rv"]), _slot()
    g.call("uz_bn_relu_fwd", y.ptr, c.C, y.ctot, _dev(op["gamma"]), _dev(op["beta"]), rm, rv, None, a.ptr, a.ctot,
           c.N, c.H, c.W, R.EPS, R.MOMENTUM, 0, relu, slot, None)            # no statistics pass: no workspace either
    _gate(f"{R.case_id(c)} eval a", _err(a.get(), ref["a_eval"]), 2e-5)
    top = float(ref["a_eval"].abs().max())
    assert top * (1 - 1e-5) <= float(slot.max()) <= top * 1.001
    assert torch.equal(rm.cpu(), op["rm"]) and torch.equal(rv.cpu(), op["rv"])      # eval mode leaves the running statistics alone
    assert y.untouched() and a.outside_kept()


def test_one_value_per_channel_is_refused_before_any_launch():
    """(1, C, 1, 1) in training mode: an error like torch's, and nothing written."""
    g = _g()
    c = next(c for c in R.CASES if c.o("refused"))
    op = R.operands(c)
    d = g.dev()
    y, a = View(op["y"]), View(op["y"].shape)
    rm, rv = _dev(op["rm"]), _dev(op["rv"])
    save, slot, ws = torch.full((2 * c.C,), NAN, device=d), _slot(), _ws(c)
    rc = g.L().uz_bn_relu_fwd(y.ptr.data_ptr(), c.C, y.ctot, _dev(op["gamma"]).data_ptr(), _dev(op["beta"]).data_ptr(), rm.data_ptr(), rv.data_ptr(),
                              save.data_ptr(), a.ptr.data_ptr(), a.ctot, c.N, c.H, c.W, R.EPS, R.MOMENTUM, 1, 1, slot.data_ptr(), ws.data_ptr(), g.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"more than 1 value" in g.L().uz_last_error()
    assert a.untouched() and y.untouched() and bool(torch.isnan(save).all()) and float(slot.abs().max()) == 0.0
    assert torch.equal(rm.cpu(), op["rm"]) and torch.equal(rv.cpu(), op["rv"])


@pytest.mark.parametrize("case", R.UNBIASED_CASES, ids=R.case_id)
def test_running_variance_takes_the_unbiased_factor(case):
    """n / (n - 1) at n = 2, 512 and 513, where the running-variance gate cannot hide it: with momentum 1 the running variance IS the
    unbiased batch variance, compared per channel at 1e-6 relative with fp64."""
    g = _g()
    c, op, ref = case, R.operands(case), R.reference(case, 1)
    d = g.dev()
    n = c.N * c.H * c.W
    y, a = View(op["y"]), View(op["y"].shape)
    rm, rv, save = torch.zeros(c.C, device=d), torch.zeros(c.C, device=d), torch.empty(2 * c.C, device=d)
    g.call("uz_bn_relu_fwd", y.ptr, c.C, y.ctot, _dev(op["gamma"]), _dev(op["beta"]), rm, rv, save, a.ptr, a.ctot, c.N, c.H, c.W, R.EPS, 1.0, 1, 1, None, _ws(c))
    want = ref["var"] * (n / (n - 1.0))
    err = float(((rv.cpu().double() - want).abs() / want).max())
    print(f"{R.case_id(c)}: unbiased variance off by {err:.3e} (biased would be off by {1.0 / n:.3e})")
    assert err <= 1e-6
    assert float(((rm.cpu().double() - ref["mean"]).abs() / ref["mean"].abs().clamp_min(1.0)).max()) <= 1e-6


# ---------------------------------------------------------------- folded inputs, synthesised on the host
def _rows_of(c, rows, *cols):
    """[rows][C][len(cols)] fp32 partials: the pixels of a channel (image-major) cut into `rows` slices, each column reduced per
    slice - ("sum", t) or ("max", t) with t an fp64 NCHW tensor."""
    out = torch.empty(rows, c.C, len(cols), dtype=torch.float64)
    for k, (how, t) in enumerate(cols):
        for r, piece in enumerate(torch.tensor_split(t.permute(1, 0, 2, 3).reshape(c.C, -1), rows, dim=1)):
            out[r, :, k] = piece.sum(1) if how == "sum" else piece.amax(1)
    return out.float().contiguous().to(_g().dev())


@pytest.mark.parametrize("rows", R.PARTIAL_ROWS)
@pytest.mark.parametrize("case", R.PARTIAL_CASES, ids=R.case_id)
def test_forward_statistics_from_convolution_partials(case, rows):
    g = _g()
    c, op, ref = case, R.operands(case), R.reference(case, 1)
    d, tag = g.dev(), f"{R.case_id(case)} rows {rows}"
    y64 = op["y"].double()
    part = _rows_of(c, rows, ("sum", y64), ("sum", y64 * y64), ("max", y64), ("max", -y64))
    y, ws = View(op["y"]), _ws(c)
    gm, bt = _dev(op["gamma"]), _dev(op["beta"])
    args = (c.N, c.H, c.W, R.EPS, R.MOMENTUM)
    # the stand-alone statistics pass
    a0, save0 = View(op["y"].shape), torch.empty(2 * c.C, device=d)
    g.call("uz_bn_relu_fwd", y.ptr, c.C, y.ctot, gm, bt, None, None, save0, a0.ptr, a0.ctot, *args, 1, 1, None, ws)
    # _pre
    a1, save1, slot1, rm1, rv1 = View(op["y"].shape), torch.empty(2 * c.C, device=d), _slot(), _dev(op["rm"]), _dev(op["rv"])
    g.call("uz_bn_relu_fwd_pre", y.ptr, c.C, y.ctot, gm, bt, rm1, rv1, save1, a1.ptr, a1.ctot, *args, 1, 1, slot1, ws, part, rows)
    _check_forward(tag + " pre", ref, a1.get(), save1.cpu(), rm1.cpu(), rv1.cpu(), slot1.cpu(), gate_a=3e-5)
    _gate(tag + " save against the stand-alone pass", g.relerr(save1, save0), 2e-6)
    assert a1.outside_kept()
    # _ex: the 4 C table (mean, rstd, alpha, beta')
    a2, save2, slot2, rm2, rv2 = View(op["y"].shape), torch.full((4 * c.C,), NAN, device=d), _slot(), _dev(op["rm"]), _dev(op["rv"])
    g.call("uz_bn_relu_fwd_ex", y.ptr, c.C, y.ctot, gm, bt, rm2, rv2, save2, a2.ptr, a2.ctot, *args, 1, 1, slot2, ws, part, rows, 0)
    _check_forward(tag + " ex", ref, a2.get(), save2.cpu(), rm2.cpu(), rv2.cpu(), slot2.cpu(), gate_a=3e-5)
    _gate(tag + " alpha", _rel(save2[2 * c.C:3 * c.C], ref["alpha"]), 2e-6)
    _gate(tag + " beta'", _err(save2[3 * c.C:], ref["beta_"]) / max(1.0, float(ref["beta_"].abs().max())), 2e-6)
    assert torch.equal(save2[:2 * c.C], save1) and a2.outside_kept()
    if c.N * c.H * c.W <= g.L().uz_bn_fwd_fused_limit(c.H, c.W):
        return                                      # the two-phase form serves the planes beyond the one-launch limit only
    # _phase 1: statistics, table and bound; y is not read (null here) and a keeps its bits
    a3, save3, slot3, rm3, rv3 = View(op["y"].shape), torch.full((4 * c.C,), NAN, device=d), _slot(), _dev(op["rm"]), _dev(op["rv"])
    g.call("uz_bn_relu_fwd_phase", None, c.C, y.ctot, gm, bt, rm3, rv3, save3, a3.ptr, a3.ctot, *args, 1, slot3, part, rows, 0, 1)
    assert a3.untouched()
    assert torch.equal(save3, save2) and torch.equal(rm3, rm2) and torch.equal(rv3, rv2) and torch.equal(slot3, slot2)
    # _phase 2: the apply pass alone, from the table phase 1 left
    g.call("uz_bn_relu_fwd_phase", y.ptr, c.C, y.ctot, gm, bt, rm3, rv3, save3, a3.ptr, a3.ctot, *args, 1, slot3, None, 0, 0, 2)
    _check_forward(tag + " phase", ref, a3.get(), save3.cpu(), rm3.cpu(), rv3.cpu(), slot3.cpu(), gate_a=3e-5)
    assert torch.equal(rm3, rm2) and a3.outside_kept() and y.untouched()


@pytest.mark.parametrize("rows", R.PARTIAL_ROWS)
@pytest.mark.parametrize("case", R.PARTIAL_CASES, ids=R.case_id)
def test_backward_sums_from_data_gradient_partials(case, rows):
    """conv_partials rows {sum dz, sum dz x_hat, max |dz|, max |x_hat|} from a dA that already carries the mask, the conv-bias
    gradient through dbias_partials + uz_chan_sum_partials_d where the shape has rows for it."""
    g = _g()
    c, op, ref = case, R.operands(case), R.reference(case, 1)
    d, tag = g.dev(), f"{R.case_id(case)} rows {rows}"
    part = _rows_of(c, rows, ("sum", ref["dz"]), ("sum", ref["dz"] * ref["xh"]), ("max", ref["dz"].abs()), ("max", ref["xh"].abs()))
    y, da, dy, ws = View(op["y"]), View(ref["dz"].float()), View(op["y"].shape), _ws(c)
    gm, bt = _dev(op["gamma"]), _dev(op["beta"])
    save = torch.cat([ref["mean"], ref["rstd"]]).float().to(d)
    dgm, dbt, dbias = (torch.full((c.C,), NAN, device=d) for _ in range(3))
    nrow = g.L().uz_bn_bwd_dbias_rows(c.N, c.H, c.W)
    if nrow:
        dpart = torch.full((nrow, c.C), NAN, device=d, dtype=torch.float64)
        g.call("uz_bn_relu_bwd_ex", da.ptr, da.ctot, y.ptr, c.C, y.ctot, gm, bt, save, dy.ptr, dy.ctot, dgm, dbt, None, c.N, c.H, c.W, 1, None, ws,
               part, rows, 0, dpart, None, 0)
        g.call("uz_chan_sum_partials_d", dpart, nrow, c.C, dbias)
    else:                                           # within the one-launch limit a shape has no rows: the call sums dbias itself
        g.call("uz_bn_relu_bwd_ex", da.ptr, da.ctot, y.ptr, c.C, y.ctot, gm, bt, save, dy.ptr, dy.ctot, dgm, dbt, dbias, c.N, c.H, c.W, 1, None, ws,
               part, rows, 0, None, None, 0)
    _check_backward(tag, ref, dy.get(), dgm.cpu(), dbt.cpu(), dbias.cpu())
    assert dy.outside_kept() and y.untouched() and da.untouched()


@pytest.mark.parametrize("nslab", R.SLAB_COUNTS)
@pytest.mark.parametrize("case", R.SLAB_CASES, ids=R.case_id)
def test_small_path_sums_split_k_slabs(case, nslab):
    """uz_bn_relu_fwd_slabs / da_slabs: y (dA) = the slabs added in order, in fp32 - y is written, bit for bit that sum."""
    g = _g()
    c, op = case, R.operands(case)
    d, tag = g.dev(), f"{R.case_id(case)} slabs {nslab}"
    shape = (c.N, c.C, c.H, c.W)
    bias = R._rnd(c.C, seed=31) * 0.5 + 0.7
    ys = [R._rnd(*shape, seed=40 + k) * (2.0 / nslab ** 0.5) for k in range(nslab)]
    yv = bias.view(1, -1, 1, 1).expand(shape).clone()
    for s in ys:
        yv = yv + s                                 # fp32, slab order
    ds = [R._rnd(*shape, seed=60 + k) / nslab ** 0.5 for k in range(nslab)]
    edge = R.reference_of(yv, ds[0], op["gamma"], op["beta"], op["rm"], op["rv"], 1)["edge"]
    ds = [torch.where(edge, torch.zeros(()), s) for s in ds]
    dav = torch.zeros(shape)
    for s in ds:
        dav = dav + s
    ref = R.reference_of(yv, dav, op["gamma"], op["beta"], op["rm"], op["rv"], 1)
    assert ref["edge_share"] <= R.RELU_EDGE_SHARE
    y, a, dy = View(shape), View(shape), View(shape)
    gm, bt, rm, rv = (_dev(op[k]) for k in ("gamma", "beta", "rm", "rv"))
    save, slot = torch.empty(2 * c.C, device=d), _slot()
    g.call("uz_bn_relu_fwd_slabs", torch.stack(ys).to(d), nslab, bias.to(d), y.ptr, c.C, y.ctot, gm, bt, rm, rv, save, a.ptr, a.ctot,
           c.N, c.H, c.W, R.EPS, R.MOMENTUM, 1, 1, slot)
    assert torch.equal(_bits(y.get()), _bits(yv)), f"{tag}: y is not bias + slabs in order"
    _check_forward(tag, ref, a.get(), save.cpu(), rm.cpu(), rv.cpu(), slot.cpu())
    dgm, dbt, dbias = (torch.full((c.C,), NAN, device=d) for _ in range(3))
    g.call("uz_bn_relu_bwd_ex", None, c.C, y.ptr, c.C, y.ctot, gm, bt, save, dy.ptr, dy.ctot, dgm, dbt, dbias, c.N, c.H, c.W, 1, None, None,
           None, 0, 0, None, torch.stack(ds).to(d), nslab)
    _check_backward(tag, ref, dy.get(), dgm.cpu(), dbt.cpu(), dbias.cpu())
    assert y.outside_kept() and a.outside_kept() and dy.outside_kept()


def _flags(clear):
    g = _g()
    out = ctypes.c_int(0)
    from unet_zoo_amd import _ffi
    _ffi.check(g.L().uz_device_flags(ctypes.byref(out), clear, g.stream()), "device_flags")
    return out.value


def _unpack(packed, slot):
    out = torch.empty_like(packed)
    _g().call("uz_unpack_split", packed, out, packed.numel(), slot)
    return out


@pytest.mark.parametrize("case", R.PACKED_CASES, ids=R.case_id)
def test_split_storage_output(case):
    """out_packed on the mid path (a-priori bound) and on the large path (bound from the partials), forward and backward, read back
    through uz_unpack_split at the gate tests/test_split_storage_gpu.py holds packed BatchNorm output to (3e-5 of the maximum);
    the device flag word stays clear."""
    g = _g()
    c, op, ref = case, R.operands(case), R.reference(case, 1)
    d, tag = g.dev(), R.case_id(case)
    y64 = op["y"].double()
    mid = c.claims[0][1][0] == R.MID
    part, rows = (None, 0) if mid else (_rows_of(c, 3, ("sum", y64), ("sum", y64 * y64), ("max", y64), ("max", -y64)), 3)
    y, da, ws = View(op["y"]), View(ref["da"]), _ws(c)
    gm, bt = _dev(op["gamma"]), _dev(op["beta"])
    _flags(1)
    a, save, slot = torch.full(op["y"].shape, NAN, device=d), torch.empty(4 * c.C, device=d), _slot()
    g.call("uz_bn_relu_fwd_ex", y.ptr, c.C, y.ctot, gm, bt, None, None, save, a, c.C, c.N, c.H, c.W, R.EPS, R.MOMENTUM, 1, 1, slot, ws, part, rows, 1)
    _gate(tag + " a", _err(_unpack(a, slot), ref["a"]), 3e-5 * float(ref["a"].abs().max()))
    assert float(slot.max()) >= float(ref["a"].abs().max()) * (1 - 1e-5)
    dy, dslot = torch.full(op["y"].shape, NAN, device=d), _slot()
    dgm, dbt, dbias = (torch.full((c.C,), NAN, device=d) for _ in range(3))
    g.call("uz_bn_relu_bwd_ex", da.ptr, da.ctot, y.ptr, c.C, y.ctot, gm, bt, save, dy, c.C, dgm, dbt, dbias, c.N, c.H, c.W, 1, dslot, ws,
           None, 0, 1, None, None, 0)
    assert float(dslot.max()) >= float(ref["dy"].abs().max()) * (1 - 1e-5)
    _check_backward(tag, ref, _unpack(dy, dslot), dgm.cpu(), dbt.cpu(), dbias.cpu())
    assert _flags(0) == 0
    assert y.untouched() and da.untouched()


# ---------------------------------------------------------------- bf16 storage
def _b16_close(what, got, ref, stored_b16, fp32_gate):
    """The gate of tests/test_b16_storage_gpu.py::test_batchnorm_in_bf16_storage for a stored tensor - one bf16 ulp, 2^-7 of the
    value - on top of the fp32 gate of the same quantity (there the comparison is with the fp32-storage kernel; here with fp64,
    which the fp32-storage kernel is itself held to at that gate)."""
    got, ref = got.double(), ref.double()
    over = (got - ref).abs() - (ref.abs() * 2.0 ** -7 if stored_b16 else 0.0)
    _gate(what, float(over.max()), fp32_gate)


@pytest.mark.parametrize("case", B16, ids=R.case_id)
def test_bf16_storage_in_every_combination(case):
    g = _g()
    c, op, ref = case, R.operands(case), R.reference(case, 1)          # operands are bf16-representable
    d, tag = g.dev(), R.case_id(case)
    ws = _ws(c, 64)
    gm, bt = _dev(op["gamma"]), _dev(op["beta"])
    ty = {0: torch.float32, 1: torch.bfloat16}
    ys = {b: View(op["y"], dtype=ty[b]) for b in (0, 1)}
    das = {b: View(ref["da"], dtype=ty[b]) for b in (0, 1)}
    stats = torch.cat([ref["mean"], ref["rstd"]]).float()
    save = None
    for yb, ab in ([(1, 1)] if c.o("big") else [(0, 0), (0, 1), (1, 0), (1, 1)]):
        y, a = ys[yb], View(op["y"].shape, dtype=ty[ab])
        assert y.aligned() and a.aligned()
        rm, rv, save = _dev(op["rm"]), _dev(op["rv"]), torch.full((2 * c.C,), NAN, device=d)
        g.call("uz_bn_relu_fwd_b16", y.ptr, c.C, y.ctot, gm, bt, rm, rv, save, a.ptr, a.ctot, c.N, c.H, c.W, R.EPS, R.MOMENTUM, 1, 1, ws, None, 0, yb, ab)
        assert torch.allclose(save.cpu(), stats, rtol=2e-6, atol=1e-7), (tag, yb, ab)
        assert torch.allclose(rm.cpu(), ref["rm"].float(), rtol=1e-5, atol=1e-8) and torch.allclose(rv.cpu(), ref["rv"].float(), rtol=1e-5)
        _b16_close(f"{tag} y{yb} a{ab} a", a.get(), ref["a"], ab, 2e-5)
        assert a.outside_kept() and y.untouched()
    for dab, yb, dyb in ([(1, 1, 1)] if c.o("big") else [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]):
        da, y, dy = das[dab], ys[yb], View(op["y"].shape, dtype=ty[dyb])
        assert da.aligned() and dy.aligned()
        dgm, dbt, dbias = (torch.full((c.C,), NAN, device=d) for _ in range(3))
        g.call("uz_bn_relu_bwd_b16", da.ptr, da.ctot, y.ptr, c.C, y.ctot, gm, bt, save, dy.ptr, dy.ctot, dgm, dbt, dbias, c.N, c.H, c.W, 1, ws, dab, yb, dyb)
        t = f"{tag} da{dab} y{yb} dy{dyb}"
        assert torch.allclose(dgm.cpu(), ref["dgamma"].float(), rtol=1e-5, atol=1e-3) and torch.allclose(dbt.cpu(), ref["dbeta"].float(), rtol=1e-5, atol=1e-3), t
        got = dy.get()
        _b16_close(t + " dy", got, ref["dy"], dyb, 3e-5 * max(1.0, float(ref["dy"].abs().max())))
        # the conv-bias gradient is the sum of the STORED dy
        assert torch.allclose(dbias.cpu().double(), got.double().sum((0, 2, 3)), rtol=1e-6, atol=1e-3), t
        assert dy.outside_kept() and y.untouched() and da.untouched()
