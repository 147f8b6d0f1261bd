"""Every case of tests/_aux_cases.py through the C ABI: the validation metrics, the batch assembly, the latent-noise stream with its
step counters and the posterior input, each against the fp64 reference of the same operation on the same operands.  Every operand
is a view inside a larger allocation filled with NaN (floats) or a sentinel (bytes, integers); inputs must keep every bit and
outputs every bit outside the view.  Gates (tests/_aux_cases.py): pair counts, posterior input and the rows of
the batch assembly that are exact by construction bit for bit; cross-entropy maps, images and noise 4 x the distance of the same
formulas in numpy float32 from fp64 on the same case; NCC 4 x 2^-24; labels equal wherever the fp64 margin is at least 1e-4.
`-s` prints every measured distance."""
import numpy as np
import pytest
import torch

from tests import _aux_cases as A

pytestmark = pytest.mark.gpu

PAD = 8                      # guard elements behind a view (and at least `off` in front of it)
BYTE_SENTINEL, INT_SENTINEL = 0xEE, -777


def _g():
    from tests import _gpu
    return _gpu


def _rc(name, *args):
    from tests import _views
    return _views.rc(name, *args)


class Buf:
    """A contiguous array that starts `off` elements into an allocation filled with NaN / a sentinel (data None: an output)."""
    BITS = {torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int32: torch.int32, torch.int64: torch.int64}
    FILL = {torch.float32: float("nan"), torch.uint8: BYTE_SENTINEL, torch.int32: INT_SENTINEL, torch.int64: INT_SENTINEL}

    def __init__(self, shape, dtype, off, data=None):
        self.n, self.off = int(np.prod(shape, dtype=np.int64)), off
        self.flat = torch.full((off + self.n + PAD,), self.FILL[dtype], dtype=dtype, device=_g().dev())
        self.ptr = self.flat[off:off + self.n]
        if data is not None:
            self.ptr.copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(-1).to(dtype))
        self.shape, self.bits = tuple(shape), self.BITS[dtype]
        self.before = self.flat.clone()
        assert self.flat.data_ptr() % 256 == 0

    def get(self):
        return self.ptr.cpu().numpy().reshape(self.shape)

    def outside_untouched(self):
        a, b = self.flat.view(self.bits), self.before.view(self.bits)
        return torch.equal(a[:self.off], b[:self.off]) and torch.equal(a[self.off + self.n:], b[self.off + self.n:])

    def untouched(self):
        return torch.equal(self.flat.view(self.bits), self.before.view(self.bits))


def _close(got, ref, gate, what):
    err = A.rel_err(got, ref)
    print(f"{what}: error {err:.3e} (gate {gate:.3e})")
    assert err <= gate, f"{what}: error {err:.3e} of max(1, max |ref|) exceeds {gate:.3e}"


# ================================================================================================ validation metrics
@pytest.mark.parametrize("Na,Nb", A.PC_NANB)
@pytest.mark.parametrize("HW", A.PC_HW)
def test_pair_counts_are_exact(HW, Na, Nb):
    g = _g()
    a, b = A.pc_maps(HW, Na, Nb)
    for oa, ob in A.PC_OFFSETS:
        av, bv = Buf(a.shape, torch.uint8, oa, a), Buf(b.shape, torch.uint8, ob, b)
        assert av.ptr.data_ptr() % 2 == oa % 2 and bv.ptr.data_ptr() % 2 == ob % 2
        for label in A.PC_LABELS:
            out = Buf((Na * Nb * 3,), torch.int32, 8)
            g.call("uz_label_pair_counts", av.ptr, Na, bv.ptr, Nb, HW, label, out.ptr)
            assert np.array_equal(out.get().astype(np.int64), A.pc_ref(a, b, label)), (HW, Na, Nb, label, oa, ob)
            assert out.outside_untouched()
        assert av.untouched() and bv.untouched()


def test_pair_counts_refuse_a_grid_beyond_65535():
    a, b, out = Buf((4,), torch.uint8, 0, np.zeros(4, np.uint8)), Buf((4,), torch.uint8, 0, np.zeros(4, np.uint8)), Buf((12,), torch.int32, 8)
    assert _rc("uz_label_pair_counts", a.ptr, 1, b.ptr, 65536, 4, 0, out.ptr) != 0
    assert out.untouched()


@pytest.mark.parametrize("N,M,K", A.NM_NMK)
@pytest.mark.parametrize("HW", A.NM_HW)
def test_ncc_maps_against_fp64(HW, N, M, K):
    g = _g()
    soft, gt = A.nm_operands(N, M, K, HW)
    ess_ref, esy_ref = A.nm_ref(soft, gt)
    f32 = A.NM_F32[A.nm_id(N, M, K, HW)]
    sv, gv = Buf(soft.shape, torch.float32, 3, soft), Buf(gt.shape, torch.float32, 1, gt)
    ess, esy = Buf((HW,), torch.float32, 5), Buf((M, HW), torch.float32, 2)
    g.call("uz_ncc_maps", sv.ptr, gv.ptr, N, M, K, HW, ess.ptr, esy.ptr)
    assert sv.untouched() and gv.untouched() and ess.outside_untouched() and esy.outside_untouched()
    _close(ess.get(), ess_ref, 4 * f32[0], f"E_ss {A.nm_id(N, M, K, HW)}")
    _close(esy.get(), esy_ref, 4 * f32[1], f"E_sy {A.nm_id(N, M, K, HW)}")


@pytest.mark.parametrize("M", A.NCC_M)
@pytest.mark.parametrize("HW", A.NCC_HW)
def test_ncc_against_two_pass_fp64(HW, M):
    g = _g()
    a, v = A.ncc_operands(M, HW)
    ref = A.ncc_ref(a, v)
    av, vv, out = Buf(a.shape, torch.float32, 1, a), Buf(v.shape, torch.float32, 3, v), Buf((M,), torch.float32, 5)
    g.call("uz_ncc", av.ptr, vv.ptr, M, HW, out.ptr)
    assert av.untouched() and vv.untouched() and out.outside_untouched()
    got = out.get().astype(np.float64)
    if HW == 1:                 # a single pixel is a constant map: 0 / 0 in the reference and in the kernel
        assert np.isnan(ref).all() and np.isnan(got).all()
        return
    err = float(np.abs(got - ref).max())
    print(f"ncc M={M} HW={HW}: error {err:.3e} (gate {A.NCC_GATE:.3e})")
    assert err <= A.NCC_GATE, (err, got, ref)


def test_metrics_end_to_end_three_labels_and_an_empty_mask():
    from oracle import metrics as OM
    from unet_zoo_amd import metrics as DM
    dev = _g().dev()
    s, gts, soft = A.e2e_operands()
    st, gt_t = torch.from_numpy(s).to(dev), torch.from_numpy(gts).to(dev)
    ged = DM.generalised_energy_distance(st, gt_t, nlabels=3, label_range=range(3))
    ged_ref = OM.generalised_energy_distance(s, gts, nlabels=3, label_range=range(3))
    assert abs(ged - ged_ref) <= 1e-12, (ged, ged_ref)
    for i, j in [(0, 0), (3, 2), (1, 2), (3, 1)]:                 # (3, .): a prediction without label 2; (., 2): the empty mask
        d, d_ref = DM.per_label_dice(st[i], gt_t[j], 3), OM.per_label_dice(s[i], gts[j], 3)
        assert np.allclose(d, d_ref, atol=1e-12, rtol=0), (i, j, d, d_ref)
    onehot = np.stack([(gts == k) for k in range(3)], axis=1).astype(np.int64)
    ncc = DM.variance_ncc_dist(torch.from_numpy(soft).to(dev), torch.from_numpy(onehot).to(dev))
    ncc_ref = float(np.asarray(OM.variance_ncc_dist(soft, onehot)).reshape(-1)[0])
    print(f"end to end: GED {ged:.12f} ({ged_ref:.12f}), NCC {ncc:.8f} ({ncc_ref:.8f})")
    assert abs(ncc - ncc_ref) <= 1e-5, (ncc, ncc_ref)


# ================================================================================================ batch assembly
def _augment_call(case, X, Y, nlabels=None, B=None, null=None):
    """The operands of one uz_augment_batch call as guarded views; returns (return code, operands)."""
    rows = np.asarray(case.rows, np.float32)
    Bn = len(case.rows)
    ops = dict(X=Buf(X.shape, torch.float32, 1, X), Y=Buf(Y.shape, torch.uint8, 3, Y), idx=Buf((Bn,), torch.int32, 1, np.asarray(case.idx[:Bn], np.int32)),
               ann=Buf((Bn,), torch.int32, 3, np.asarray(case.ann[:Bn], np.int32)), prm=Buf(rows.shape, torch.float32, 2, rows),
               xo=Buf((Bn, 1, case.H, case.W), torch.float32, 7), so=Buf((Bn, case.H, case.W), torch.float32, 5))
    args = [None if null == k else ops[k].ptr for k in ("X", "Y")] + [case.H, case.W, case.A] + \
           [None if null == k else ops[k].ptr for k in ("idx", "ann", "prm")] + [Bn if B is None else B, case.nlabels if nlabels is None else nlabels] + \
           [None if null == k else ops[k].ptr for k in ("xo", "so")]
    return _rc("uz_augment_batch", *args), ops


@pytest.mark.parametrize("case", A.AUG_CASES, ids=lambda c: c.name)
def test_batch_assembly_against_the_fp64_twin(case):
    X, Y = A.aug_dataset(case)
    img_ref, lbl_ref, margin = A.aug_ref(case, X=X, Y=Y)
    rc, ops = _augment_call(case, X, Y)
    assert rc == 0
    for k in ("X", "Y", "idx", "ann", "prm"):
        assert ops[k].untouched(), k
    assert ops["xo"].outside_untouched() and ops["so"].outside_untouched()
    img, lbl = ops["xo"].get()[:, 0], ops["so"].get()
    exact = np.array([A.aug_row_exact(case, r) for r in case.rows])
    for b in np.nonzero(exact)[0]:
        assert np.array_equal(img[b].astype(np.float64), img_ref[b]), f"row {b}: exact by construction, image differs"
        assert np.array_equal(lbl[b].astype(np.int64), lbl_ref[b]), f"row {b}: exact by construction, labels differ"
    if not exact.all():
        gate = min(4 * A.AUG_F32[case.name], A.AUG_IMAGE_FLOOR)
        _close(img[~exact], img_ref[~exact], gate, f"augment {case.name} image")
        safe = margin[~exact] >= A.AUG_MARGIN
        wrong = (lbl[~exact].astype(np.int64) != lbl_ref[~exact]) & safe
        print(f"augment {case.name}: {int((~safe).sum())} of {safe.size} labels below the margin, "
              f"{int((lbl[~exact].astype(np.int64) != lbl_ref[~exact]).sum())} differ in all")
        assert not wrong.any(), f"{int(wrong.sum())} labels differ where the fp64 margin is at least {A.AUG_MARGIN:g}"


def test_batch_assembly_refuses_bad_calls():
    case = A.AUG_CASES[4]
    X, Y = A.aug_dataset(case)
    for kw in (dict(nlabels=9), dict(B=0), dict(null="prm"), dict(null="so")):
        rc, ops = _augment_call(case, X, Y, **kw)
        assert rc != 0, kw
        assert ops["xo"].untouched() and ops["so"].untouched(), kw


# ================================================================================================ latent noise and counters
def _state(seed, offset):
    def i64(v):
        return v - 2 ** 64 if v >= 2 ** 63 else v
    return Buf((2,), torch.int64, 2, np.array([i64(seed), i64(offset & (2 ** 64 - 1))], np.int64))


def _noise_gate(case):
    return 4 * A.NOISE_F32[A.noise_id(case)] if A.NOISE_GATE is None else A.NOISE_GATE


@pytest.mark.parametrize("case", A.NOISE_CASES, ids=A.noise_id)
def test_noise_stream_is_philox4x32_10_with_box_muller(case):
    g = _g()
    seed, offset, n = case
    ref = A.noise_ref(seed, offset, n)
    st, dst = _state(seed, offset), Buf((n,), torch.float32, 5)
    g.call("uz_randn_fill", dst.ptr, n, st.ptr)
    assert st.untouched() and dst.outside_untouched()
    err = float(np.abs(dst.get().astype(np.float64) - ref).max())          # NaN (unwritten) fails the comparison below
    print(f"noise {A.noise_id(case)}: max |got - fp64| {err:.3e} (numpy float32 {A.NOISE_F32[A.noise_id(case)]:.3e}, gate {_noise_gate(case):.3e})")
    assert err <= _noise_gate(case), (A.noise_id(case), err)


def test_noise_of_no_elements_touches_nothing():
    st, dst = _state(12345, 0), Buf((4,), torch.float32, 5)
    assert _rc("uz_randn_fill", dst.ptr, 0, st.ptr) == 0
    assert st.untouched() and dst.untouched()


def test_noise_stream_continues_behind_step_counters():
    g = _g()
    seed, offset, n1, n2 = A.SEED2, 2 ** 32 - 3, 10, 7
    st, d1, d2 = _state(seed, offset), Buf((n1,), torch.float32, 1), Buf((n2,), torch.float32, 3)
    g.call("uz_randn_fill", d1.ptr, n1, st.ptr)
    g.call("uz_step_counters", None, None, 0, st.ptr, (n1 + 3) // 4)
    g.call("uz_randn_fill", d2.ptr, n2, st.ptr)
    assert st.outside_untouched() and d1.outside_untouched() and d2.outside_untouched()
    assert st.get().tolist() == [seed - 2 ** 64, offset + (n1 + 3) // 4]
    for d, o, n in ((d1, offset, n1), (d2, offset + (n1 + 3) // 4, n2)):
        gate = 4 * A.noise_f32_error((seed, o, n)) if A.NOISE_GATE is None else A.NOISE_GATE
        err = float(np.abs(d.get().astype(np.float64) - A.noise_ref(seed, o, n)).max())
        print(f"noise continuity at {o:x}: {err:.3e}")
        assert err <= gate, (o, err)


def test_step_counters_over_two_workgroups_and_with_an_advance():
    g = _g()
    rs = np.random.default_rng(3)
    idx = rs.permutation(A.COUNTERS_N)[:A.COUNTERS_IDX].astype(np.int64)
    start = rs.integers(0, 1000, A.COUNTERS_N).astype(np.int64)
    cnt, iv, st = Buf((A.COUNTERS_N,), torch.int64, 3, start), Buf(idx.shape, torch.int64, 1, idx), _state(A.SEED2, 2 ** 40)
    g.call("uz_step_counters", cnt.ptr, iv.ptr, A.COUNTERS_IDX, None, 0)
    want = start.copy()
    want[idx] += 1
    assert np.array_equal(cnt.get(), want) and cnt.outside_untouched() and iv.untouched() and st.untouched()
    g.call("uz_step_counters", cnt.ptr, iv.ptr, A.COUNTERS_IDX, st.ptr, 12345678901)             # counts and advances in one launch
    want[idx] += 1
    assert np.array_equal(cnt.get(), want) and cnt.outside_untouched() and iv.untouched() and st.outside_untouched()
    assert st.get().tolist() == [A.SEED2 - 2 ** 64, 2 ** 40 + 12345678901]


# ================================================================================================ posterior input
@pytest.mark.parametrize("in_ch,nlabels", A.PI_CH)
@pytest.mark.parametrize("H,W", A.PI_HW)
def test_posterior_input_is_exact(H, W, in_ch, nlabels):
    g = _g()
    patch, mask, ref = A.pi_operands(H, W, in_ch, nlabels)
    pv, mv, out = Buf(patch.shape, torch.float32, 1, patch), Buf(mask.shape, torch.float32, 3, mask), Buf(ref.shape, torch.float32, 5)
    g.call("uz_posterior_input", pv.ptr, in_ch, mv.ptr, nlabels, out.ptr, A.PI_N, H, W)
    assert pv.untouched() and mv.untouched() and out.outside_untouched()
    assert np.array_equal(out.get().view(np.int32), ref.view(np.int32))
