"""The references and case lists of tests/_aux_cases.py, checked without a GPU: the Philox twin against the published known-answer
vectors, the gate tables recomputed, the margin cap of the batch-assembly cases, the float32 default of oracle/augment.py - and that
the cases DISCRIMINATE: each deliberately wrong twin below changes the expected output of a named case beyond that case's gate, so a
kernel with the same mistake fails tests/test_aux_cases_gpu.py."""
import numpy as np
import pytest

from tests import _aux_cases as A


# ------------------------------------------------------------------------------------------------ the Philox twin
@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_twin_gives_the_known_answers(ctr, key, want):
    out = A.philox4x32([np.array([c], np.uint64) for c in ctr], [np.array([k], np.uint64) for k in key])
    assert " ".join(f"{int(w[0]):08x}" for w in out) == want


def test_noise_twin_lays_its_counters_out_as_the_kernel_does():
    seed, offset = A.SEED2, 2 ** 32 - 2
    w = A.noise_words(seed, offset, 16)
    for q in (0, 1, 2, 3):                                      # q = 2 carries into the high counter word
        c = offset + q
        one = A.philox4x32([np.array([c & 0xFFFFFFFF], np.uint64), np.array([c >> 32], np.uint64), np.array([0x5A5A5A5A], np.uint64), np.array([0], np.uint64)],
                           [np.array([seed & 0xFFFFFFFF], np.uint64), np.array([seed >> 32], np.uint64)])
        assert [int(x[0]) for x in one] == [int(x) for x in w[q]]
    x = A.noise_ref(12345, 0, 1 << 16)
    assert abs(x.mean()) < 2e-2 and abs(x.std() - 1) < 2e-2 and np.isfinite(x).all()
    assert np.array_equal(A.noise_ref(12345, 0, 9)[:5], A.noise_ref(12345, 0, 5))              # a ragged count is a prefix
    assert np.array_equal(A.noise_ref(12345, 2, 8), A.noise_ref(12345, 0, 16)[8:])            # the offset counts quads


def test_noise_gate_table_is_what_numpy_float32_measures():
    assert set(A.NOISE_F32) == {A.noise_id(c) for c in A.NOISE_CASES} and len(A.NOISE_F32) == len(A.NOISE_CASES)
    for c in A.NOISE_CASES:
        assert A.noise_f32_error(c) == pytest.approx(A.NOISE_F32[A.noise_id(c)], rel=1e-2), A.noise_id(c)


def _noise_gate(c):
    return 4 * A.NOISE_F32[A.noise_id(c)] if A.NOISE_GATE is None else A.NOISE_GATE


@pytest.mark.parametrize("defect,case", [
    ("ctr_hi", (A.SEED2, 2 ** 32 - 2, 16)), ("ctr_hi", (A.SEED2, 2 ** 40 + 7, 64)),
    ("key_hi", (0xDEADBEEF12345678, 0, 1025)), ("key_hi", (A.SEED2, 3, 4 * A.VGRID_QUADS + 5)),
    ("rounds", (12345, 0, 1)), ("rounds", (0xDEADBEEF12345678, 0, 1025)),
    ("stride", (A.SEED2, 3, 4 * A.VGRID_QUADS + 5)),
])
def test_a_wrong_noise_twin_fails_a_case(defect, case):
    assert case in A.NOISE_CASES
    good, bad = A.noise_ref(*case), A.noise_ref(*case, defects=(defect,))
    d = np.abs(bad - good)
    err = float("inf") if np.isnan(d).any() else float(d.max())
    assert err > 100 * _noise_gate(case), (defect, A.noise_id(case), err)
    if defect == "ctr_hi":                                     # and the cases of the old test (offset 0, seed 12345) would not have noticed
        assert np.array_equal(A.noise_ref(12345, 0, 64, defects=("ctr_hi", "key_hi")), A.noise_ref(12345, 0, 64))


# ------------------------------------------------------------------------------------------------ metrics
def test_pair_count_cases_cover_what_they_claim():
    for HW in A.PC_HW:
        for Na, Nb in A.PC_NANB:
            a, b = A.pc_maps(HW, Na, Nb)
            assert np.array_equal(b[Nb - 1], a[0])
            assert not (a == 7).any() and not (b == 7).any()
            if Nb > 1 and HW >= 63:
                assert (a == 3).any() and not (b[:Nb - 1] == 3).any() and (b == 255).any() and not (a == 255).any()
            ident = A.pc_ref(a, b, 1).reshape(Na, Nb, 3)[0, Nb - 1]
            assert ident[0] == ident[1] == ident[2]
    assert all(c.tolist() == [0, 0, 0] for c in A.pc_ref(*A.pc_maps(1000, 3, 5), 7).reshape(-1, 3))


@pytest.mark.parametrize("Na,Nb", [(3, 5), (5, 3)])
def test_pair_counts_indexed_with_the_wrong_extent_fail(Na, Nb):
    a, b = A.pc_maps(257, Na, Nb)
    assert not np.array_equal(A.pc_ref(a, b, 1, stride=Na), A.pc_ref(a, b, 1))
    a, b = A.pc_maps(257, 1, 1)
    assert np.array_equal(A.pc_ref(a, b, 1, stride=1), A.pc_ref(a, b, 1))


def test_ncc_map_gate_table_is_what_numpy_float32_measures():
    ids = [A.nm_id(*nmk, hw) for nmk in A.NM_NMK for hw in A.NM_HW]
    assert set(A.NM_F32) == set(ids) and len(ids) == len(A.NM_F32)
    for nmk in A.NM_NMK:
        for hw in A.NM_HW:
            got, want = A.nm_f32_error(*nmk, hw), A.NM_F32[A.nm_id(*nmk, hw)]
            assert got == pytest.approx(want, rel=1e-2), A.nm_id(*nmk, hw)
            assert all(0 < v < 5e-7 for v in want)            # 4 x each stays far below one dropped term (>= 1e-3 of these maps)


def test_one_pixel_ncc_map_cases_take_the_first_draw_with_a_representative_float32_distance(monkeypatch):
    assert set(A.NM_DRAW) == {(N, M, K, 1) for N, M, K in A.NM_NMK if N > 1}
    for key, draw in A.NM_DRAW.items():
        assert min(A.NM_F32[A.nm_id(*key)]) >= A.NM_DRAW_FLOOR
        for d in range(draw):
            monkeypatch.setitem(A.NM_DRAW, key, d)
            assert min(A.nm_f32_error(*key)) < A.NM_DRAW_FLOOR, (key, d)
        monkeypatch.setitem(A.NM_DRAW, key, draw)


def test_ncc_map_cases_hold_exact_zeros_ones_and_an_empty_mask():
    for N, M, K in A.NM_NMK:
        for HW in A.NM_HW:
            soft, gt = A.nm_operands(N, M, K, HW)
            assert (soft == 0).any() or K == 1 and HW == 1
            assert (soft == 1).any()
            assert np.array_equal(gt.sum(1), np.ones((M, HW), np.float32))
            if M > 1:
                assert (gt[M - 1, 0] == 1).all()
            ess, esy = A.nm_ref(soft, gt)
            assert np.isfinite(ess).all() and np.isfinite(esy).all()
            if K > 1 and HW > 1:
                assert esy[0].max() > 18.0 / N                 # -log(0 + 1e-8) = 18.42: the eps decides a value


@pytest.mark.parametrize("HW", [1, 255, 257, 1000])
def test_ncc_maps_without_their_tail_fail(HW):
    N, M, K = 6, 4, 2
    soft, gt = A.nm_operands(N, M, K, HW)
    good, bad = A.nm_ref(soft, gt), A.nm_ref(soft, gt, tail=False)
    gate = A.NM_F32[A.nm_id(N, M, K, HW)]
    assert A.rel_err(bad[0], good[0]) > 4 * gate[0] and A.rel_err(bad[1], good[1]) > 4 * gate[1]
    soft, gt = A.nm_operands(N, M, K, 256)
    assert A.rel_err(A.nm_ref(soft, gt, tail=False)[0], A.nm_ref(soft, gt)[0]) == 0


def test_ncc_cases_reach_the_offsets_they_claim():
    worst = 0.0
    for M in A.NCC_M:
        for HW in A.NCC_HW[1:]:
            a, v = A.ncc_operands(M, HW)
            ref = A.ncc_ref(a, v)
            assert np.isfinite(ref).all() and (np.abs(ref) <= 1 + 1e-12).all()
            worst = max([worst, abs(a.mean()) / a.std()] + [abs(x.mean()) / x.std() for x in v])
            # the one-pass fp64 form the kernel evaluates stays within the gate of the two-pass reference
            x = a.astype(np.float64)
            for j, y in enumerate(v.astype(np.float64)):
                one = (np.mean(x * y) - x.mean() * y.mean()) / np.sqrt((np.mean(x * x) - x.mean() ** 2) * (np.mean(y * y) - y.mean() ** 2))
                assert abs(one - ref[j]) < 1e-8
    assert 900 < worst < 1200
    assert np.isnan(A.ncc_ref(*A.ncc_operands(4, 1))).all()


def test_end_to_end_case_has_an_empty_mask_and_three_labels():
    from oracle import metrics as OM
    s, g, soft = A.e2e_operands()
    assert s.shape[1:] == (24, 20) and not g[2].any() and set(np.unique(g)) == {0, 1, 2} and not (s[3] == 2).any()
    assert np.isfinite(OM.generalised_energy_distance(s, g, nlabels=3, label_range=range(3)))
    assert OM.per_label_dice(s[3], g[2], 3)[2] == 1.0 and OM.per_label_dice(s[0], g[2], 3)[1] == 0.0


# ------------------------------------------------------------------------------------------------ batch assembly
@pytest.fixture(scope="module")
def aug():
    """Datasets and the two twins of every case, computed once."""
    out = {}
    for c in A.AUG_CASES:
        X, Y = A.aug_dataset(c)
        out[c.name] = (X, Y, A.aug_ref(c, X=X, Y=Y), A.aug_ref(c, np.float32, X=X, Y=Y))
    return out


def test_the_float32_default_of_the_twin_is_the_arithmetic_it_was(aug):
    """float32 in, float32 out, every intermediate float32; and the un-resampled rows are the plain gather."""
    from oracle import augment as OA
    c = A.AUG_CASES[2]
    X, Y = aug[c.name][:2]
    for b, row in enumerate(c.rows):
        img, lbl = OA.augment(X[c.idx[b]], Y[c.idx[b], ..., c.ann[b]], np.asarray(row, np.float32), c.nlabels)
        assert img.dtype == np.float32 and np.array_equal(img, aug[c.name][3][0][b]) and np.array_equal(lbl, aug[c.name][3][1][b])
    plain = OA.augment(X[5], Y[5, ..., 1], np.asarray(c.rows[0], np.float32), c.nlabels)
    assert np.array_equal(plain[0], X[5]) and np.array_equal(plain[1], Y[5, ..., 1])
    assert OA._bilinear_zero(X[0], np.full((2, 2), 3.25, np.float32), np.full((2, 2), 1.5, np.float32)).dtype == np.float32


@pytest.mark.parametrize("case", A.AUG_CASES, ids=lambda c: c.name)
def test_parameter_rows_stay_inside_the_image(case):
    assert 6 <= A.AUG_ROWS <= 8 and len(case.rows) <= 8 and len(case.idx) >= len(case.rows)
    idx = case.idx[:len(case.rows)]
    assert len(set(idx)) == len(idx) - 1 and list(idx) != sorted(idx) and max(idx) < A.AUG_ROWS
    assert all(0 <= a < case.A for a in case.ann) and (case.A == 1 or any(a != 0 for a in case.ann))
    for do_rot, c, s, do_scale, px, py, r, flips in case.rows:
        assert abs(c * c + s * s - 1) < 1e-6 and flips in (0, 1, 2, 3)
        if do_scale:
            assert r >= 1 and px + r <= case.W and py + r <= case.H


def test_the_cases_cover_every_branch():
    rows = [(c, r) for c in A.AUG_CASES for r in c.rows]
    for rot in (0, 1):
        for sc in (0, 1):
            assert any(r[0] == rot and r[3] == sc for _, r in rows)
    assert {r[7] for _, r in rows if not r[0] and not r[3]} == {0, 1, 2, 3}
    assert {c.nlabels for c in A.AUG_CASES} == {1, 2, 3, 8} and {c.A for c in A.AUG_CASES} == {1, 4}
    assert {(c.H, c.W) for c in A.AUG_CASES} == {(128, 128), (136, 160), (160, 136), (5, 7), (1, 300)}
    assert any(c.H * c.W > 64 * 256 and c.H * c.W % (64 * 256) for c in A.AUG_CASES)      # a second, partial trip of the grid-stride loop
    sq = [r for c, r in rows if c.H == c.W == 128]
    assert any(r[0] and (r[1], r[2]) == (1.0, 0.0) for r in sq) and any(r[0] and (r[1], r[2]) == (0.0, 1.0) for r in sq)
    assert any(r[0] and r[2] > 0.1 for r in sq) and any(r[0] and r[2] < -0.1 for r in sq)
    assert any(r[3] and r[6] == 128 for r in sq) and any(r[3] and r[6] == 1 for r in sq)
    assert any(r[3] and r[6] == 98 and r[4] == 0 for r in sq) and any(r[3] and r[6] == 98 and r[4] == 30 and r[5] == 30 for r in sq)


@pytest.mark.parametrize("case", A.AUG_CASES, ids=lambda c: c.name)
def test_margin_cap_exact_rows_and_gate_table(case, aug):
    X, Y, (img64, lbl64, margin), (img32, lbl32) = aug[case.name]
    exact = np.array([A.aug_row_exact(case, r) for r in case.rows])
    for b in np.nonzero(exact)[0]:                            # exact by construction: the two precisions agree bit for bit
        assert np.array_equal(img32[b].astype(np.float64), img64[b]) and np.array_equal(lbl32[b], lbl64[b]), b
    low = (margin[~exact] < A.AUG_MARGIN)
    assert low.sum() <= A.AUG_MARGIN_CAP * margin.size, (case.name, int(low.sum()))
    if (~exact).any():                                         # the fp32 twin itself obeys the label rule
        assert not ((lbl32[~exact] != lbl64[~exact]) & ~low).any()
    assert A.aug_f32_error(case) == pytest.approx(A.AUG_F32[case.name], rel=1e-2, abs=0)
    if case.nlabels >= 3 and case.H >= 128:
        # three labels inside one 2 x 2 tap window: the runner-up and the first-maximum rule are about real pixels
        m = Y[..., 0].astype(np.int64)
        win = np.sort(np.stack([m[:, :-1, :-1], m[:, 1:, :-1], m[:, :-1, 1:], m[:, 1:, 1:]], -1), -1)
        assert ((np.diff(win, axis=-1) != 0).sum(-1) >= 2).any()


def _aug_fails(case, aug, defect):
    """Does the twin with `defect` leave the gates of the GPU tier on this case?  (image gate, labels above the margin, exact rows)"""
    X, Y, (img64, lbl64, margin), _ = aug[case.name]
    bad = A.aug_ref(case, defects=(defect,), X=X, Y=Y)
    exact = np.array([A.aug_row_exact(case, r) for r in case.rows])
    if exact.any() and (not np.array_equal(bad[0][exact], img64[exact]) or not np.array_equal(bad[1][exact], lbl64[exact])):
        return True
    if (~exact).any():
        if A.rel_err(bad[0][~exact], img64[~exact]) > min(4 * A.AUG_F32[case.name], A.AUG_IMAGE_FLOOR):
            return True
        return bool(((bad[1][~exact] != lbl64[~exact]) & (margin[~exact] >= A.AUG_MARGIN)).any())
    return False


@pytest.mark.parametrize("defect,failing,blind", [
    ("centre", ["136x160", "160x136", "5x7", "1x300"], ["sq128-resample"]),          # H = W cannot see a swapped centre
    ("scale", ["136x160", "160x136", "5x7"], ["sq128-resample"]),
    ("flips", ["sq128-exact", "136x160", "5x7", "1x300"], []),
    ("annotator", ["sq128-exact", "sq128-resample", "136x160", "5x7"], ["160x136"]),   # A = 1 has no offset to ignore
    ("argmax", ["sq128-exact", "sq128-resample", "136x160"], ["sq128-one-label"]),
])
def test_a_wrong_augmentation_twin_fails_a_case(defect, failing, blind, aug):
    by_name = {c.name: c for c in A.AUG_CASES}
    for name in failing:
        assert _aug_fails(by_name[name], aug, defect), (defect, name)
    for name in blind:
        assert not _aug_fails(by_name[name], aug, defect), (defect, name)


# ------------------------------------------------------------------------------------------------ posterior input
def test_posterior_input_cases_sit_at_the_workgroup_edges():
    assert [h * w for h, w in A.PI_HW] == [1, 255, 256, 1023, 1024, 1025, 4097]
    for (H, W) in A.PI_HW:
        for in_ch, nl in A.PI_CH:
            patch, mask, ref = A.pi_operands(H, W, in_ch, nl)
            assert ref.shape == (A.PI_N, in_ch + nl, H, W) and (mask == nl).any() and (mask < 0).any()
            assert set(np.unique(ref[:, in_ch:])) <= {-0.5, 0.5}
            outside = (mask < 0) | (mask >= nl)
            assert (ref[:, in_ch:].transpose(0, 2, 3, 1)[outside] == -0.5).all()
