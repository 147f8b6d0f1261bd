"""PHISeg3D on volumes with three unequal extents, without a device: the plans of every case of tests/_aniso3d.py carry one level
of the volume's pyramid in every op, the three wide orientations reach the kernel mixes the table claims, a run with the volume's
axes confused differs from the right one by far more than any gate, and the CPU oracle's fp32 run of every case sits inside the
gates the GPU tier (tests/test_aniso3d_gpu.py) holds the kernels to - so a case that fails there fails because of the kernels."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi, _ops
from oracle import refgraph3d as R3
from tests import _aniso3d as A
from tests import _bn_routes as BR
from tests import _vol_routes as VR


@pytest.fixture(scope="module")
def plans():
    """name -> the training plan of the case under the default arithmetic policy, built once (device="cpu": structure only)."""
    built = {}

    def get(name):
        if name not in built:
            L = _ffi.lib()
            L.uz_set_conv_math(1)
            try:
                built[name] = A.plan(A.BY_NAME[name])
            finally:
                L.uz_set_conv_math(-1)
        return built[name]
    return get


def _triple(o):
    s = _ops.SCHEMA[o["code"]]
    return (o.i("D") if "D" in s.ix else o.i("N"), o.i("H"), o.i("W"))


# ------------------------------------------------------------------------------------------ 1. the table
def test_the_table_holds_what_the_tiers_rely_on():
    assert len(set(A.IDS)) == len(A.CASES) == 9
    for c in A.CASES:
        R = A.levels_of(c)
        assert all(n % (1 << (R - 1)) == 0 for n in c.dhw) and c.latent_levels <= R, c.name
        pyr = A.pyramid(c)
        assert len(pyr) == R
        for d, h, w in pyr:                                                           # three different extents at every level: any swap of two
            assert len({d, h, w}) == 3, (c.name, (d, h, w))                           # axes is off the pyramid ...
        mixed = {(a[0], b[1], e[2]) for a in pyr for b in pyr for e in pyr} - set(pyr)
        assert len(mixed) == R ** 3 - R, c.name                                       # ... and so is every triple of mixed levels
    d, h, w = A.BY_NAME[A.NARROW_L3[0]].dhw
    assert [A.BY_NAME[n].dhw for n in A.NARROW_L3] == [(d, h, w), (w, d, h), (h, w, d)]          # cyclic permutations
    assert all(A.BY_NAME[n].filters == A.NARROW3 and A.BY_NAME[n].latent_levels == 3 and not A.BY_NAME[n].reversible for n in A.NARROW_L3)
    wide = [A.BY_NAME[n].dhw for n in A.WIDE]
    assert len(set(wide)) == 3 and all(sorted(s) == [16, 32, 80] for s in wide)
    assert all(np.prod(s) > 32768 for s in wide)                                      # the large BatchNorm path at level 0
    assert set(A.VALIDATION) <= set(A.IDS) and set(A.REPLAY) <= set(A.IDS) and A.PREDICT in A.NARROW_L3
    assert [c.reversible for c in A.CASES].count(True) == 1
    deep = {c.name: min(A.pyramid(c)) for c in A.CASES}
    assert deep["narrow-4x24x40"][0] == 1 and deep["narrow-r4-8x16x24"] == (1, 2, 3) and deep["narrow-8x12x20"] == (2, 3, 5)


# ------------------------------------------------------------------------------------------ 2. every op, one level
@pytest.mark.parametrize("name", A.IDS)
def test_every_op_carries_one_level_of_the_volumes_pyramid(name, plans):
    """Every op whose schema has H and W slots and a D or an N slot holds (D0 >> l, H0 >> l, W0 >> l) for ONE level l - two axes
    exchanged, or extents of different levels, are no level of a pyramid whose extents all differ.  The named exceptions: the
    depth stage of the trilinear interpolation carries the in-plane-upsampled input of level l, (D0 >> (l + 1), H0 >> l, W0 >> l),
    as Plan.trilinear emits it, and the nearest resize carries its level with the factors that take each axis to the full volume."""
    c = A.BY_NAME[name]
    D0, H0, W0 = c.dhw
    pyr, R = A.pyramid(c), A.levels_of(c)
    seen, checked, lerps, nearest = set(), 0, 0, 0
    for o in A.tapes(plans(name)):
        s = _ops.SCHEMA[o["code"]]
        if "H" not in s.ix or "W" not in s.ix or not ("D" in s.ix or "N" in s.ix):
            continue
        d, h, w = _triple(o)
        if o["code"] in ("UZ_OP_DEPTH_LERP_FWD", "UZ_OP_DEPTH_LERP_BWD"):
            lvl = pyr.get((2 * d, h, w))
            assert lvl is not None and lvl < R - 1, (o["code"], (d, h, w), sorted(pyr))
            lerps += 1
        else:
            assert (d, h, w) in pyr, (o["code"], (d, h, w), sorted(pyr))
            lvl = pyr[(d, h, w)]
            if o["code"] in ("UZ_OP_NEAREST3D_FWD", "UZ_OP_NEAREST3D_BWD"):
                f, fz = o.i("factor", "factor_z")
                assert f == H0 // h and f == W0 // w and fz == D0 // d and f > 1, (o["code"], (d, h, w), f, fz)
                nearest += 1
        seen.add(lvl)
        checked += 1
    # 350 - 450 ops in a training plan (the reversible one: 956), 250 - 320 of them with such slots (632)
    assert checked >= 250 and len(A.tapes(plans(name))) >= 350 and seen == set(range(R)), (checked, seen)
    assert lerps >= 2 * (c.latent_levels - 1) and nearest == 2 * (c.latent_levels - 1), (lerps, nearest)


@pytest.mark.parametrize("name", A.IDS)
def test_the_ce_terms_are_scaled_by_the_depth(name, plans):
    """The CE kernel averages over its batch axis - the D slices of the one sample: the loss tape scales the L terms, and the
    backward tape their seed, by D (not H, not W) to give the sum over voxels the reference computes."""
    c = A.BY_NAME[name]
    p = plans(name)
    scales = [(o["n"], o["f"][0]) for ops in (p.loss_ops, p.bwd_ops) for o in ops if o["code"] == "UZ_OP_SCALE"]
    assert scales == [(c.latent_levels, float(c.dhw[0])), (1, float(c.dhw[0]))], (name, scales)


# ------------------------------------------------------------------------------------------ 3. noise shapes, level tables
@pytest.mark.parametrize("name", A.IDS)
def test_the_noise_buffers_have_the_oracles_shapes(name, plans):
    c = A.BY_NAME[name]
    D, H, W = c.dhw
    R, L = A.levels_of(c), c.latent_levels
    want = R3.phiseg3d_eps_shapes(D, H, W, R, L)
    got = [(1, v.C, v.N, v.H, v.W) for v in plans(name).io["eps"]]
    assert got == want + want == [tuple(s) for s in A.eps_shapes(c)]
    assert want[0] == (1, 2, D >> (R - 1), H >> (R - 1), W >> (R - 1)) and want[-1] == (1, 2, D >> (R - L), H >> (R - L), W >> (R - L))
    assert [tuple(e.shape) for e in A.operands(c)[3]] == want + want


@pytest.mark.parametrize("name", [c.name for c in A.CASES if c.filters[0] == 4 and not c.reversible])      # predict() is not built for the reversible variant
def test_the_level_tables_of_a_draw_plan_hold_both_factors(name):
    """The tables uz_vol_sample_accum reads: per level the pointer's channel count, f = H0 // h_l = W0 // w_l and fz = D0 // d_l, from
    levels of the volume's pyramid.  On a pyramid of powers of two f and fz are the same number at every level, so this test cannot
    tell one from the other; what it pins is that each comes out as 2^l from a level whose three extents are the volume's.  The two
    factors of the nearest resize are told apart by test_every_op_carries_one_level_of_the_volumes_pyramid."""
    c = A.BY_NAME[name]
    D, H, W = c.dhw
    m = A.net(c, device="cpu")
    m.eval()
    draw = m._build_predict(D, H, W, "draw")
    tb = m._level_tables(draw, D, H, W)
    lv = draw.io["s_in"]
    diff = A.levels_of(c) - c.latent_levels
    assert [(v.N, v.H, v.W) for v in lv] == [(D >> l, H >> l, W >> l) for l in range(c.latent_levels)]
    assert list(tb["f"]) == [H // v.H for v in lv] == [W // v.W for v in lv] == [1 << l for l in range(c.latent_levels)]
    assert list(tb["fz"]) == [D // v.N for v in lv] == list(tb["f"]) and list(tb["ctot"]) == [v.Ctot for v in lv]
    assert draw.io["s"] is None and not any(o["code"] == "UZ_OP_NEAREST3D_FWD" for o in draw.fwd_ops)
    assert diff >= 0 and [v.C for v in lv] == [A.K] * c.latent_levels


# ------------------------------------------------------------------------------------------ 4. routes
# (direction 0 fwd / 1 dgrad / 2 wgrad, plane (D, H, W)) -> floor on the number of split-route 3 x 3 convolutions; the keys are exact
SPLIT_ROUTES = {
    "wide-16x32x80": {(0, (16, 32, 80)): 14, (1, (16, 32, 80)): 13},                  # no split weight gradient: W % 32 != 0
    "wide-16x80x32": {(0, (16, 80, 32)): 13, (1, (16, 80, 32)): 13, (2, (16, 80, 32)): 6,
                      (0, (8, 40, 16)): 15, (1, (8, 40, 16)): 13, (2, (8, 40, 16)): 15},
    "wide-80x16x32": {(0, (80, 16, 32)): 13, (1, (80, 16, 32)): 13, (2, (80, 16, 32)): 6},
}
FP32_ROUTE_FLOOR = {"wide-16x32x80": 115, "wide-16x80x32": 67, "wide-80x16x32": 110}


def _conv_routes(p):
    """(Counter of (direction, plane) over the split-route 3 x 3 convolutions, number of fp32-route 3 x 3 convolutions) of a plan."""
    L = _ffi.lib()
    split, f32 = collections.Counter(), 0
    for o in A.tapes(p):
        if o["code"] in _ops.CONV_KIND and o.i("ks") == 3:
            kind, cin, cout, N, H, W, ks = _ops.conv_dims(o)
            r = L.uz_conv_route(kind, cin, cout, N, H, W, ks)
            if r == 1:
                split[(kind, (N, H, W))] += 1
            else:
                assert r == 0, (o["code"], r)
                f32 += 1
    return split, f32


@pytest.mark.parametrize("name", A.IDS)
def test_conv_routes_of_the_three_orientations(name, plans):
    """Under the default policy (uz_set_conv_math(1)): the wide cases take the split-fp16 route on exactly the planes and in the
    directions of SPLIT_ROUTES - three orientations, three mixes -, the narrow cases nowhere."""
    L = _ffi.lib()
    p = plans(name)
    L.uz_set_conv_math(1)
    try:
        assert L.uz_get_conv_math() == 1
        split, f32 = _conv_routes(p)
    finally:
        L.uz_set_conv_math(-1)
    print(f"{name}: split-route 3x3 convolutions {dict(split)}, fp32-route {f32}")
    if name in A.WIDE:
        want = SPLIT_ROUTES[name]
        assert set(split) == set(want), (name, dict(split))
        assert all(split[k] >= n for k, n in want.items()), (name, dict(split))
        assert f32 >= FP32_ROUTE_FLOOR[name], (name, f32)
        assert len({o["lane"] for o in p.fwd_ops}) > 1 and len({o["lane"] for o in p.bwd_ops}) > 1
    else:
        assert not split and f32 > 50, (name, dict(split), f32)


def test_the_three_wide_orientations_are_three_mixes_of_kernels():
    keys = [frozenset((k, tuple(sorted(plane))) for k, plane in SPLIT_ROUTES[n]) for n in A.WIDE]
    assert all(set(plane) <= {8, 16, 32, 40, 80} for n in A.WIDE for _, plane in SPLIT_ROUTES[n])
    assert len({frozenset(SPLIT_ROUTES[n]) for n in A.WIDE}) == 3 and keys[0] != keys[1] and keys[1] != keys[2]


@pytest.mark.parametrize("name", A.WIDE)
def test_wide_level0_batchnorms_take_the_large_path(name, plans):
    """uz_bn_route on every BatchNorm op of the plan: level 0 (40 960 values per channel) answers the large path in both directions,
    the deeper levels (5 120 and 640) the mid and the small path."""
    L = _ffi.lib()
    c = A.BY_NAME[name]
    pyr = A.pyramid(c)
    got = collections.defaultdict(set)
    for o in A.tapes(plans(name)):
        if o["code"] not in ("UZ_OP_BN_RELU_FWD", "UZ_OP_BN_RELU_BWD"):
            continue
        Cc, N, H, W = o.i("C", "N", "H", "W")
        out = (ctypes.c_int * 6)()
        direction = int(o["code"].endswith("BWD"))
        assert L.uz_bn_route(direction, N, Cc, H, W, 1, 1, 0, out) == 0
        got[(pyr[(N, H, W)], direction)].add(out[0])
    assert got[(0, 0)] == got[(0, 1)] == {BR.LARGE}, dict(got)
    assert got[(1, 0)] == got[(1, 1)] == {BR.MID} and got[(2, 0)] == got[(2, 1)] == {BR.SMALL}, dict(got)


@pytest.mark.parametrize("name", A.NARROW_L3)
def test_narrow_volumes_take_the_scalar_pooling_kernels_below_level_0(name, plans):
    """uz_vol_route on every pooling and depth-interpolation op of the plan, with the alignment of the views as the plan lays them
    out.  AvgPool3d: W % 4 == 0 at level 0 (20, 12, 8) - the float4 kernels -, W % 4 != 0 below it (10, 6, 4 -> the 12 x 20 x 8 case
    keeps W = 4 and stays on float4 there) - the scalar kernels.  Nearest backward from level 2: 64 children, one wave per element.
    The depth stage's predicate is H W % 4 == 0, which every plane it writes in these cases meets (60, 24, 40 at level 1): it stays
    on the float4 kernels; its scalar form is pinned at kernel level (tests/_vol_routes.py)."""
    L = _ffi.lib()
    c = A.BY_NAME[name]
    p = plans(name)
    pyr = A.pyramid(c)
    got = collections.defaultdict(set)

    def align(v):
        a = p._resolve(v)
        return 16 if a % 16 == 0 else 8 if a % 8 == 0 else 4
    codes = {"UZ_OP_AVGPOOL3D_FWD": 0, "UZ_OP_AVGPOOL3D_BWD": 1, "UZ_OP_DEPTH_LERP_FWD": 2, "UZ_OP_DEPTH_LERP_BWD": 3, "UZ_OP_NEAREST3D_BWD": 5}
    for o in A.tapes(p):
        if o["code"] not in codes:
            continue
        op = codes[o["code"]]
        Cc, D, H, W = o.i("C", "D", "H", "W")
        f, fz = (o.i("factor", "factor_z") if op == 5 else (1, 1))
        src, dst = o["p"][0], o["p"][1]
        kernel, _ = VR.query(L, op, Cc, D, H, W, f, fz, align(src), align(dst))
        lvl = pyr[(2 * D, H, W)] if op in (2, 3) else pyr[(D, H, W)]
        got[(op // 2, lvl)].add((W % 4 == 0, kernel))
    W0 = c.dhw[2]
    assert got[(0, 0)] == {(True, VR.VEC)}, dict(got)                                  # level-0 pooling, forward and backward
    assert got[(0, 1)] == ({(False, VR.SCALAR)} if (W0 // 2) % 4 else {(True, VR.VEC)}), dict(got)
    assert (0, 2) not in got and {k for _, k in got[(1, 0)] | got[(1, 1)]} == {VR.VEC}, dict(got)
    assert {k for _, k in got[(2, 1)]} == {VR.SCALAR} and {k for _, k in got[(2, 2)]} == {VR.WAVE}, dict(got)
    assert sum(1 for n in A.NARROW_L3 if (A.BY_NAME[n].dhw[2] // 2) % 4) == 2          # two of the three reach the scalar pooling kernels


# ------------------------------------------------------------------------------------------ 5. the cases discriminate
TRANSPOSITIONS = ((1, 0, 2), (2, 1, 0), (0, 2, 1))


@pytest.mark.parametrize("name", A.NARROW)
def test_a_confused_geometry_is_far_from_the_case(name):
    """The fp64 oracle on the same weights with two axes of the volume, its labels and its noise exchanged - each of the three
    transpositions -, with the nearest resize's factors taken from the wrong axes, and with the CE terms scaled by H instead of D:
    each is off the case's own run by more than 100 LOSS_REL in the loss and, where the shapes agree after permuting back, by more
    than 100 FWD_CAP in some level's logits.  (The weights are not permuted: a 3 x 3 x 3 kernel is not symmetric.)"""
    c = A.BY_NAME[name]
    r64 = A.oracle_run(c, torch.float64)
    for axes in TRANSPOSITIONS:
        v = A.variant_run(c, ("perm", axes))
        d_loss = abs(v.loss - r64.loss) / abs(r64.loss)
        d_fwd = max(A.maxabs(A.unpermuted(v.fwd[f"s_in{l}"], axes), r64.fwd[f"s_in{l}"]) for l in range(c.latent_levels))
        print(f"{name} axes {axes}: loss off by {d_loss:.1e}, level logits by {d_fwd:.1e}")
        assert d_loss > 100 * A.LOSS_REL and d_fwd > 100 * A.FWD_CAP, (name, axes, d_loss, d_fwd)
    v = A.variant_run(c, "nearest")
    d_loss = abs(v.loss - r64.loss) / abs(r64.loss)
    d_fwd = max(A.maxabs(v.fwd[f"s{l}"], r64.fwd[f"s{l}"]) for l in range(c.latent_levels))
    print(f"{name} nearest factors exchanged: loss off by {d_loss:.1e}, resized logits by {d_fwd:.1e}")
    assert d_loss > 100 * A.LOSS_REL and d_fwd > 100 * A.FWD_CAP, (name, d_loss, d_fwd)
    assert all(A.maxabs(v.fwd[f"s_in{l}"], r64.fwd[f"s_in{l}"]) == 0 for l in range(c.latent_levels))
    v = A.variant_run(c, "ce")
    d_loss = abs(v.loss - r64.loss) / abs(r64.loss)
    worst = max(abs(v.terms[k] - r64.terms[k]) / abs(r64.terms[k]) for k in r64.terms if k.startswith("residual"))
    print(f"{name} CE scaled by H: loss off by {d_loss:.1e}, a CE term by {worst:.1e}")
    assert d_loss > 100 * A.LOSS_REL and worst > 100 * A.LOSS_REL, (name, d_loss, worst)


# ------------------------------------------------------------------------------------------ 6. the yardstick meets its own gates
@pytest.mark.parametrize("name", A.IDS)
def test_reference_margin(name):
    """The fp32 oracle against the fp64 oracle on the case's inputs: loss and every term within LOSS_REL, every forward tensor within
    FWD_CAP, the same set of parameters without a gradient, the buffers within RM_TOL / RV_REL; and the second fp32 evaluation on
    the CPU (oneDNN off) passes the three gradient gates against the default backend - the robustness the weight seeds of the table
    were chosen for; for the narrow cases the default backend passes them against the second evaluation too.  The wide cases hold
    ReLU inputs within 1e-6 of zero, so their two fp32 evaluations depend on the host's CPU model (tests/_aniso3d.py, RESEEDED):
    their seeds pass on the two models tried, and on a third this check can turn red for a wide case with no change in the code -
    the remedy is the next seed of the scan in DESIGN.md section 5, never a gate.  Prints the reference's own distances."""
    c = A.BY_NAME[name]
    r32, r64 = A.oracle_run(c, torch.float32), A.oracle_run(c, torch.float64)
    rel = abs(r32.loss - r64.loss) / abs(r64.loss)
    fwd = {k: A.maxabs(r32.fwd[k], r64.fwd[k]) for k in r64.fwd}
    keys = A.grad_keys(r64)
    rc = A.grad_ratios(lambda k: r32.grads[k], r64, keys)
    alt = A.second_fp32_run(c)
    ra = A.grad_ratios(lambda k: alt.grads[k], r64, keys)
    print(f"{name}: fp32 oracle vs fp64 oracle: loss rel {rel:.1e}, forward max {max(fwd.values()):.1e} at {max(fwd, key=fwd.get)}, gradients "
          f"median {np.median(rc):.1e} p90 {np.percentile(rc, 90):.1e} max {rc.max():.1e} over {len(keys)} tensors; second fp32 evaluation: "
          f"median {np.median(ra):.1e} p90 {np.percentile(ra, 90):.1e} max {ra.max():.1e}")
    assert np.isfinite(r64.loss) and rel <= A.LOSS_REL, (name, rel)
    assert list(r64.terms) == A.term_names(c.latent_levels)
    for k, v in r64.terms.items():
        assert abs(r32.terms[k] - v) <= A.LOSS_REL * abs(v), (name, k, r32.terms[k], v)
    assert max(fwd.values()) <= A.FWD_CAP, (name, fwd)
    D, H, W = c.dhw
    for l in range(c.latent_levels):
        assert tuple(r64.fwd[f"s{l}"].shape) == (1, A.K, D, H, W) and tuple(r64.fwd[f"s_in{l}"].shape) == (1, A.K, D >> l, H >> l, W >> l)
        assert torch.equal(r64.fwd[f"s{l}"], A.nearest_full(r64.fwd[f"s_in{l}"], c.dhw))
    assert r32.none_grads == r64.none_grads and len(keys) > 10
    assert all(float(r64.grads[k].abs().max()) > 0 for k in keys), name                # r = err / max |g64| is defined for every tensor
    print(f"{name}: gates the second evaluation misses against the first: {[f[0] for f in A.gradient_gates(ra, rc, keys)]}, the first against it: "
          f"{[f[0] for f in A.gradient_gates(rc, ra, keys)]}")
    assert not A.gradient_gates(ra, rc, keys), (name, A.gradient_gates(ra, rc, keys))
    if name in A.NARROW:
        assert not A.gradient_gates(rc, ra, keys), (name, A.gradient_gates(rc, ra, keys))
    b32, b64 = A.expected_buffers(c, r32), A.expected_buffers(c, r64)
    for k, v in b64.items():
        if k.endswith("running_mean"):
            assert A.maxabs(b32[k], v) <= A.RM_TOL, k
        elif k.endswith("running_var"):
            assert float(((b32[k].double() - v.double()).abs() / v.double().abs()).max()) <= A.RV_REL, k
        else:
            assert torch.equal(b32[k], v), k


@pytest.mark.parametrize("name", A.IDS)
def test_small_plane_relus_keep_their_distance_from_the_kink(name):
    """Where it can be had - the narrow cases - the weight seed keeps every ReLU input on a plane of at most 1 024 voxels at least
    KINK_MARGIN from zero in the fp64 oracle; for the wide cases the figure is printed only."""
    c = A.BY_NAME[name]
    margin = A.relu_kink_margin(c)
    print(f"{name}: smallest |ReLU input| on planes of at most 1024 voxels, fp64 oracle: {margin:.1e}")
    assert 0 < margin < 1.0
    if name in A.NARROW:
        assert margin >= A.KINK_MARGIN, (name, margin)


@pytest.mark.parametrize("name", A.VALIDATION)
def test_validation_reference_margin(name):
    """The eval-mode forward of the oracle from the off-identity state: fp32 within FWD_CAP of fp64, and the running statistics do
    matter - the same forward from the identity state is far from it."""
    c = A.validation_case(name)
    r32, r64 = A.oracle_run(c, torch.float32, train=False), A.oracle_run(c, torch.float64, train=False)
    e = max(A.maxabs(r32.fwd[k], r64.fwd[k]) for k in r64.fwd)
    plain = A.oracle_run(A.BY_NAME[name], torch.float64, train=False)
    off = max(A.maxabs(plain.fwd[f"s_in{l}"], r64.fwd[f"s_in{l}"]) for l in range(c.latent_levels))
    print(f"{name}: eval-mode fp32 oracle within {e:.1e} of fp64; identity statistics move the level logits by {off:.1e}")
    assert e <= A.FWD_CAP and off > 100 * A.FWD_CAP


def test_the_oracle_decides_the_labels_of_the_predict_case():
    m = A.predict_case()
    c = m.case
    D, H, W = c.dhw
    assert m.r64.acc.shape == (m.S, A.K, D, H, W) and [tuple(e.shape) for e in m.eps] == [(m.S, *s[1:]) for s in A.eps_shapes(c)[:c.latent_levels]]
    counts = np.bincount(m.r64.labels.reshape(-1).numpy(), minlength=A.K)
    print(f"predict {c.name}: {m.unsure_fraction:.1e} of the voxels within {A.MARGIN} of a tie, labels {counts.tolist()}")
    assert m.unsure_fraction <= A.MARGIN_FRACTION and sorted(counts)[1] >= 0.1 * counts.sum(), (m.unsure_fraction, counts)
    assert torch.equal(m.r32.labels[m.sure], m.r64.labels[m.sure])
    assert all(not torch.equal(m.r64.acc[s], m.r64.acc[0]) for s in range(1, m.S))    # the samples differ
    for s in range(m.S):
        for l in range(c.latent_levels):
            assert A.maxabs(m.r32.s_in[s][l], m.r64.s_in[s][l]) <= A.FWD_CAP
    assert A.maxabs(m.r32.mean_soft, m.r64.mean_soft) <= 1e-5
