"""The 2-D models on images with H != W, without a device: the plans of every case of tests/_nonsquare.py carry a plane of the
image's pyramid in every op, the two wide PHISeg cases reach the split-fp16 route and every optional kernel form on non-square
planes (and are not each other's mirror), and the CPU oracle's fp32 run of every case sits inside the caps the GPU tier
(tests/test_nonsquare_gpu.py) holds the kernels to - so a case that fails there fails because of the kernels."""
import collections

import numpy as np
import pytest
import torch

import oracle
import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi, _ops
from tests import _nonsquare as NS

OPTIONAL_FORMS = ("x_packed", "x_seg2_c0", "a_packed", "y_packed", "dy_packed", "slabs_only", "nslab", "fold", "dbias_rows")


@pytest.fixture(scope="module")
def plans():
    """name -> the training plan of the case, built once (device="cpu": structure only)."""
    built = {}

    def get(name):
        if name not in built:
            built[name] = NS.plan(NS.BY_NAME[name])
        return built[name]
    return get


def _routes(p, only_nonsquare):
    """Counter of (direction, uz_conv_route's answer) over the 3 x 3 convolutions of a plan."""
    L = _ffi.lib()
    got = collections.Counter()
    for o in NS.tapes(p):
        if o["code"] in _ops.CONV_KIND and o.i("ks") == 3:
            kind, cin, cout, N, H, W, ks = _ops.conv_dims(o)
            if H != W or not only_nonsquare:
                got[(kind, L.uz_conv_route(kind, cin, cout, N, H, W, ks))] += 1
    return got


def _forms(p, only_nonsquare=False):
    """Counter of the optional-form slots (the schema's `opts`) that some op of the plan sets."""
    got = collections.Counter()
    for o in NS.tapes(p):
        s = _ops.SCHEMA[o["code"]]
        if only_nonsquare and not ("H" in s.ix and "W" in s.ix and o.i("H") != o.i("W")):
            continue
        for nm in s.opts:
            if o.i(nm):
                got[nm] += 1
    return got


def test_the_table_holds_what_the_tiers_rely_on():
    assert len(set(NS.IDS)) == len(NS.CASES) == 11
    for c in NS.CASES:
        assert c.H != c.W and c.H % (1 << (NS.levels_of(c) - 1)) == 0 and c.W % (1 << (NS.levels_of(c) - 1)) == 0, c.name
        assert all(h != w for h, w in NS.pyramid(c)), c.name                          # no level of the pyramid is square: a swap shows everywhere
    shapes = {(c.model, tuple(c.filters), c.reversible): set() for c in NS.CASES}
    for c in NS.CASES:
        shapes[(c.model, tuple(c.filters), c.reversible)].add((c.H, c.W))
    assert sum(any((w, h) in s for h, w in s) for s in shapes.values()) == 4          # both orientations: narrow and wide PHISeg, narrow Unet, ProbabilisticUnet
    for name in NS.WIDE_PHISEG:
        c = NS.BY_NAME[name]
        assert c.filters == NS.WIDE7 and c.N * c.H * c.W > 32768                        # the large BatchNorm path
    assert all(NS.BY_NAME[n].filters[0] == 4 for n in NS.NARROW) and set(NS.VALIDATION) <= set(NS.NARROW) and set(NS.REPLAY) <= set(NS.IDS)


@pytest.mark.parametrize("name", NS.IDS)
def test_every_op_carries_a_plane_of_the_images_pyramid(name, plans):
    """Every op whose schema has H and W slots (and no D) holds (ceil(H0 / 2^l), ceil(W0 / 2^l)) for ONE level l - H and W swapped,
    or taken from different levels, is no plane of a non-square pyramid - and every N slot holds the case's batch.  The named
    exception: the ProbabilisticUnet's two Gaussian heads, 1 x 1 convolutions on the 1 x 1 plane behind the spatial mean."""
    c = NS.BY_NAME[name]
    p = plans(name)
    pyr = NS.pyramid(c)
    seen, checked = set(), 0
    for o in NS.tapes(p):
        s = _ops.SCHEMA[o["code"]]
        if "N" in s.ix:
            assert o.i("N") == c.N, (o["code"], o.i("N"))
        if "H" not in s.ix or "W" not in s.ix or "D" in s.ix:
            continue
        hw = tuple(o.i("H", "W"))
        if c.model == "probunet" and hw == (1, 1):
            assert o["code"] in _ops.CONV_KIND and o.i("ks") == 1 and o.i("cin") == c.filters[-1] and o.i("cout") == NS.LATENT, o
            continue
        assert hw in pyr, (o["code"], hw, sorted(pyr))
        seen.add(pyr[hw])
        checked += 1
    assert checked > 80 and seen == set(range(NS.levels_of(c))), (checked, seen)       # every level of the pyramid, image and deepest included


@pytest.mark.parametrize("name", NS.IDS)
def test_the_noise_buffers_have_the_oracles_shapes(name, plans):
    c = NS.BY_NAME[name]
    io = plans(name).io
    if c.model == "unet":
        assert "eps" not in io
        return
    bufs = io["eps"] if c.model == "phiseg" else [io["eps"]]
    got = [(v.N, v.C, v.H, v.W) for v in bufs]
    if c.model == "phiseg":
        want = oracle.phiseg_eps_shapes(c.N, c.H, c.W)
        assert got == want + want and want[0][2:] == (c.H // 64, c.W // 64) and want[-1][2:] == (c.H // 4, c.W // 4)
    else:
        assert got == [(c.N, NS.LATENT, 1, 1)]
    assert [tuple(s) for s in NS.eps_shapes(c)] == [g if c.model == "phiseg" else g[:2] for g in got]


@pytest.mark.parametrize("name", NS.WIDE_PHISEG)
def test_wide_phiseg_reaches_the_split_route_and_every_optional_form_off_the_square(name, plans):
    p = plans(name)
    routes = _routes(p, only_nonsquare=True)
    for kind in (0, 1, 2):
        assert routes[(kind, 1)] >= 1, (name, kind, dict(routes))                      # split-fp16 forward, data and weight gradient
        assert routes[(kind, 0)] >= 1, (name, kind, dict(routes))                      # ... beside fp32 layers of the same plan
    forms = _forms(p, only_nonsquare=True)
    for nm in OPTIONAL_FORMS:
        assert forms[nm] >= 1, (name, nm, dict(forms))
    assert len({o["lane"] for o in p.fwd_ops}) > 1 and len({o["lane"] for o in p.bwd_ops}) > 1


def test_the_two_wide_phiseg_cases_are_not_each_others_mirror(plans):
    tall, wide = (_forms(plans(n)) for n in NS.WIDE_PHISEG)
    assert tall["a_packed"] != wide["a_packed"] and tall["x_packed"] != wide["x_packed"], (dict(tall), dict(wide))
    assert _routes(plans(NS.WIDE_PHISEG[0]), True) != _routes(plans(NS.WIDE_PHISEG[1]), True)


@pytest.mark.parametrize("name", NS.NARROW)
def test_narrow_cases_stay_on_the_fp32_routes(name, plans):
    c = NS.BY_NAME[name]
    p = plans(name)
    routes = _routes(p, only_nonsquare=False)
    assert sum(routes.values()) > 50 and all(r != 1 for _, r in routes), (name, dict(routes))
    assert not any(_forms(p)[nm] for nm in ("x_packed", "a_packed", "y_packed", "dy_packed")), name
    if c.model == "phiseg" and not c.reversible:
        assert len({o["lane"] for o in p.fwd_ops}) > 1 and len({o["lane"] for o in p.bwd_ops}) > 1


@pytest.mark.parametrize("name", NS.IDS)
def test_reference_margin(name):
    """The fp32 oracle against the fp64 oracle on the case's inputs: loss within LOSS_REL, every forward tensor within FWD_CAP -
    the caps the GPU tier applies to the kernels, which a correct fp32 implementation therefore can meet - and the same set of
    parameters without a gradient.  Prints the reference's own distances (DESIGN.md section 5 quotes them)."""
    c = NS.BY_NAME[name]
    r32, r64 = NS.oracle_run(c, torch.float32), NS.oracle_run(c, torch.float64)
    rel = abs(r32.loss - r64.loss) / abs(r64.loss)
    fwd = {k: NS.maxabs(r32.fwd[k], r64.fwd[k]) for k in r64.fwd}
    keys = NS.grad_keys(r64)
    rc = NS.grad_ratios(lambda k: r32.grads[k], r64, keys)
    print(f"{name}: fp32 oracle vs fp64 oracle: loss rel {rel:.1e}, forward max {max(fwd.values()):.1e} at {max(fwd, key=fwd.get)}, gradients "
          f"median {np.median(rc):.1e} p90 {np.percentile(rc, 90):.1e} max {rc.max():.1e} over {len(keys)} tensors")
    if c.model != "unet":
        # not a gate: how far a second fp32 evaluation on the CPU (torch's other convolution backend) lies from the first - at these
        # batch sizes rounding noise is amplified chaotically, and the weight seeds of the two re-seeded cases were chosen with this
        alt = NS.second_fp32_run(c)
        ra = NS.grad_ratios(lambda k: alt.grads[k], r64, keys)
        print(f"{name}: second fp32 CPU evaluation: gradients median {np.median(ra):.1e} p90 {np.percentile(ra, 90):.1e} max {ra.max():.1e}; gates it "
              f"misses against the first: {[f[0] for f in NS.gradient_gates(ra, rc, keys)]}, the first against it: {[f[0] for f in NS.gradient_gates(rc, ra, keys)]}")
    assert np.isfinite(r64.loss) and rel <= NS.LOSS_REL, (name, rel)
    for k, v in r64.terms.items():
        assert abs(r32.terms[k] - v) <= NS.LOSS_REL * abs(v), (name, k, r32.terms[k], v)
    assert max(fwd.values()) <= NS.FWD_CAP, (name, fwd)
    assert r32.none_grads == r64.none_grads and len(keys) > 10
    assert all(float(r64.grads[k].abs().max()) > 0 for k in keys), name                # r = err / max |g64| is defined for every tensor
    b32, b64 = NS.expected_buffers(c, r32), NS.expected_buffers(c, r64)
    for k, v in b64.items():
        if k.endswith("running_mean"):
            assert NS.maxabs(b32[k], v) <= NS.RM_TOL, k
        elif k.endswith("running_var"):
            assert float(((b32[k].double() - v.double()).abs() / v.double().abs()).max()) <= NS.RV_REL, k
        else:
            assert torch.equal(b32[k], v), k


@pytest.mark.parametrize("name", NS.VALIDATION)
def test_validation_reference_labels_both_classes_off_a_tie(name):
    """The eval-mode forward of the oracle: fp32 within FWD_CAP of fp64; at most MARGIN_FRACTION of the pixels have their two
    largest accumulated fp64 logits closer than MARGIN, and both classes label at least a tenth of the image - the argmax
    comparison of the GPU tier covers nearly every pixel and cannot pass on a constant map."""
    c = NS.validation_case(name)
    r32, r64 = NS.oracle_run(c, torch.float32, train=False), NS.oracle_run(c, torch.float64, train=False)
    assert max(NS.maxabs(r32.fwd[k], r64.fwd[k]) for k in r64.fwd) <= NS.FWD_CAP
    acc = NS.accumulated(c, r64)
    frac, sure = NS.unsure_fraction(acc)
    counts = np.bincount(acc.argmax(dim=1).reshape(-1).numpy(), minlength=2)
    print(f"{name}: {frac:.1e} of the pixels within {NS.MARGIN} of a tie, labels {counts.tolist()}")
    assert frac <= NS.MARGIN_FRACTION and counts.min() >= 0.1 * counts.sum(), (frac, counts)
    assert torch.equal(NS.accumulated(c, r32).argmax(dim=1)[sure], acc.argmax(dim=1)[sure])


@pytest.mark.parametrize("no_convs", sorted(NS.PROBUNET_PREDICT_SEEDS))
def test_the_oracle_decides_the_labels_of_the_tall_predict_case(no_convs):
    """As test_fcomb_cpu.test_the_oracle_decides_the_labels_of_the_model_level_cases, for the tall shape of this file."""
    from tests import _fcomb as F
    m = NS.probunet_predict_case(no_convs)
    B, S, H, W = NS.PREDICT_SHAPE
    assert H > W and (B, S, W, H) in F.SHAPES                                         # the transpose of the existing wide case
    assert m.logits.shape == (S * B, 2, H, W) and m.z.shape == (S * B, F.LATENT)
    assert 1.0 - float(m.sure.float().mean()) <= 0.01
    assert 0.2 <= float(m.labels.float().mean()) <= 0.8
    assert float(m.sigma.min()) > 0.1
    rows = m.logits.reshape(S, B, 2, H, W)
    assert all(not bool((rows[s] == rows[0]).all()) for s in range(1, S))


KINK_MARGIN = 1e-5      # the device was seen to take the other side of a ReLU whose fp64 input is 6.3e-6 (tests/_nonsquare.py, RESEEDED)


@pytest.mark.parametrize("name", [c.name for c in NS.CASES if c.model != "unet"])
def test_small_plane_relus_keep_their_distance_from_the_kink(name):
    """Where the case's size allows it - the narrow PHISeg and the ProbabilisticUnet cases - the weight seed keeps every ReLU input
    on a plane of at most 1 024 pixels at least KINK_MARGIN from zero in the fp64 oracle, so that an fp32 forward within 1e-5 cannot
    decide a mask the other way.  The wide and the reversible cases hold 10 - 30 x as many such values and no seed of 77 .. 116
    keeps them beyond 4e-6: for them the figure is printed only."""
    c = NS.BY_NAME[name]
    margin = NS.relu_kink_margin(c)
    print(f"{name}: smallest |ReLU input| on planes of at most 1024 pixels, fp64 oracle: {margin:.1e}")
    assert 0 < margin < 1.0
    if c.filters == NS.NARROW7 and not c.reversible or c.model == "probunet":
        assert margin >= KINK_MARGIN, (name, margin)


@pytest.mark.parametrize("shape", [(64, 128), (128, 64)])
def test_scale_augmentation_is_refused_off_the_square(shape):
    """Found by the harness test of the GPU tier: the reference's scale augmentation draws one crop side from the image's width and
    the crop's position on each axis from the other axis' size, so on a 64 x 128 image a draw failed inside numpy ("high <= 0") for
    about every second batch - and the synthetic stand-in data asked for it at every image size.  It is refused with a message now,
    whatever the draws, and rotations and flips go on working."""
    from unet_zoo_amd.data import batch_provider as BP
    np.random.seed(0)
    for _ in range(20):                                                               # whatever the draws
        with pytest.raises(ValueError, match="non-square"):
            BP.draw_augmentation(2, shape, dict(do_rotations=True, do_scaleaug=True, nlabels=2))
    prm = BP.draw_augmentation(64, shape, dict(do_rotations=True, do_scaleaug=False, do_fliplr=True, nlabels=2, augment_every_nth=1))
    assert prm.shape == (64, 8) and prm[:, 0].all() and not prm[:, 3].any() and prm[:, 7].any()
    assert BP.draw_augmentation(8, (64, 64), dict(do_scaleaug=True, nlabels=2, augment_every_nth=1))[:, 3].all()      # the square is what it was
