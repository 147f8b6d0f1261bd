"""PHiSeg3D (BASELINE config 5; reference models/phiseg3D.py).  The reference's own forward cannot complete (its
last statement, :398, raises on 5-D input) - parity is pinned on what it does execute: the fixtures tests/golden/phiseg3d_*.npz
come from its Posterior / prior / Likelihood modules, its loss functions and autograd (tools/gen_golden.py `3d`), and
tests/test_oracle_golden.py checks the oracle against them.  Here: the native model against those fixtures and the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import refgraph3d as R3
import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ops
from tests import _golden as G


def _b16_word(o):
    """The storage-format bits of op `o`; 0 for an op that has no bf16-storage form."""
    return o.i("b16") if _ops.SCHEMA[o["code"]].b16 else 0


# ----------------------------------------------------------------------------- host side (CPU tier)
@pytest.mark.parametrize("name", ["phiseg3d_small", "phiseg3d_l3"])
def test_state_dict_keys_match_the_reference_model(name):
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    _, meta = G.load(name)
    net = PHISeg3D(meta["input_channels"], meta["num_classes"], meta["filters"], latent_levels=meta["latent_levels"], device="cpu")
    ours = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    ref = {k: tuple(s) for k, s, _ in meta["spec"]}                 # the real reference module's state_dict (keys, shapes)
    assert ours == ref and list(ours) == list(ref)


def test_plan_builds_schedules_and_rejects_what_the_reference_rejects():
    from tests.test_host_cpu import _check_lane_schedule
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    arena = {}
    for rev in (False, True):
        net = PHISeg3D(4, 3, [8, 16, 16], latent_levels=2, reversible=rev, device="cpu")
        plan = net._build(16, 32, 32, True, True)
        for which, ops in (("fwd", plan.fwd_ops), ("bwd", plan.bwd_ops)):
            pairs, _, _ = _check_lane_schedule(plan, which, ops)
            assert pairs > 100
        codes = [o["code"] for o in plan.fwd_ops]
        assert "UZ_OP_W3D_PERMUTE" in codes and "UZ_OP_AVGPOOL3D_FWD" in codes and "UZ_OP_DEPTH_LERP_FWD" in codes
        arena[rev] = plan.summary()["arena_MB"]
    assert arena[True] < arena[False]
    with pytest.raises(ValueError):                                 # likelihood_post_c_path channel arithmetic (phiseg3D.py:343,372)
        PHISeg3D(4, 3, [8, 16, 32], latent_levels=2, device="cpu")
    net = PHISeg3D(4, 3, [8, 16, 16], latent_levels=2, device="cpu")
    with pytest.raises(ValueError):
        net._build(10, 32, 32, True, True)                          # 10 is not divisible by 2^(levels-1)
    with pytest.raises(RuntimeError):                               # no CPU fallback
        net.forward(torch.zeros(1, 4, 16, 32, 32), torch.zeros(1, 3, 16, 32, 32))


@pytest.mark.parametrize("reversible", [False, True])
@pytest.mark.parametrize("filters,latent_levels", [([8, 16, 16], 3), ([8, 16, 16], 2), ([8, 16, 16, 16], 2)])   # level difference 0, 1, 2
def test_every_level_layout_builds_its_train_eval_and_decode_plans(filters, latent_levels, reversible):
    from unet_zoo_amd.models.phiseg3D import PHISeg3D, phiseg3d_spec
    cin, K, dhw = 4, 3, (16, 32, 32)
    net = PHISeg3D(cin, K, filters, latent_levels=latent_levels, reversible=reversible, device="cpu")
    assert len(phiseg3d_spec(cin, K, filters, latent_levels, reversible)) == len(net.state_dict())
    for args in ((True, True), (False, False), (False, False, True)):           # train, eval, decode
        io = net._build(*dhw, *args).io
        assert [(v.N, v.C, v.H, v.W) for v in io["s"]] == [(dhw[0], K, dhw[1], dhw[2])] * latent_levels
        if not args[2:]:
            assert len(io["eps"]) == 2 * latent_levels


def test_bf16_storage_pass_marks_buffers_and_operands_consistently(monkeypatch):
    """Plan._b16_pass (BASELINE config 5, bf16 STORAGE): which volume tensors become 2-byte buffers is decided per buffer from its
    readers and writers; every op then carries one format bit per tensor operand (i[13]).  Checked here on the CPU: the bits of every
    op agree with the buffers behind its operands (a bf16 buffer read as fp32, or the reverse, would be silent garbage on the device),
    only ops with a bf16-storage form touch a bf16 buffer, a unit's three backward ops agree on their dy scratch class, the arena
    shrinks, the lane schedule still orders every hazard, and nothing changes outside the bf16 arithmetic mode."""
    from tests.test_host_cpu import _check_lane_schedule
    from unet_zoo_amd import _ffi
    from unet_zoo_amd._plan import View, _ScratchView
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    L = _ffi.lib()

    def build(b16, mode):
        monkeypatch.setenv("UZ_STORE_B16", b16)
        L.uz_set_conv_math(mode)
        try:
            net = PHISeg3D(4, 3, [32, 64, 64], latent_levels=2, device="cpu")
            return net._build(32, 64, 64, True, True)
        finally:
            L.uz_set_conv_math(-1)
    off = build("0", 3)
    on = build("1", 3)
    assert off.b16_info["buffers"] == 0 and not any(b.b16 for b in off.bufs) and not any(_b16_word(o) for o in off.fwd_ops + off.bwd_ops)
    assert build("1", 1).b16_info["buffers"] == 0                   # the fp32-accurate split mode never stores bf16
    info = on.b16_info
    assert info["buffers"] >= 10 and info["grads"] >= 5 and info["dy"] >= 5 and info["ops"] >= 40, info
    assert on.arena_floats < 0.8 * off.arena_floats
    assert all(b.vol and b.W % 32 == 0 and (b.N - 2) * b.H * b.W > 32768 for b in on.bufs if b.b16)

    def fmt(r):
        if isinstance(r, View):
            return r.buf.b16
        if isinstance(r, tuple) and r and r[0] == "win":
            return r[1].buf.b16
        if isinstance(r, _ScratchView) and r.zkey is not None:
            return len(r.zkey) > 2
        if isinstance(r, tuple) and r and r[0] in ("gyvol", "gywin"):
            return len(r[1]) > 2
        return None
    flagged = 0
    for ops in (on.fwd_ops, on.loss_ops, on.bwd_ops):
        for o in ops:
            slots = dict(on._b16_slots(o))
            bits = _b16_word(o)
            for j, r in enumerate(o["p"]):
                f = fmt(r)
                if f is None:
                    continue
                if j in slots:
                    assert bool((bits >> slots[j]) & 1) == bool(f), (o["code"], j, bits)
                    flagged += bool(f)
                else:
                    assert not f, (o["code"], j)                     # an operand slot without a bf16 form only ever sees fp32 buffers
            assert not bits or on._b16_ok(o)
    assert flagged >= 100
    for which, ops in (("fwd", on.fwd_ops), ("bwd", on.bwd_ops)):
        _check_lane_schedule(on, which, ops)
    # bench.py prices every operand at its storage width (the HBM fractions of the bf16 line would otherwise be 2x too high)
    import bench
    for o in on.fwd_ops + on.bwd_ops:
        bits = _b16_word(o)
        if o["code"] == "UZ_OP_BN_RELU_BWD" and bits == 7:
            C, N, H, W = o.i("C", "N", "H", "W")
            assert bench.op_bytes(o) == C * N * H * W * (2 * (2 + 2) + 2) == bench.op_bytes(dict(o, i=o["i"][:_ops.B16_SLOT])) / 2
        if o["code"] == "UZ_OP_CONV_FWD" and bits == 3 and o.i("ks") == 3:
            assert bench.conv_bytes(o) < 0.55 * bench.conv_bytes(dict(o, i=o["i"][:_ops.B16_SLOT])) + 4.0 * o.i("cin") * o.i("cout") * 9
    # byte-typed pointers: consecutive bf16 buffers are packed at 2 bytes per element
    b = next(b for b in on.bufs if b.b16)
    assert b.words == (b.numel + 1) // 2 and on.tensor(View(b)).dtype == torch.bfloat16 and on.tensor(View(b)).shape == (b.N, b.C, b.H, b.W)
    v = View(b, 1, b.C - 1, 1, b.N - 2)
    assert on._resolve(v) - on._resolve(View(b)) == 2 * (b.C + 1) * b.H * b.W


def test_brats_experiment_file_resolves_to_the_native_model(tmp_path):
    """The reference's phiseg_brats.py, rebuilt in its layout from the stored settings (golden/reference_experiments.json)."""
    from tests import _golden as G
    from unet_zoo_amd import train_model as TM
    cfg = TM.load_experiment(G.reference_experiment_file("phiseg_brats", tmp_path))
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    assert cfg.model is PHISeg3D and cfg.image_size == (4, 128, 128, 128) and cfg.use_reversible is True
    # the file's own filter list does not satisfy the reference's channel arithmetic: constructing it raises there too
    with pytest.raises(ValueError):
        cfg.model(cfg.input_channels, cfg.n_classes, cfg.filter_channels, latent_levels=cfg.latent_levels, device="cpu")


# ----------------------------------------------------------------------------- device kernels vs torch
def _g():
    from tests import _gpu
    return _gpu


def _vol(t):
    """(C, D, H, W) CPU tensor -> GPU volume [D + 2][C][H][W] with zero border slices; returns (storage, interior view)."""
    c, d, h, w = t.shape
    buf = torch.zeros(d + 2, c, h, w, device="cuda")
    buf[1:d + 1] = t.permute(1, 0, 2, 3).to("cuda")
    return buf, buf[1:d + 1]


def _unvol(v):
    return v.permute(1, 0, 2, 3).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("C,D,H,W", [(3, 6, 10, 8), (5, 7, 9, 11)])
def test_avgpool3d_trilinear_nearest_vs_torch(C, D, H, W):
    g = _g()
    x = g.rnd(C, D, H, W, seed=1)
    xr = x.clone()[None].requires_grad_(True)
    # AvgPool3d(2, 2, ceil_mode=True)
    yr = F.avg_pool3d(xr, 2, 2, 0, ceil_mode=True)
    Do, Ho, Wo = yr.shape[-3:]
    _, xv = _vol(x)
    ybuf = torch.zeros(Do + 2, C, Ho, Wo, device="cuda")
    g.call("uz_avgpool3d_fwd", xv, C, C, ybuf[1:], C, D, H, W)
    assert g.maxabs(_unvol(ybuf[1:Do + 1]), yr[0]) <= 1e-6
    assert float(ybuf[0].abs().max()) == 0 and float(ybuf[Do + 1].abs().max()) == 0
    dy = g.rnd(*yr.shape[1:], seed=2)
    yr.backward(dy[None])
    _, dyv = _vol(dy)
    dx = torch.full((D, C, H, W), float("nan"), device="cuda")
    g.call("uz_avgpool3d_bwd", dyv, C, C, dx, C, D, H, W, 0)
    assert g.maxabs(_unvol(dx), xr.grad[0]) <= 1e-6
    g.call("uz_avgpool3d_bwd", dyv, C, C, dx, C, D, H, W, 1)
    assert g.maxabs(_unvol(dx), 2 * xr.grad[0]) <= 2e-6
    # trilinear x2, align_corners=True = the 2-D bilinear kernel per slice + the depth interpolation
    xr.grad = None
    tr = F.interpolate(xr, scale_factor=2, mode="trilinear", align_corners=True)
    mid = torch.zeros(D + 2, C, 2 * H, 2 * W, device="cuda")
    g.call("uz_bilinear2x_fwd", xv, C, C, mid[1:], C, D, H, W, 1, None, None)
    out = torch.zeros(2 * D + 2, C, 2 * H, 2 * W, device="cuda")
    g.call("uz_depth_lerp2x_fwd", mid[1:], C, C, out[1:], C, D, 2 * H, 2 * W)
    assert g.maxabs(_unvol(out[1:2 * D + 1]), tr[0]) <= 2e-6
    dt = g.rnd(*tr.shape[1:], seed=3)
    tr.backward(dt[None])
    _, dtv = _vol(dt)
    dmid = torch.full((D, C, 2 * H, 2 * W), float("nan"), device="cuda")
    g.call("uz_depth_lerp2x_bwd", dtv, C, C, dmid, C, D, 2 * H, 2 * W, 0)
    dx2 = torch.full((D, C, H, W), float("nan"), device="cuda")
    g.call("uz_bilinear2x_bwd", dmid, C, C, dx2, C, D, H, W, 1, 0)
    assert g.maxabs(_unvol(dx2), xr.grad[0]) <= 1e-5
    # nearest resize by integer factors
    xr.grad = None
    nr = F.interpolate(xr, size=[2 * D, 4 * H, 4 * W], mode="nearest")
    nout = torch.zeros(2 * D + 2, C, 4 * H, 4 * W, device="cuda")
    g.call("uz_nearest3d_fwd", xv, C, C, nout[1:], C, D, H, W, 4, 2)
    assert g.maxabs(_unvol(nout[1:2 * D + 1]), nr[0]) == 0
    dn = g.rnd(*nr.shape[1:], seed=4)
    nr.backward(dn[None])
    _, dnv = _vol(dn)
    dx3 = torch.full((D, C, H, W), float("nan"), device="cuda")
    g.call("uz_nearest3d_bwd", dnv, C, C, dx3, C, D, H, W, 4, 2, 0)
    assert g.maxabs(_unvol(dx3), xr.grad[0]) <= 1e-5
    # large factors (>= 64 children per element: one wave per element sums them), overwrite and accumulate
    for f, fz in ((4, 4), (8, 8)):
        xr.grad = None
        nr = F.interpolate(xr, size=[fz * D, f * H, f * W], mode="nearest")
        dn = g.rnd(*nr.shape[1:], seed=5)
        nr.backward(dn[None])
        _, dnv = _vol(dn)
        dx4 = torch.full((D, C, H, W), float("nan"), device="cuda")
        g.call("uz_nearest3d_bwd", dnv, C, C, dx4, C, D, H, W, f, fz, 0)
        assert g.maxabs(_unvol(dx4), xr.grad[0]) <= 1e-5 * f * f * fz
        g.call("uz_nearest3d_bwd", dnv, C, C, dx4, C, D, H, W, f, fz, 1)
        assert g.maxabs(_unvol(dx4), 2 * xr.grad[0]) <= 2e-5 * f * f * fz


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,D,H,W", [(4, 8, 6, 12, 10), (16, 32, 8, 16, 16), (2, 16, 4, 8, 8)])
def test_conv3d_as_depth_window_vs_torch(Cin, Cout, D, H, W):
    """Conv3d(3x3x3, pad 1) through the C ABI: uz_w3d_permute + uz_conv_fwd / uz_conv_bwd_weight / uz_conv_bwd_data on the
    [D + 2][C][H][W] volume with the depth window as 3 Cin channels (include/uz_api.h, volumes section)."""
    from unet_zoo_amd import _ffi
    g = _g()
    L = _ffi.lib()
    x = g.rnd(Cin, D, H, W, seed=1)
    w = g.rnd(Cout, Cin, 3, 3, 3, seed=2, scale=0.2)
    b = g.rnd(Cout, seed=3)
    xr, wr = x.clone()[None].requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv3d(xr, wr, b, padding=1)
    dy = g.rnd(Cout, D, H, W, seed=4)
    yr.backward(dy[None])
    xbuf, xv = _vol(x)
    wd, bd = w.cuda(), b.cuda()
    wp = torch.empty(Cout * Cin * 27, device="cuda")
    g.call("uz_w3d_permute", wd, wp, Cout, Cin, 0)
    ws_b = max(L.uz_conv_workspace(3 * Cin, Cout, D, H, W, 3), L.uz_conv_workspace(Cin, 3 * Cout, D, H, W, 3),
               L.uz_conv_bwd_weight_workspace(3 * Cin, Cout, D, H, W, 3))
    ws = torch.empty(ws_b // 4 + 16, device="cuda")
    y = torch.full((D, Cout, H, W), float("nan"), device="cuda")
    g.call("uz_conv_fwd", xbuf, 3 * Cin, Cin, wp, bd, y, Cout, Cout, D, H, W, 3, 0, None, None, None, ws, ws_b)
    assert g.relerr(_unvol(y), yr[0]) <= 2e-5
    # weight gradient in the window layout, permuted back to [co][ci][kd][kh][kw]
    dybuf, dyv = _vol(dy)
    # a depth-window call (3 Cin view channels over a Cin-channel buffer) leaves its gradient in the Conv3d parameter layout
    # [Cout][Cin][3][3][3] itself: the slab reduction permutes on the way out (round 3; it used to need uz_w3d_permute mode 2)
    dw = torch.empty(Cout, Cin, 3, 3, 3, device="cuda")
    g.call("uz_conv_bwd_weight", xbuf, 3 * Cin, Cin, dyv, Cout, Cout, dw, None, D, H, W, 3, None, None, ws, ws_b)
    assert g.relerr(dw, wr.grad) <= 2e-5
    # data gradient: the dy volume read through a depth window of 3 Cout channels against the depth-flipped weights
    wp2 = torch.empty(Cout * Cin * 27, device="cuda")
    g.call("uz_w3d_permute", wd, wp2, Cout, Cin, 1)
    dx = torch.full((D, Cin, H, W), float("nan"), device="cuda")
    g.call("uz_conv_bwd_data", dybuf, 3 * Cout, Cout, wp2, dx, Cin, Cin, D, H, W, 3, 0, None, None, ws, ws_b)
    assert g.relerr(_unvol(dx), xr.grad[0]) <= 2e-5


# ----------------------------------------------------------------------------- model vs the reference's modules / the oracle
def _run_native(meta, arrays, reversible=False, sd=None, training=True):
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    dev = torch.device("cuda", 0)
    L = meta["latent_levels"]
    net = PHISeg3D(meta["input_channels"], meta["num_classes"], meta["filters"], latent_levels=L, reversible=reversible,
                   image_size=(meta["input_channels"], *meta["dhw"]))
    net.load_state_dict(sd if sd is not None else oracle.deterministic_state_dict(G.spec_of(meta), seed=meta["weight_seed"]))
    net.train()
    T = lambda k: torch.from_numpy(arrays[k]).to(dev)       # noqa: E731
    s = net.forward(T("patch"), T("mask_onehot"), training=training, eps=[T(f"eps{k}") for k in range(2 * L)])
    loss = net.loss(T("labels"))
    return net, s, loss


@pytest.fixture
def conv_math(request):
    """`split`: the split-fp16 kernels (and the pre-packed depth-window weight images) on every 3x3x3 layer, also on planes the
    default policy leaves to the fp32 kernels - the fixtures' volumes are small."""
    from unet_zoo_amd import _ffi
    if request.param == "split":
        _ffi.lib().uz_set_conv_math(2)
    yield request.param
    _ffi.lib().uz_set_conv_math(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("conv_math", ["default", "split"], indirect=True)
@pytest.mark.parametrize("name", ["phiseg3d_small", "phiseg3d_l3"])
def test_native_model_vs_reference_modules(name, conv_math):
    arrays, meta = G.load(name)
    L = meta["latent_levels"]
    net, s, loss = _run_native(meta, arrays)
    if conv_math == "split":
        assert len(net._cur._packs["fwd"]) > 10 and len(net._cur._packs["bwd"]) > 10
    tol = lambda ref: 1e-4 * max(1.0, float(np.abs(ref).max()))     # noqa: E731  (north_star: within 1e-4 fp32)
    for l in range(L):
        for attr, key in ((net.posterior_mu, "post_mu"), (net.posterior_sigma, "post_sigma"), (net.posterior_latent_space, "post_z"),
                          (net.prior_mu, "prior_mu"), (net.prior_sigma, "prior_sigma"), (net.s_in_list, "s_in")):
            ref = arrays[f"{key}{l}"]
            got = attr[l].cpu().numpy()
            assert got.shape == ref.shape, (key, l, got.shape, ref.shape)
            assert G.maxabs(got, ref) <= tol(ref), (key, l, G.maxabs(got, ref))
    # the resized level logits: nearest resize of s_in to the full volume (the statement the reference cannot execute)
    D, H, W = meta["dhw"]
    for l in range(L):
        want = F.interpolate(torch.from_numpy(arrays[f"s_in{l}"]), size=[D, H, W], mode="nearest").numpy()
        assert s[l].shape == want.shape and G.maxabs(s[l].cpu().numpy(), want) <= tol(want)
    ref_loss = float(arrays["loss"])
    assert abs(float(loss) - ref_loss) <= 5e-5 * abs(ref_loss), (float(loss), ref_loss)
    for l in range(L):
        for nm in ("KL_divergence_loss_lvl%d" % l, "residual_multinoulli_loss_lvl%d" % l):
            r = float(arrays["loss:" + nm])
            assert abs(float(net.loss_dict[nm]) - r) <= 1e-4 * max(1.0, abs(r)), nm
    bn_fwd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if "running_" in k}
    loss.backward()
    noise = G.bn_shadowed_biases([k for k, _, _ in meta["spec"]])
    worst, wk, n = 0.0, None, 0
    for k, p in net.named_parameters():
        if ("g:" + k) not in arrays:
            assert p.grad is None or k in meta["no_grad"] or float(p.grad.abs().max()) == 0.0, k
            continue
        if k in noise:
            continue
        ref = arrays["g:" + k]
        err = G.maxabs(p.grad.cpu().numpy(), ref) / (float(np.abs(ref).max()) + 1e-30)
        n += 1
        if err > worst:
            worst, wk = err, k
    print(f"{name}: loss rel {abs(float(loss) - ref_loss) / abs(ref_loss):.1e}; worst gradient deviation {worst:.2e} at {wk} over {n} tensors")
    assert n > 40 and worst <= 2e-3, (worst, wk)
    for k, v in bn_fwd.items():
        ref = arrays["sd1:" + k]
        assert G.maxabs(v, ref) <= 1e-4 * max(1.0, float(np.abs(ref).max())), k


@pytest.mark.gpu
def test_native_reversible_and_eval_vs_oracle():
    """reversible=True (ReversibleSequence, reversible_depth 1: phiseg3D.py:61-86) and the training=False path against the
    oracle (revtorch is not importable: parity unpinned for the reversible variant, see oracle/refgraph.py:rev_sequence)."""
    from unet_zoo_amd.models.phiseg3D import phiseg3d_spec
    arrays, meta = G.load("phiseg3d_small")
    L = meta["latent_levels"]
    T = lambda k: torch.from_numpy(arrays[k])       # noqa: E731
    eps = [T(f"eps{k}") for k in range(2 * L)]
    for rev in (True, False):
        spec = phiseg3d_spec(meta["input_channels"], meta["num_classes"], meta["filters"], L, reversible=rev)
        sd0 = oracle.deterministic_state_dict(spec, seed=77)
        for k, v in sd0.items():
            if rev and k.endswith("convolution.1.weight"):
                sd0[k] = v * 0.3
        training = rev                                       # reversible: training graph; plain: the prior-sampling graph
        net, s, loss = _run_native(meta, arrays, reversible=rev, sd=sd0, training=training)
        lv = G.leaves(sd0)
        out = R3.phiseg3d_forward(lv, T("patch"), T("mask_onehot"), eps, training=training, bn_train=True)
        total, _ = R3.phiseg3d_loss(out, T("labels"), num_classes=meta["num_classes"])
        assert abs(float(loss) - float(total)) <= 5e-5 * abs(float(total)), (rev, float(loss), float(total))
        for l in range(L):
            ref = out["s"][l].detach().numpy()
            assert G.maxabs(s[l].cpu().numpy(), ref) <= 2e-4 * max(1.0, float(np.abs(ref).max())), (rev, l)
        if not rev:
            continue
        loss.backward()
        total.backward()
        noise = G.bn_shadowed_biases(lv.keys())
        worst, wk = 0.0, None
        for k, p in net.named_parameters():
            ref = lv[k].grad
            if ref is None or k in noise:
                continue
            err = G.maxabs(p.grad.cpu().numpy(), ref.numpy()) / (float(ref.abs().max()) + 1e-30)
            if err > worst:
                worst, wk = err, k
        print(f"reversible PHiSeg3D: worst gradient deviation {worst:.2e} at {wk}")
        assert worst <= 5e-3, (worst, wk)


@pytest.mark.gpu
def test_native_reconstruct_and_sample_vs_oracle():
    """reconstruct(z) / sample() (phiseg3D.py:443-452): the likelihood on given latent volumes + accumulate_output."""
    arrays, meta = G.load("phiseg3d_small")
    L = meta["latent_levels"]
    net, s, _ = _run_native(meta, arrays, training=False)
    net.eval()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}      # incl. the BN buffers the training-mode forward just updated
    z = [torch.randn(*arrays[f"post_z{l}"].shape, generator=torch.Generator().manual_seed(5 + l)) for l in range(L)]
    recon, layers = net.reconstruct([t.cuda() for t in z], use_softmax=True)
    want_s, _ = R3.likelihood3d(sd, z, bn_train=False, full_size=meta["dhw"])
    acc = want_s[-1].clone()
    for l in range(L - 1):
        acc = acc + want_s[l]
    for l in range(L):
        # the reference accumulates IN PLACE into the coarsest level's tensor (phiseg3D.py:469-472), which it also returns
        ref = acc if l == L - 1 else want_s[l]
        assert G.maxabs(layers[l].cpu().numpy(), ref.numpy()) <= 1e-4 * max(1.0, float(ref.abs().max())), l
    assert G.maxabs(recon.cpu().numpy(), torch.softmax(acc, dim=1).numpy()) <= 1e-5
    smp = net.sample(testing=True)
    assert smp.shape == (1, meta["num_classes"], *meta["dhw"]) and bool(torch.isfinite(smp).all())
    with pytest.raises(NotImplementedError):
        net.sample(testing=False)


@pytest.mark.gpu
def test_native_five_level_volume_trains():
    """BASELINE config 5's shape class at a test-sized volume: 5 resolution / 5 latent levels, 4 input channels, 3 labels,
    hipGraph replay + fused Adam: loss matches the oracle at step 0, stays finite and decreases over a few steps."""
    from unet_zoo_amd.models.phiseg3D import PHISeg3D, phiseg3d_spec
    from unet_zoo_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    filters, dhw, K, Cin = [8, 16, 32, 32, 32], (32, 32, 16), 3, 4
    sd0 = oracle.deterministic_state_dict(phiseg3d_spec(Cin, K, filters, 5), seed=5)
    shapes = R3.phiseg3d_eps_shapes(*dhw, 5, 5)
    x, onehot, lab, eps = R3.synthetic_volume(Cin, K, dhw, 3, shapes + shapes)
    net = PHISeg3D(Cin, K, filters, latent_levels=5, image_size=(Cin, *dhw))
    net.load_state_dict(sd0)
    net.train()
    xd, od, ld = (torch.from_numpy(a).to(dev) for a in (x, onehot, lab))
    net.forward(xd, od, training=True, eps=[torch.from_numpy(e).to(dev) for e in eps])
    loss0 = float(net.loss(ld))
    out = R3.phiseg3d_forward(G.leaves(sd0), torch.from_numpy(x), torch.from_numpy(onehot), [torch.from_numpy(e) for e in eps])
    total, _ = R3.phiseg3d_loss(out, torch.from_numpy(lab), num_classes=K)
    assert abs(loss0 - float(total)) <= 1e-4 * abs(float(total)), (loss0, float(total))
    net.enable_graphs(True)
    opt = FusedAdam(net, lr=1e-3, weight_decay=1e-5)
    losses = []
    for _ in range(6):
        net.forward(xd, od, training=True, eps=[torch.from_numpy(e).to(dev) for e in eps])
        l = net.loss(ld)
        opt.zero_grad()
        l.backward()
        opt.step()
        losses.append(float(l))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


@pytest.mark.gpu
def test_baseline_config5_architecture_at_full_volume_size():
    """BASELINE.json configs[4] at its real size: PHISeg3D 5 resolution / 5 latent levels, filters 32-64-128-192-192, 4 input
    channels, 3 labels, one 128 x 128 x 64 volume per GPU, default math (the bf16 arithmetic the config names: next-but-one test;
    storage is fp32 in both).  (a) The same network and weights on a 64 x 64 x 32 sub-volume against the CPU oracle (the full
    volume costs the oracle minutes): loss within 1e-4 relative, level logits within 1e-4 of their range.  (b) At full size:
    three hipGraph-replayed training steps, loss finite and decreasing, no violated magnitude bound."""
    from unet_zoo_amd.models.phiseg3D import PHISeg3D, phiseg3d_spec
    from unet_zoo_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    filters, K, Cin = [32, 64, 128, 192, 192], 3, 4
    sd0 = oracle.deterministic_state_dict(phiseg3d_spec(Cin, K, filters, 5), seed=11)
    # (a) sub-volume vs oracle
    dhw = (64, 64, 32)
    shapes = R3.phiseg3d_eps_shapes(*dhw, 5, 5)
    x, onehot, lab, eps = R3.synthetic_volume(Cin, K, dhw, 7, shapes + shapes)
    net = PHISeg3D(Cin, K, filters, latent_levels=5, image_size=(Cin, *dhw))
    net.load_state_dict(sd0)
    net.train()
    xd, od, ld = (torch.from_numpy(a).to(dev) for a in (x, onehot, lab))
    s_native = net.forward(xd, od, training=True, eps=[torch.from_numpy(e).to(dev) for e in eps])
    loss0 = float(net.loss(ld))
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = R3.phiseg3d_forward(G.leaves(sd0), torch.from_numpy(x), torch.from_numpy(onehot), [torch.from_numpy(e) for e in eps])
    total, _ = R3.phiseg3d_loss(out, torch.from_numpy(lab), num_classes=K)
    assert abs(loss0 - float(total)) <= 1e-4 * abs(float(total)), (loss0, float(total))
    del net
    torch.cuda.empty_cache()
    # (b) the full 128 x 128 x 64 volume
    dhw = (128, 128, 64)
    shapes = R3.phiseg3d_eps_shapes(*dhw, 5, 5)
    x, onehot, lab, eps = R3.synthetic_volume(Cin, K, dhw, 9, shapes + shapes)
    net = PHISeg3D(Cin, K, filters, latent_levels=5, image_size=(Cin, *dhw))
    net.load_state_dict(sd0)
    net.train()
    net.enable_graphs(True)
    opt = FusedAdam(net, lr=1e-3, weight_decay=1e-5)
    xd, od, ld = (torch.from_numpy(a).to(dev) for a in (x, onehot, lab))
    epsd = [torch.from_numpy(e).to(dev) for e in eps]
    losses = []
    for _ in range(4):
        net.forward(xd, od, training=True, eps=epsd)
        l = net.loss(ld)
        opt.zero_grad()
        l.backward()
        opt.step()
        losses.append(float(l))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert net.check_bounds() == 0
    out = net.forward(xd, od, training=True, eps=epsd)
    assert len(out) == 5 and tuple(out[0].shape[-3:]) == dhw and all(bool(torch.isfinite(o).all()) for o in out)


@pytest.mark.gpu
def test_bf16_arithmetic_mode_against_the_operand_rounding_oracle():
    """BASELINE configs[4] is quoted in bf16.  UZ_CONV_MATH=bf16 (uz_set_conv_math(3)) runs the large 3x3x3 convolutions with ONE
    bf16 piece per operand and one MFMA product, fp32 accumulation, fp32 storage.  The oracle gets the same rounding on exactly the
    layers the library routes that way (oracle.refgraph.CONV_OPERAND_ROUNDING + uz_conv_route), so the forward comparison is
    tight again: loss within 2e-4 relative, level logits within 2e-3 of their range (bf16 rounding decisions can flip on the
    last fp32 bit of an activation, so this is not the 1e-4 of the fp32 modes); against the UN-rounded fp32 oracle the loss moves
    by less than 2 % - the price of bf16 arithmetic, stated, not hidden.  Then three training steps: finite and decreasing."""
    from unet_zoo_amd import _ffi
    from unet_zoo_amd.models.phiseg3D import PHISeg3D, phiseg3d_spec
    from unet_zoo_amd.optim import FusedAdam
    from oracle import refgraph as RG
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    filters, dhw, K, Cin = [32, 64, 128, 192, 192], (64, 64, 32), 3, 4
    sd0 = oracle.deterministic_state_dict(phiseg3d_spec(Cin, K, filters, 5), seed=13)
    shapes = R3.phiseg3d_eps_shapes(*dhw, 5, 5)
    x, onehot, lab, eps = R3.synthetic_volume(Cin, K, dhw, 5, shapes + shapes)
    try:
        L.uz_set_conv_math(3)

        def routed(xx, ww):                              # the library's own routing decision for this layer's forward convolution
            if ww.dim() != 5 or ww.shape[-1] != 3:
                return False
            _, c, d, h, w_ = xx.shape
            return L.uz_conv_route(0, 3 * c, ww.shape[0], d, h, w_, 3) == 1
        net = PHISeg3D(Cin, K, filters, latent_levels=5, image_size=(Cin, *dhw))
        net.load_state_dict(sd0)
        net.train()
        xd, od, ld = (torch.from_numpy(a).to(dev) for a in (x, onehot, lab))
        epsd = [torch.from_numpy(e).to(dev) for e in eps]
        s_native = net.forward(xd, od, training=True, eps=epsd)
        loss0 = float(net.loss(ld))
        torch.set_num_threads(min(16, torch.get_num_threads()))
        args = (torch.from_numpy(x), torch.from_numpy(onehot), [torch.from_numpy(e) for e in eps])
        RG.CONV_OPERAND_ROUNDING = routed
        try:
            out_r = R3.phiseg3d_forward(G.leaves(sd0), *args)
            total_r, _ = R3.phiseg3d_loss(out_r, torch.from_numpy(lab), num_classes=K)
        finally:
            RG.CONV_OPERAND_ROUNDING = None
        out_f = R3.phiseg3d_forward(G.leaves(sd0), *args)
        total_f, _ = R3.phiseg3d_loss(out_f, torch.from_numpy(lab), num_classes=K)
        assert abs(loss0 - float(total_r)) <= 2e-4 * abs(float(total_r)), (loss0, float(total_r))
        dev_fp32 = abs(loss0 - float(total_f)) / abs(float(total_f))
        assert 1e-7 < dev_fp32 < 2e-2, dev_fp32
        net.enable_graphs(True)
        opt = FusedAdam(net, lr=1e-3, weight_decay=1e-5)
        losses = []
        for _ in range(4):
            net.forward(xd, od, training=True, eps=epsd)
            l = net.loss(ld)
            opt.zero_grad(); l.backward(); opt.step()
            losses.append(float(l))
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    finally:
        L.uz_set_conv_math(-1)


@pytest.mark.gpu
def test_baseline_config5_full_volume_in_bf16_mode():
    """BASELINE.json configs[4] as it is quoted - bf16 - AT ITS REAL SIZE (the bf16 mode was only run at 64 x 64 x 32):
    PHISeg3D 5 / 5 levels, filters 32-64-128-192-192, 4 x 128 x 128 x 64, uz_set_conv_math(3) (one bf16 piece per operand, one MFMA
    product, fp32 accumulation; storage stays fp32 - DESIGN.md section 8).  The CPU oracle needs minutes for this volume, so the
    reference point is the SAME network through the fp32-accurate split mode on the device (that path is pinned against the oracle
    on the 64 x 64 x 32 sub-volume above): first-step loss within 2 % (the price of bf16 arithmetic, measured at 64 x 64 x 32
    against the oracle: < 2 %), level logits within 5 % of their range, and three replayed training steps finite and decreasing."""
    from unet_zoo_amd import _ffi
    from unet_zoo_amd.models.phiseg3D import PHISeg3D, phiseg3d_spec
    from unet_zoo_amd.optim import FusedAdam
    L = _ffi.lib()
    if L.uz_get_conv_math() == 0:
        pytest.skip("fp32-only run")
    dev = torch.device("cuda", 0)
    filters, K, Cin, dhw = [32, 64, 128, 192, 192], 3, 4, (128, 128, 64)
    sd0 = oracle.deterministic_state_dict(phiseg3d_spec(Cin, K, filters, 5), seed=11)
    shapes = R3.phiseg3d_eps_shapes(*dhw, 5, 5)
    x, onehot, lab, eps = R3.synthetic_volume(Cin, K, dhw, 9, shapes + shapes)
    xd, od, ld = (torch.from_numpy(a).to(dev) for a in (x, onehot, lab))
    epsd = [torch.from_numpy(e).to(dev) for e in eps]
    res = {}
    try:
        for mode in (1, 3):
            L.uz_set_conv_math(mode)
            net = PHISeg3D(Cin, K, filters, latent_levels=5, image_size=(Cin, *dhw))
            net.load_state_dict(sd0)
            net.train()
            s = net.forward(xd, od, training=True, eps=epsd)
            res[mode] = (float(net.loss(ld)), [t.clone() for t in s])
            if mode == 3:
                n_bf16 = sum(1 for o in net._cur.fwd_ops if o["code"] == "UZ_OP_CONV_FWD" and o.i("ks") == 3 and
                             L.uz_conv_route(0, *o.i("cin", "cout", "N", "H", "W"), 3) == 1)
                assert n_bf16 >= 20                                   # the volume's 3 x 3 x 3 convolutions really run on the one-piece kernels
                net.enable_graphs(True)
                opt = FusedAdam(net, lr=1e-3, weight_decay=1e-5)
                losses = []
                for _ in range(4):
                    net.forward(xd, od, training=True, eps=epsd)
                    l = net.loss(ld)
                    opt.zero_grad(); l.backward(); opt.step()
                    losses.append(float(l))
                assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
            del net
            torch.cuda.empty_cache()
    finally:
        L.uz_set_conv_math(-1)
    (l_ref, s_ref), (l_bf, s_bf) = res[1], res[3]
    rel = abs(l_bf - l_ref) / abs(l_ref)
    print(f"config 5 at full size: loss fp32-accurate split {l_ref:.6g}, bf16 arithmetic {l_bf:.6g} (rel {rel:.2e})")
    assert 1e-8 < rel < 2e-2, (l_ref, l_bf)
    for a, b in zip(s_ref, s_bf):
        rng = float(a.max() - a.min())
        assert float((a - b).abs().max()) <= 5e-2 * max(rng, 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "bf16_storage"])
def test_baseline_config5_full_volume_vs_the_reference_digest(mode, monkeypatch):
    """BASELINE.json configs[4] at its LITERAL size (4 x 128 x 128 x 64, filters 32 / 64 / 128 / 192 / 192) against the REAL reference
    (VERDICT r4 P4): tests/golden/phiseg3d_full_digest holds what the reference's own Posterior / prior / Likelihood modules and loss
    compute in fp32 on the CPU for the weights and the volume this test regenerates from the same seeds (tools/gen_golden.py 3d_full:
    losses, 2 048 sampled entries + max / norm / mean of every level's logits, s_in, mu, sigma, and of every parameter gradient).
    `split` = the fp32-accurate arithmetic: the north-star gate (1e-4 of the tensor's magnitude on every sampled activation, loss to
    5e-5, gradients to 1e-2 of their largest entry like the 2-D headline test).  `bf16_storage` = the configuration as BASELINE words
    it (bf16 arithmetic AND storage): what bf16 can hold - sampled activations within 8 % of the tensor's magnitude (measured 5 %), loss within
    2e-3, gradient norms within 25 % (measured 13 %: a BatchNorm scale of the first block), their median within 3 %."""
    from unet_zoo_amd import _ffi
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    L_ = _ffi.lib()
    if L_.uz_get_conv_math() == 0 and mode != "split":
        pytest.skip("fp32-only run")
    arrays, meta = G.load("phiseg3d_full_digest")
    dev = torch.device("cuda", 0)
    filters, K, Cin, dhw, L = meta["filters"], meta["num_classes"], meta["input_channels"], tuple(meta["dhw"]), meta["latent_levels"]
    sd0 = oracle.deterministic_state_dict(G.spec_of(meta), seed=meta["weight_seed"])
    shapes = R3.phiseg3d_eps_shapes(*dhw, len(filters), L)
    x, onehot, lab, eps = R3.synthetic_volume(Cin, K, dhw, meta["volume_seed"], shapes + shapes)
    try:
        if mode == "bf16_storage":
            L_.uz_set_conv_math(3)
            monkeypatch.setenv("UZ_STORE_B16", "1")
        net = PHISeg3D(Cin, K, filters, latent_levels=L, image_size=(Cin, *dhw))
        net.load_state_dict(sd0)
        net.train()
        s = net.forward(torch.from_numpy(x).to(dev), torch.from_numpy(onehot).to(dev), training=True, eps=[torch.from_numpy(e).to(dev) for e in eps])
        loss = net.loss(torch.from_numpy(lab).to(dev))
        ref_loss = float(arrays["loss"])
        exact = mode == "split"
        assert abs(float(loss) - ref_loss) <= (5e-5 if exact else 2e-3) * abs(ref_loss), (float(loss), ref_loss)
        worst = 0.0
        for l in range(L):
            for got_t, key in ((s[l], f"s{l}"), (net.s_in_list[l], f"s_in{l}"), (net.posterior_mu[l], f"post_mu{l}"), (net.posterior_sigma[l], f"post_sigma{l}"),
                               (net.prior_mu[l], f"prior_mu{l}"), (net.prior_sigma[l], f"prior_sigma{l}")):
                idx, ref, mom = arrays["i:" + key], arrays["v:" + key], arrays["m:" + key]
                got = got_t.float().reshape(-1)[torch.from_numpy(idx).to(dev)].cpu().numpy()
                scale = max(1.0, float(mom[0]))                 # the tensor's largest magnitude in the reference run
                err = float(np.abs(got - ref).max()) / scale
                worst = max(worst, err)
                assert err <= (1e-4 if exact else 8e-2), (key, err)        # (bf16: measured worst 5.0e-2 - the deepest level's prior mean)
        loss.backward()
        noise = G.bn_shadowed_biases([k for k, _, _ in meta["spec"]])
        n, worst_g, wk, devs = 0, 0.0, None, []
        for k, p_ in net.named_parameters():
            if ("v:g:" + k) not in arrays:
                assert p_.grad is None or k in meta["no_grad"] or float(p_.grad.abs().max()) == 0.0, k
                continue
            if k in noise:
                continue
            idx, ref, mom = arrays["i:g:" + k], arrays["v:g:" + k], arrays["m:g:" + k]
            g_ = p_.grad.float()
            got = g_.reshape(-1)[torch.from_numpy(idx).to(dev)].cpu().numpy()
            if exact:
                err = float(np.abs(got - ref).max()) / (float(mom[0]) + 1e-30)
            else:
                err = abs(float(g_.double().norm()) - float(mom[1])) / (float(mom[1]) + 1e-30)
            n += 1
            devs.append(err)
            if err > worst_g:
                worst_g, wk = err, k
        med = sorted(devs)[len(devs) // 2]
        print(f"config 5 at full size, {mode}: loss rel {abs(float(loss) - ref_loss) / abs(ref_loss):.1e}, worst activation sample {worst:.1e}, "
              f"worst gradient {'sample' if exact else 'norm'} deviation {worst_g:.1e} at {wk} (median {med:.1e}) over {n} tensors")
        # (bf16: per-tensor gradient NORMS against the fp32 reference - BatchNorm scale gradients are sums with heavy cancellation and
        #  move by up to 13 % in bf16 arithmetic, the median tensor by under 1 %)
        assert n > 100 and worst_g <= (1e-2 if exact else 2.5e-1) and med <= (2e-3 if exact else 3e-2), (worst_g, wk, med)
    finally:
        L_.uz_set_conv_math(-1)


@pytest.mark.gpu
def test_baseline_config5_full_volume_in_bf16_storage(monkeypatch):
    """BASELINE.json configs[4] LITERALLY - bf16 arithmetic AND bf16 storage, 4 x 128 x 128 x 64: with UZ_STORE_B16=1
    the plan keeps the volume's large tensors (activations, their gradients, every unit's dy on the 128 x 64 and 64 x 32 planes) as
    2-byte bf16 elements (Plan._b16_pass; the kernels are pinned per op, by equalities, in tests/test_b16_storage_gpu.py).
    Reference points on the device: the same network with fp32 storage in the same arithmetic, and in the fp32-accurate split mode
    (pinned against the CPU oracle on the 64 x 64 x 32 sub-volume above).  Gates: first-step loss within 1e-3 of both (measured 1e-5 /
    4e-5), level logits within 5 % of their range of the split mode's (measured 2.4 %; fp32 storage: 2.0 %), > 7 GB of tensors in bf16
    and a third less arena, three replayed training steps finite and decreasing."""
    from unet_zoo_amd import _ffi
    from unet_zoo_amd.models.phiseg3D import PHISeg3D, phiseg3d_spec
    from unet_zoo_amd.optim import FusedAdam
    L = _ffi.lib()
    if L.uz_get_conv_math() == 0:
        pytest.skip("fp32-only run")
    dev = torch.device("cuda", 0)
    filters, K, Cin, dhw = [32, 64, 128, 192, 192], 3, 4, (128, 128, 64)
    sd0 = oracle.deterministic_state_dict(phiseg3d_spec(Cin, K, filters, 5), seed=11)
    shapes = R3.phiseg3d_eps_shapes(*dhw, 5, 5)
    x, onehot, lab, eps = R3.synthetic_volume(Cin, K, dhw, 9, shapes + shapes)
    xd, od, ld = (torch.from_numpy(a).to(dev) for a in (x, onehot, lab))
    epsd = [torch.from_numpy(e).to(dev) for e in eps]
    res = {}
    try:
        for tag, mode, b16 in (("split", 1, "0"), ("f32 storage", 3, "0"), ("bf16 storage", 3, "1")):
            L.uz_set_conv_math(mode)
            monkeypatch.setenv("UZ_STORE_B16", b16)
            net = PHISeg3D(Cin, K, filters, latent_levels=5, image_size=(Cin, *dhw))
            net.load_state_dict(sd0)
            net.train()
            s = net.forward(xd, od, training=True, eps=epsd)
            res[tag] = (float(net.loss(ld)), [t.float().clone() for t in s], net._cur.arena_floats)
            info = net._cur.b16_info
            if tag == "bf16 storage":
                assert info["buffers"] >= 60 and info["grads"] >= 30 and info["dy"] >= 30 and info["bytes_saved"] >= 7e9, info
                from unet_zoo_amd._plan import View
                stored = [b for b in net._cur.bufs if b.b16]
                t16 = net._cur.tensor(View(stored[0]))
                assert t16.dtype == torch.bfloat16 and bool(torch.isfinite(t16.float()).all())
                net.enable_graphs(True)
                opt = FusedAdam(net, lr=1e-3, weight_decay=1e-5)
                losses = []
                for _ in range(4):
                    net.forward(xd, od, training=True, eps=epsd)
                    l = net.loss(ld)
                    opt.zero_grad(); l.backward(); opt.step()
                    losses.append(float(l))
                assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
                assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
            else:
                assert info["buffers"] == 0 and info["ops"] == 0
            del net
            torch.cuda.empty_cache()
    finally:
        L.uz_set_conv_math(-1)
    l_split, s_split, _ = res["split"]
    l_f32, s_f32, a_f32 = res["f32 storage"]
    l_b16, s_b16, a_b16 = res["bf16 storage"]
    print(f"config 5, bf16 storage: loss {l_b16:.7g} (fp32 storage {l_f32:.7g}, split {l_split:.7g}); arena {4 * a_b16 / 1e9:.2f} GB vs {4 * a_f32 / 1e9:.2f} GB")
    assert abs(l_b16 - l_f32) <= 1e-3 * abs(l_f32) and abs(l_b16 - l_split) <= 1e-3 * abs(l_split)
    assert a_b16 <= 0.67 * a_f32
    for a, b in zip(s_split, s_b16):
        rng = float(a.max() - a.min())
        assert float((a - b).abs().max()) <= 5e-2 * max(rng, 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_bf16_mode_against_the_reference_modules_run_in_bf16(storage, monkeypatch):
    """tests/golden/phiseg3d_bf16.*: the reference's Posterior / prior / Likelihood modules run under
    torch.autocast('cpu', torch.bfloat16) (and in fp32) on a 32 x 64 x 64 volume, filters 32-32-64 - large enough that the
    library routes the 3x3x3 layers to the matrix-pipe kernels (tools/gen_golden.py 3d_bf16; every 7th element stored).
    Gate (stated): the reference's own bf16 run differs from its fp32 run by up to 3 % of a tensor's range (it also rounds every
    convolution OUTPUT to bf16: measured 3.6 %); the native bf16 arithmetic mode keeps outputs in fp32, so it must be CLOSER to the
    reference's fp32 tensors than the reference's own bf16 run is (measured 2.1 %), and - two independent bf16 perturbations of one
    fp32 result - within 6 % of the reference's bf16 tensors (measured 4.6 %); loss within 1e-3 of both."""
    from unet_zoo_amd import _ffi
    from oracle.refgraph3d import phiseg3d_eps_shapes, synthetic_volume
    arrays, meta = G.load("phiseg3d_bf16")
    L, Lv = _ffi.lib(), meta["latent_levels"]
    D, H, W = meta["dhw"]
    shapes = phiseg3d_eps_shapes(D, H, W, len(meta["filters"]), Lv)
    x, onehot, lab, eps = synthetic_volume(meta["input_channels"], meta["num_classes"], (D, H, W), meta["input_seed"], shapes + shapes)
    inputs = dict(patch=x, mask_onehot=onehot, labels=lab, **{f"eps{k}": e for k, e in enumerate(eps)})
    # storage == "bf16": the full-resolution tensors of this volume are also STORED in bf16 (UZ_STORE_B16=1, Plan._b16_pass) - what the
    # reference's autocast run does with every convolution output; the gates below are the same for both storages
    monkeypatch.setenv("UZ_STORE_B16", "1" if storage == "bf16" else "0")
    try:
        L.uz_set_conv_math(3)
        net, s, loss = _run_native(meta, inputs)
        assert (net._cur.b16_info["buffers"] >= 10) == (storage == "bf16"), net._cur.b16_info
        n_bf16 = sum(1 for o in net._cur.fwd_ops if o["code"] == "UZ_OP_CONV_FWD" and o.i("ks") == 3 and
                     L.uz_conv_route(0, *o.i("cin", "cout", "N", "H", "W"), 3) == 1)
        assert n_bf16 >= 10, n_bf16                                   # the mode is really exercised
    finally:
        L.uz_set_conv_math(-1)
    st = meta["logit_stride"]
    worst_vs_bf16 = worst_vs_f32 = ref_gap = 0.0
    for l in range(Lv):
        for attr, key in ((net.posterior_mu, "post_mu"), (net.posterior_sigma, "post_sigma"), (net.prior_mu, "prior_mu"),
                          (net.prior_sigma, "prior_sigma"), (net.s_in_list, "s_in")):
            got = attr[l].cpu().numpy().reshape(-1)[::st]
            rb, rf = arrays[f"bf16:{key}{l}"], arrays[f"fp32:{key}{l}"]
            rng = float(np.abs(rf).max())
            worst_vs_bf16 = max(worst_vs_bf16, G.maxabs(got, rb) / rng)
            worst_vs_f32 = max(worst_vs_f32, G.maxabs(got, rf) / rng)
            ref_gap = max(ref_gap, G.maxabs(rb, rf) / rng)
    print(f"native bf16 mode ({storage} storage) vs reference-bf16 {worst_vs_bf16:.3e}, vs reference-fp32 {worst_vs_f32:.3e}; reference bf16 vs its fp32 {ref_gap:.3e}")
    assert worst_vs_bf16 <= 6e-2 and worst_vs_f32 <= ref_gap
    lf, lb = float(arrays["fp32:loss"]), float(arrays["bf16:loss"])
    assert abs(float(loss) - lf) <= 1e-3 * abs(lf) and abs(float(loss) - lb) <= 1e-3 * abs(lb), (float(loss), lf, lb)
