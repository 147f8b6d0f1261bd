"""Mask-free inference on the device: the two kernels of csrc/predict.hip at their dispatch edges against torch / fp64, and
PHISeg.predict against the CPU oracle, against forward() on the repeated patch, and against the numpy twin of uz_sample_stats
on its own level logits.  Gates: level logits 1e-4 against the oracle (the project's logit gate), 2e-4 between two device paths
that each carry 1e-4; softmax 1e-6 (test_accumulate_softmax_argmax); the rest is derived in tests/_predict.py."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import oracle
from oracle import refgraph as R
from tests import _golden as G
from tests import _nets as N
from tests import _predict as P

pytestmark = pytest.mark.gpu

FILTERS = [4, 8, 8, 8, 8, 8, 8]
SHAPES = [(1, 4, 64, 64), (3, 2, 64, 64), (2, 3, 64, 128)]                         # (B, S, H, W): 64 puts the deepest plane at 1 x 1
LOGIT_TOL = 1e-4                                                                   # no existing PHiSeg test widens it for a forced-split run


def _g():
    from tests import _gpu
    return _gpu


# ------------------------------------------------------------------------------------------ op level: uz_batch_repeat_fwd
CANARY = -777.0


def _repeat_case(g, B, S, H, W, xs, ys, shift=0):
    """One call on C-channel slices of wider buffers whose other channels hold a canary; shift = floats the buffers start off
    a 16-byte boundary."""
    C = P.REPEAT_C
    (ctx, ox), (cty, oy) = xs, ys
    x = g.rnd(B, C, H, W, seed=B * 100 + S * 10 + H)
    xraw = torch.full((B * ctx * H * W + shift,), CANARY, device=g.dev())
    yraw = torch.full((S * B * cty * H * W + shift,), CANARY, device=g.dev())
    xb, yb = xraw[shift:].view(B, ctx, H, W), yraw[shift:].view(S * B, cty, H, W)
    xb[:, ox:ox + C] = x.to(g.dev())
    g.call("uz_batch_repeat_fwd", xb[:, ox:], C, ctx, yb[:, oy:], cty, B, S, H, W)
    want = torch.full((S * B, cty, H, W), CANARY)
    want[:, oy:oy + C] = x.repeat(S, 1, 1, 1)
    assert torch.equal(yb.cpu(), want), (B, S, H, W, xs, ys, shift)                 # the slice bit for bit, the guard channels untouched
    assert torch.equal(xb[:, ox:ox + C].cpu(), x) and float(yraw[:shift].sum()) == CANARY * shift


@pytest.mark.parametrize("H,W", P.REPEAT_PLANES)
def test_batch_repeat_is_patch_repeat_into_a_slice(H, W):
    g = _g()
    for B, S in P.REPEAT_BS:
        for xs in P.REPEAT_SIDES:
            for ys in P.REPEAT_SIDES:
                _repeat_case(g, B, S, H, W, xs, ys)


def test_batch_repeat_takes_the_scalar_path_for_unaligned_slices_of_float4_planes():
    g = _g()
    for shift in (1, 2):
        _repeat_case(g, 3, 2, 4, 4, (13, 3), (13, 3), shift=shift)
        _repeat_case(g, 1, 5, 32, 32, (8, 0), (13, 0), shift=shift)


def test_batch_repeat_rejects_bad_sizes():
    from unet_zoo_amd import _ffi
    g = _g()
    t = torch.zeros(64, device=g.dev())
    for args in ((t, 0, 1, t, 1, 1, 1, 1, 1), (t, 2, 1, t, 2, 1, 1, 1, 1), (t, 1, 1, t, 1, 1, 0, 1, 1), (None, 1, 1, t, 1, 1, 1, 1, 1)):
        with pytest.raises(_ffi.UzError):
            g.call("uz_batch_repeat_fwd", *args)


# ------------------------------------------------------------------------------------------ op level: uz_sample_stats
def _stats_call(g, lv_dev, K, B, S, H, W, soft=True, labels=True, mean_label=True, entropy=True):
    dev = g.dev()
    tab = torch.tensor([t.data_ptr() for t in lv_dev], dtype=torch.int64, device=dev)
    out = dict(soft=torch.full((S * B, K, H, W), CANARY, device=dev) if soft else None,
               labels=torch.full((S * B, H, W), 255, dtype=torch.uint8, device=dev) if labels else None,
               mean_soft=torch.full((B, K, H, W), CANARY, device=dev),
               mean_label=torch.full((B, H, W), 255, dtype=torch.uint8, device=dev) if mean_label else None,
               entropy=torch.full((B, H, W), CANARY, device=dev) if entropy else None)
    g.call("uz_sample_stats", tab, len(lv_dev), K, B, S, H, W, out["soft"], out["labels"], out["mean_soft"], out["mean_label"], out["entropy"])
    return out


@pytest.mark.parametrize("K", P.STATS_K)
@pytest.mark.parametrize("L", P.STATS_L)
def test_sample_stats_vs_fp64(K, L):
    """Entropy gate: an fp32 torch-CPU evaluation of the same formula is within 3.67e-7 of fp64 on these inputs (measured,
    tests/test_predict_cpu.py asserts it); the device's exp / log are not libm's: 4 x the recorded 3.7e-7 = 1.48e-6."""
    g = _g()
    for B, S, H, W in P.stats_cases(K, L):
        levels, ref = P.stats_case(K, L, B, S, H, W)
        lv_dev = [torch.from_numpy(lv.copy()).to(g.dev()) for lv in levels]
        got = _stats_call(g, lv_dev, K, B, S, H, W)
        case = (K, L, B, S, H, W)
        e_soft, e_mean = G.maxabs(got["soft"].cpu().numpy(), ref["soft"]), G.maxabs(got["mean_soft"].cpu().numpy(), ref["mean_soft"])
        e_ent = G.maxabs(got["entropy"].cpu().numpy(), ref["entropy"])
        print(f"sample_stats {case}: soft {e_soft:.2e} mean_soft {e_mean:.2e} entropy {e_ent:.2e}")
        assert np.array_equal(got["labels"].cpu().numpy(), ref["labels"]), case     # everywhere: the inputs make sums and ties exact
        assert np.array_equal(got["mean_label"].cpu().numpy(), ref["mean_label"]), case
        assert e_soft <= P.SOFT_TOL, case
        assert e_mean <= P.mean_soft_tol(S), case
        assert e_ent <= P.ENTROPY_TOL, case
        for lv, t in zip(levels, lv_dev):
            assert np.array_equal(t.cpu().numpy(), lv), case                        # the logits are read, never accumulated into
        again = _stats_call(g, lv_dev, K, B, S, H, W)
        assert all(torch.equal(got[k], again[k]) for k in got), case
        for drop in ("soft", "labels", "mean_label", "entropy"):                    # a null output leaves the others what they were
            part = _stats_call(g, lv_dev, K, B, S, H, W, **{drop: False})
            assert part[drop] is None and all(torch.equal(got[k], part[k]) for k in got if k != drop), (case, drop)
        bare = _stats_call(g, lv_dev, K, B, S, H, W, soft=False, labels=False, mean_label=False, entropy=False)
        assert torch.equal(bare["mean_soft"], got["mean_soft"]), case


def test_sample_stats_ties_zero_probabilities_and_class_limits():
    from unet_zoo_amd import _ffi
    g = _g()
    lv = [torch.tensor([[[[1.0]], [[2.5]], [[2.5]], [[-1.0]]]], device=g.dev())]
    got = _stats_call(g, lv, 4, 1, 1, 1, 1)
    assert int(got["labels"]) == 1 and int(got["mean_label"]) == 1                  # first maximum wins
    for big in (60.0, 500.0):                                                       # a mean probability of 7.7e-53, and of 0 exactly
        lv = [torch.tensor([[[[big]], [[-big]]]], device=g.dev())]
        got = _stats_call(g, lv, 2, 1, 1, 1, 1)
        assert torch.isfinite(got["entropy"]).all() and float(got["entropy"].abs().max()) <= 1e-30
        assert got["mean_soft"].flatten().tolist() == [1.0, 0.0] and int(got["mean_label"]) == 0
    t = torch.zeros(9, 1, 1, device=g.dev())
    for K in (0, 9):
        with pytest.raises(_ffi.UzError):
            _stats_call(g, [t.view(1, 9, 1, 1)], K, 1, 1, 1, 1)


# ------------------------------------------------------------------------------------------ model level
def _state(seed=91):
    from unet_zoo_amd.models.phiseg import phiseg_spec
    return N.off_identity_state(phiseg_spec(1, 2, FILTERS), seed)


def _net(sd=None, graphs=False):
    from unet_zoo_amd.models.phiseg import PHISeg
    net = PHISeg(1, 2, FILTERS, image_size=(1, 64, 64))
    res = net.load_state_dict(sd if sd is not None else _state())
    assert not res.missing_keys and not res.unexpected_keys
    net.eval()
    net.enable_graphs(graphs)
    return net


@functools.lru_cache(maxsize=None)
def _case(B, S, H, W):
    """Inputs, the CPU oracle's answer and one predict() of a fresh net, shared by the tests of this shape (read-only)."""
    dev = torch.device("cuda", 0)
    sd = _state()
    shapes = oracle.phiseg_eps_shapes(B * S, H, W)
    x, mask, eps = oracle.synthetic_batch(B * S, H, W, seed=40 + B + S + W, eps_shapes=shapes + shapes)
    patch = torch.from_numpy(x[:B])
    e = [torch.from_numpy(a) for a in eps]
    lv = G.leaves(sd)
    with torch.no_grad():
        z, mu, sigma = R._phiseg_encoder(lv, "prior", patch.repeat(S, 1, 1, 1), e[5:], False)
        s = R._phiseg_likelihood(lv, z, (H, W), False)
    net = _net(sd)
    with torch.no_grad():
        out = net.predict(patch.to(dev), n_samples=S, eps=[t.to(dev) for t in e[5:]], return_soft=True)
    torch.cuda.synchronize()
    keep = types.SimpleNamespace(labels=out.labels.clone(), mean_soft=out.mean_soft.clone(), mean_label=out.mean_label.clone(),
                                 entropy=out.entropy.clone(), soft=out.soft.clone(), levels=[t.clone() for t in out.levels],
                                 mu=[t.clone() for t in net.prior_mu], sigma=[t.clone() for t in net.prior_sigma],
                                 z=[t.clone() for t in net.prior_latent_space], bounds=net.check_bounds())
    return types.SimpleNamespace(sd=sd, patch=patch, mask=torch.from_numpy(mask), eps=e, ref=dict(s=s, mu=mu, sigma=sigma, z=z), out=keep, net=net)


def _check_wiring(out, B, S, K=2):
    """labels / mean_soft / mean_label / entropy = uz_sample_stats's twin on predict's OWN level logits: the wiring, not the arithmetic."""
    tw = P.sample_stats_twin([t.cpu().numpy() for t in out.levels], B, S)
    H, W = out.levels[0].shape[-2:]
    assert out.labels.shape == (S, B, H, W) and out.labels.dtype == torch.uint8
    assert out.mean_soft.shape == (B, K, H, W) and out.mean_label.shape == (B, H, W) and out.entropy.shape == (B, H, W)
    assert np.array_equal(out.labels.cpu().numpy().reshape(S * B, H, W), tw["labels"])
    assert np.array_equal(out.mean_label.cpu().numpy(), tw["mean_label"])
    assert G.maxabs(out.mean_soft.cpu().numpy(), tw["mean_soft"]) <= P.mean_soft_tol(S)
    assert G.maxabs(out.entropy.cpu().numpy(), tw["entropy"]) <= P.ENTROPY_TOL
    if out.soft is not None:
        assert out.soft.shape == (S, B, K, H, W)
        assert G.maxabs(out.soft.cpu().numpy().reshape(S * B, K, H, W), tw["soft"]) <= P.SOFT_TOL


@pytest.mark.parametrize("B,S,H,W", SHAPES)
def test_predict_model_vs_cpu_oracle(B, S, H, W):
    c = _case(B, S, H, W)
    assert c.out.bounds == 0
    for l in range(5):
        errs = [G.maxabs(got[l].cpu().numpy(), c.ref[k][l].numpy()) for got, k in ((c.out.levels, "s"), (c.out.mu, "mu"), (c.out.sigma, "sigma"), (c.out.z, "z"))]
        print(f"predict {(B, S, H, W)} level {l}: logits {errs[0]:.2e} mu {errs[1]:.2e} sigma {errs[2]:.2e} z {errs[3]:.2e}")
        assert c.out.levels[l].shape == (S * B, 2, H, W)
        assert errs[0] <= LOGIT_TOL and errs[1] <= 1e-4 and errs[2] <= 1e-4 and errs[3] <= 1e-4, (l, errs)
    _check_wiring(c.out, B, S)


@pytest.mark.parametrize("B,S,H,W", SHAPES)
def test_predict_model_vs_forward_on_the_repeated_patch(B, S, H, W):
    """The parent commit's way: forward(patch.repeat(S, 1, 1, 1), some mask, training=False) - whose prior half must not depend on the mask."""
    c = _case(B, S, H, W)
    dev = torch.device("cuda", 0)
    net = _net(c.sd)
    eps = [t.to(dev) for t in c.eps]                                                # 5 arbitrary posterior draws + the prior's
    rep = c.patch.to(dev).repeat(S, 1, 1, 1)
    runs = []
    for mask in (c.mask.to(dev), 1.0 - c.mask.to(dev)):
        with torch.no_grad():
            runs.append([t.clone() for t in net.forward(rep, mask, training=False, eps=eps)])
    assert net.check_bounds() == 0
    for l in range(5):
        assert torch.equal(runs[0][l], runs[1][l]), l
        e = G.maxabs(runs[0][l].cpu().numpy(), c.out.levels[l].cpu().numpy())
        print(f"predict vs forward {(B, S, H, W)} level {l}: {e:.2e}")
        assert e <= 2e-4, (l, e)


@pytest.mark.parametrize("B,S,H,W", SHAPES)
def test_predict_model_gives_every_sample_of_an_image_the_same_trunk(B, S, H, W):
    """The same noise on every sample row of an image: the rows must then be equal bit for bit."""
    c = _case(B, S, H, W)
    dev = torch.device("cuda", 0)
    eps = [t[:B].repeat(S, 1, 1, 1).to(dev) for t in c.eps[5:]]
    with torch.no_grad():
        out = c.net.predict(c.patch.to(dev), n_samples=S, eps=eps)
    for lvl in out.levels:
        rows = lvl.reshape(S, B, *lvl.shape[1:])
        for s in range(1, S):
            assert torch.equal(rows[s], rows[0]), s
    assert torch.equal(out.labels[1:], out.labels[:1].expand(S - 1, -1, -1, -1)) and out.soft is None
    assert c.net.check_bounds() == 0
    _check_wiring(out, B, S)


@pytest.mark.parametrize("graphs", [False, True])
def test_predict_model_is_repeatable_and_replays(graphs):
    """Twice the same eps -> the same bits, eager and under enable_graphs(True) (lane replay, or hipGraph: eager, capture, replay),
    and both equal to the shared eager run; the cached plans are reused."""
    B, S, H, W = SHAPES[1]
    c = _case(B, S, H, W)
    dev = torch.device("cuda", 0)
    net = _net(c.sd, graphs=graphs)
    eps = [t.to(dev) for t in c.eps[5:]]
    for _ in range(4):
        with torch.no_grad():
            out = net.predict(c.patch.to(dev), n_samples=S, eps=eps)
        assert net.check_bounds() == 0
        assert all(torch.equal(a, b) for a, b in zip(out.levels, c.out.levels))
        assert torch.equal(out.labels, c.out.labels) and torch.equal(out.mean_soft, c.out.mean_soft)
        assert torch.equal(out.mean_label, c.out.mean_label) and torch.equal(out.entropy, c.out.entropy)
    _check_wiring(out, B, S)
    assert sorted(k[0] for k in net._plans) == ["draw", "trunk"]


def test_predict_model_draws_its_own_noise():
    B, S, H, W = SHAPES[0]
    c = _case(B, S, H, W)
    dev = torch.device("cuda", 0)
    net = _net(c.sd)
    with torch.no_grad():
        a = net.predict(c.patch.to(dev), n_samples=S)
        la, ma = [t.clone() for t in a.levels], a.mean_soft.clone()
        b = net.predict(c.patch.to(dev), n_samples=S)
    assert net.check_bounds() == 0
    assert not torch.equal(la[0], b.levels[0]) and not torch.equal(ma, b.mean_soft)
    rows = b.levels[0].reshape(S, B, *b.levels[0].shape[1:])
    assert all(not torch.equal(rows[s], rows[0]) for s in range(1, S))
    assert len(net.prior_mu) == 5 and net.prior_mu[0].shape == (S * B, 2, H // 4, W // 4) and net.prior_latent_space[4].shape == (S * B, 2, 1, 1)
    _check_wiring(b, B, S)


def test_predict_model_errors():
    dev = torch.device("cuda", 0)
    net = _net()
    x = torch.zeros(1, 1, 64, 64, device=dev)
    with pytest.raises(ValueError):
        net.predict(torch.zeros(1, 1, 96, 96, device=dev))
    with pytest.raises(ValueError):
        net.predict(x, n_samples=0)
    net.train()
    with pytest.raises(RuntimeError):
        net.predict(x)
    from unet_zoo_amd.models.phiseg import PHISeg
    rev = PHISeg(1, 2, FILTERS, image_size=(1, 64, 64), reversible=True)
    rev.eval()
    with pytest.raises(NotImplementedError):
        rev.predict(x)


def test_predict_model_leaves_training_what_it_was():
    """forward + loss + backward in train mode behind a predict(): the loss and the gradients of a fresh model with the same state."""
    B, S, H, W = SHAPES[1]
    c = _case(B, S, H, W)
    dev = torch.device("cuda", 0)
    x, m = c.patch.to(dev).repeat(S, 1, 1, 1), c.mask.to(dev)
    eps = [t.to(dev) for t in c.eps]
    got = []
    for first_predict in (True, False):
        net = _net(c.sd)
        if first_predict:
            with torch.no_grad():
                net.predict(c.patch.to(dev), n_samples=S)
            assert all(torch.equal(v.cpu(), c.sd[k]) for k, v in net.state_dict().items())      # running statistics, counters: untouched
        net.train()
        net.forward(x, m, training=True, eps=eps)
        loss = net.loss(m)
        loss.backward()
        got.append((float(loss.detach()), net._ptab.gflat.clone()))
    assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1])


def test_harness_predict_is_the_nets_predict(tmp_path):
    from unet_zoo_amd import train_model as TM
    from unet_zoo_amd.models import PHISeg, Unet
    cfg = types.SimpleNamespace(experiment_name="t", log_dir_name="t", filter_channels=FILTERS, latent_levels=5, n_classes=2, no_convs_fcomb=3,
                                beta=1.0, use_reversible=False, input_channels=1, image_size=(1, 64, 64), batch_size=2, iterations=2,
                                logging_frequency=2, model=PHISeg)
    h = TM.UNetModel(cfg, log_root=str(tmp_path))
    data = TM.SyntheticData(None, cfg, n_train=4, n_val=3)
    images = data.validation.images                                                 # (3, 64, 64) numpy
    h.net.train()
    h.net.set_rng_state(1234)
    a = h.predict(images, n_samples=2)
    assert not h.net.training
    keep = (a.labels.clone(), a.mean_soft.clone(), a.mean_label.clone(), a.entropy.clone(), [t.clone() for t in a.levels])
    h.net.set_rng_state(1234)
    with torch.no_grad():
        b = h.net.predict(torch.as_tensor(images, dtype=torch.float32).to(h.device).unsqueeze(1), n_samples=2)
    assert type(a) is type(b) and a.soft is None
    assert torch.equal(keep[0], b.labels) and torch.equal(keep[1], b.mean_soft) and torch.equal(keep[2], b.mean_label) and torch.equal(keep[3], b.entropy)
    assert all(torch.equal(p, q) for p, q in zip(keep[4], b.levels))
    _check_wiring(b, 3, 2)
    cfg_u = types.SimpleNamespace(**{**vars(cfg), "model": Unet, "filter_channels": [8, 16, 16, 16]})
    with pytest.raises(NotImplementedError):
        TM.UNetModel(cfg_u, log_root=str(tmp_path)).predict(images, n_samples=2)


@pytest.mark.parametrize("mode", ["f32", "split"])
def test_predict_model_in_the_other_arithmetic_modes(mode):
    """The model-level tests again with the convolutions forced onto the fp32-MFMA kernels and onto the split-fp16 kernels (the
    default mode is this process).  The switch is read once per process, hence the child process; the gates are the same."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, UZ_CONV_MATH=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_predict_gpu.py", "-q", "-x", "-m", "gpu", "-k", "predict_model and not arithmetic_modes"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
