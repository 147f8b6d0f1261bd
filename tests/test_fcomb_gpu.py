"""ProbabilisticUnet.predict on the device: uz_fcomb_sample_fwd (csrc/fcomb.hip) on the op-level cases of tests/_fcomb.py against
a direct fp64 evaluation, and predict() against the CPU oracle, against the device's own older route (forward, then one decode
tape per sample) and against the numpy twin of uz_sample_stats on its own logits.  Gates: z one rounded multiply-add; op-level
logits 4 x the recorded fp32 torch-CPU figure (5.4e-6, tests/_fcomb.py); model logits 1e-4 against the oracle (the project's logit
gate), 2e-4 between two device paths that each carry 1e-4; the statistics as tests/_predict.py derives them."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import _fcomb as F
from tests import _golden as G
from tests import _predict as P

pytestmark = pytest.mark.gpu

TAIL = 64                                                                           # canary floats behind every output


def _g():
    from tests import _gpu
    return _gpu


# ------------------------------------------------------------------------------------------ op level
def _dev(g, a, shift):
    """A device copy of `a` that starts `shift` floats behind a 16-byte boundary."""
    raw = torch.full((a.size + shift,), F.CANARY, device=g.dev())
    raw[shift:] = torch.from_numpy(np.array(a)).reshape(-1).to(g.dev())
    return raw[shift:]


def _run_case(g, c):
    d, ref = F.case_data(c)
    HW, N = c.H * c.W, c.S * c.B
    feat = np.full((c.B, c.Ctot, c.H, c.W), F.CANARY, np.float32)                    # the channels beyond 32 are not the kernel's
    feat[:, :F.FC] = d["feat"]
    feat_d = _dev(g, feat, c.shift)
    feat_0 = feat_d.clone()
    ops = [_dev(g, d[k], c.shift) for k in ("mu", "sigma", "eps")]
    par = [_dev(g, p[k], c.shift) for p in d["units"] for k in ("w", "b", "gamma", "beta", "rm", "rv")]
    par += [_dev(g, d["w_last"], c.shift), _dev(g, d["b_last"], c.shift)]
    tab = torch.tensor([t.data_ptr() for t in par], dtype=torch.int64, device=g.dev())
    zraw = torch.full((c.shift + N * c.L + TAIL,), F.CANARY, device=g.dev())
    lraw = torch.full((c.shift + N * c.K * HW + TAIL,), F.CANARY, device=g.dev())
    with F.forced_px(c.px):                                                         # 0: the route's own choice, the variable unset
        g.call("uz_fcomb_sample_fwd", feat_d, F.FC, c.Ctot, ops[0], ops[1], ops[2], tab, c.U, F.BN_EPS, c.L, c.K, c.B, c.S, c.H, c.W,
               zraw[c.shift:], lraw[c.shift:])
    z = zraw[c.shift:c.shift + N * c.L].cpu().numpy().reshape(N, c.L)
    logits = lraw[c.shift:c.shift + N * c.K * HW].cpu().numpy().reshape(N, c.K, c.H, c.W)
    key = F.case_id(c)
    for raw, n in ((zraw, N * c.L), (lraw, N * c.K * HW)):                           # nothing in front of or behind the outputs
        assert float(raw[:c.shift].sum()) == F.CANARY * c.shift and bool((raw[c.shift + n:] == F.CANARY).all()), key
    assert torch.equal(feat_d, feat_0), key                                         # the features, their extra channels included
    ez = float(np.max(np.abs(z.astype(np.float64) - ref.z) / F.z_tol(d, c)))
    el = G.maxabs(logits, ref.logits)
    print(f"fcomb {key} route {F.case_route(c)}: z {ez:.2f} of its gate, logits {el:.2e} (gate {F.LOGITS_TOL:.2e})")
    assert np.all(np.abs(z.astype(np.float64) - ref.z) <= F.z_tol(d, c)), key
    assert el <= F.LOGITS_TOL, (key, el)
    return zraw, lraw, (feat_d, ops, tab, par)


@pytest.mark.parametrize("H,W", F.PLANES)
def test_fcomb_sample_vs_fp64(H, W):
    """Every case of the plane, the forced-kernel ones included; the measured figures are in profiles/NOTES_predict.md."""
    g = _g()
    for c in F.cases(H, W):
        _run_case(g, c)


def test_fcomb_sample_is_bit_repeatable_on_either_kernel():
    g = _g()
    picked = [F.extra_case(e) for e in F.EXTRA if (e["S"], e["px"]) in ((1021, 0), (44, 0), (26, 0), (26, 1))] + [F.cases(64, 64)[1]]
    assert {F.case_route(c)[0] for c in picked} == {256, 512}
    for c in picked:
        a, b = _run_case(g, c), _run_case(g, c)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------ model level
def _net(sd, no_convs, graphs=False):
    from unet_zoo_amd.models.probabilistic_unet import ProbabilisticUnet
    net = ProbabilisticUnet(1, 2, F.FILTERS, latent_dim=F.LATENT, no_convs_fcomb=no_convs, image_size=(1, F.H0, F.H0))
    res = net.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    net.eval()
    net.enable_graphs(graphs)
    return net


@functools.lru_cache(maxsize=None)
def _case(no_convs, B, S, H, W):
    """The oracle's answer (tests/_fcomb.model_case) and one predict() of a fresh net with the same eps; shared, read-only."""
    m = F.model_case(no_convs, B, S, H, W)
    dev = torch.device("cuda", 0)
    net = _net(m.sd, no_convs)
    with torch.no_grad():
        out = net.predict(m.patch.to(dev), n_samples=S, eps=m.eps.to(dev), return_soft=True)
    torch.cuda.synchronize()
    keep = types.SimpleNamespace(labels=out.labels.clone(), mean_soft=out.mean_soft.clone(), mean_label=out.mean_label.clone(),
                                 entropy=out.entropy.clone(), soft=out.soft.clone(), levels=[t.clone() for t in out.levels],
                                 z=net.z_prior_sample.clone(), mu=net.prior_latent_space.mean.clone(), sigma=net.prior_latent_space.stddev.clone(),
                                 features=net.unet_features.clone(), bounds=net.check_bounds())
    return types.SimpleNamespace(m=m, out=keep, net=net)


def _check_wiring(out, B, S, K=2):
    """labels / mean_soft / mean_label / entropy = uz_sample_stats's twin on predict's OWN logits: the wiring, not the arithmetic."""
    assert len(out.levels) == 1
    lg = out.levels[0]
    H, W = lg.shape[-2:]
    assert lg.shape == (S * B, K, H, W)
    tw = P.sample_stats_twin([lg.cpu().numpy()], B, S)
    assert out.labels.shape == (S, B, H, W) and out.labels.dtype == torch.uint8
    assert out.mean_soft.shape == (B, K, H, W) and out.mean_label.shape == (B, H, W) and out.entropy.shape == (B, H, W)
    assert torch.equal(out.labels.reshape(S * B, H, W).long().cpu(), torch.argmax(lg, dim=1).cpu())     # exactly the argmax of the logits
    assert np.array_equal(out.labels.cpu().numpy().reshape(S * B, H, W), tw["labels"])
    assert np.array_equal(out.mean_label.cpu().numpy(), tw["mean_label"])
    assert G.maxabs(out.mean_soft.cpu().numpy(), tw["mean_soft"]) <= P.mean_soft_tol(S)
    assert G.maxabs(out.entropy.cpu().numpy(), tw["entropy"]) <= P.ENTROPY_TOL
    if out.soft is not None:
        assert out.soft.shape == (S, B, K, H, W)
        assert G.maxabs(out.soft.cpu().numpy().reshape(S * B, K, H, W), tw["soft"]) <= P.SOFT_TOL


@pytest.mark.parametrize("no_convs", F.NO_CONVS)
@pytest.mark.parametrize("B,S,H,W", F.SHAPES)
def test_predict_vs_cpu_oracle(no_convs, B, S, H, W):
    c = _case(no_convs, B, S, H, W)
    m, out = c.m, c.out
    assert out.bounds == 0
    e_l = G.maxabs(out.levels[0].cpu().numpy(), m.logits.numpy())
    e_mu, e_sg = G.maxabs(out.mu.cpu().numpy(), m.mu.numpy()), G.maxabs(out.sigma.cpu().numpy(), m.sigma.numpy())
    e_z = G.maxabs(out.z.cpu().numpy(), m.z.numpy())
    print(f"probunet predict fcomb{no_convs} {(B, S, H, W)} vs oracle: logits {e_l:.2e} mu {e_mu:.2e} sigma {e_sg:.2e} z {e_z:.2e}")
    assert e_l <= F.LOGIT_TOL_MODEL and e_mu <= 1e-4 and e_sg <= 1e-4 and e_z <= 1e-4
    _check_wiring(out, B, S)
    # labels against the oracle's, where the oracle is more than 2e-4 from a tie (at most 1 % of the pixels are not)
    sure = m.sure.numpy()
    assert 1.0 - sure.mean() <= 0.01
    assert np.array_equal(out.labels.cpu().numpy().reshape(S * B, H, W)[sure], m.labels.numpy()[sure])


@pytest.mark.parametrize("no_convs", F.NO_CONVS)
@pytest.mark.parametrize("B,S,H,W", F.SHAPES)
def test_predict_vs_forward_and_one_decode_per_sample(no_convs, B, S, H, W):
    """The parent commit's way to S distinct samples: forward(patch, None), then the decode tape once per sample with z_s."""
    c = _case(no_convs, B, S, H, W)
    dev = torch.device("cuda", 0)
    net = _net(c.m.sd, no_convs)
    with torch.no_grad():
        net.forward(c.m.patch.to(dev), None)
        z = c.out.z.reshape(S, B, F.LATENT)
        old = torch.cat([net._decode(z[s]) for s in range(S)], dim=0)
    assert net.check_bounds() == 0
    e = G.maxabs(old.cpu().numpy(), c.out.levels[0].cpu().numpy())
    print(f"probunet predict fcomb{no_convs} {(B, S, H, W)} vs forward + {S} x decode: {e:.2e}")
    assert e <= 2e-4


@pytest.mark.parametrize("no_convs", F.NO_CONVS)
def test_predict_sets_what_forward_sets_and_the_draws(no_convs):
    B, S, H, W = F.SHAPES[1]
    c = _case(no_convs, B, S, H, W)
    out, L = c.out, F.LATENT
    assert out.z.shape == (S * B, L) and out.mu.shape == (B, L) and out.sigma.shape == (B, L) and out.features.shape == (B, 32, H, W)
    mu, sg, eps = (t.cpu().numpy().astype(np.float64) for t in (out.mu, out.sigma, c.m.eps))
    want = np.tile(mu, (S, 1)) + np.tile(sg, (S, 1)) * eps
    gate = 2.0 ** -23 * (np.abs(np.tile(mu, (S, 1))) + np.abs(np.tile(sg, (S, 1)) * eps))
    assert np.all(np.abs(out.z.cpu().numpy() - want) <= gate)
    assert float(out.sigma.min()) > 0
    rows = out.levels[0].reshape(S, B, *out.levels[0].shape[1:])
    assert all(not torch.equal(rows[s], rows[0]) for s in range(1, S))               # samples, not the harness loop's S copies
    # the same noise on every sample row of an image: the rows are then equal bit for bit
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        same = c.net.predict(c.m.patch.to(dev), n_samples=S, eps=c.m.eps[:B].repeat(S, 1).to(dev))
    rows = same.levels[0].reshape(S, B, *same.levels[0].shape[1:])
    assert all(torch.equal(rows[s], rows[0]) for s in range(1, S)) and same.soft is None
    assert torch.equal(rows[0], c.out.levels[0][:B])
    _check_wiring(same, B, S)


@pytest.mark.parametrize("graphs", [False, True])
def test_predict_is_repeatable_and_replays(graphs):
    no_convs, (B, S, H, W) = 4, F.SHAPES[2]
    c = _case(no_convs, B, S, H, W)
    dev = torch.device("cuda", 0)
    net = _net(c.m.sd, no_convs, graphs=graphs)
    for _ in range(4):
        with torch.no_grad():
            out = net.predict(c.m.patch.to(dev), n_samples=S, eps=c.m.eps.to(dev))
        assert net.check_bounds() == 0
        assert torch.equal(out.levels[0], c.out.levels[0]) and torch.equal(out.labels, c.out.labels)
        assert torch.equal(out.mean_soft, c.out.mean_soft) and torch.equal(out.mean_label, c.out.mean_label) and torch.equal(out.entropy, c.out.entropy)
        assert torch.equal(net.z_prior_sample, c.out.z)
    assert list(net._plans) == [(B, H, W, False, False)]                            # the eval plan of forward(patch, None), nothing else


def test_predict_draws_its_own_noise():
    no_convs, (B, S, H, W) = 3, F.SHAPES[0]
    c = _case(no_convs, B, S, H, W)
    dev = torch.device("cuda", 0)
    net = _net(c.m.sd, no_convs)
    with torch.no_grad():
        a = net.predict(c.m.patch.to(dev), n_samples=S)
        la, ma, za = a.levels[0].clone(), a.mean_soft.clone(), net.z_prior_sample.clone()
        b = net.predict(c.m.patch.to(dev), n_samples=S)
    assert net.check_bounds() == 0
    assert not torch.equal(la, b.levels[0]) and not torch.equal(ma, b.mean_soft) and not torch.equal(za, net.z_prior_sample)
    rows = b.levels[0].reshape(S, B, *b.levels[0].shape[1:])
    assert all(not torch.equal(rows[s], rows[0]) for s in range(1, S))
    assert net.z_prior_sample.shape == (S * B, F.LATENT) and net.prior_latent_space.mean.shape == (B, F.LATENT)
    _check_wiring(b, B, S)


def test_predict_errors():
    from unet_zoo_amd import _ffi
    dev = torch.device("cuda", 0)
    m = F.model_case(3, *F.SHAPES[0])
    net = _net(m.sd, 3)
    x = m.patch.to(dev)
    with pytest.raises(ValueError):
        net.predict(x, n_samples=0)
    with pytest.raises(ValueError):
        net.predict(x, n_samples=2, eps=torch.zeros(3, F.LATENT, device=dev))
    net.train()
    with pytest.raises(RuntimeError):
        net.predict(x)
    from unet_zoo_amd.models.probabilistic_unet import ProbabilisticUnet
    rev = ProbabilisticUnet(1, 2, F.FILTERS, latent_dim=F.LATENT, no_convs_fcomb=3, image_size=(1, F.H0, F.H0), reversible=True)
    rev.eval()
    with pytest.raises(NotImplementedError):
        rev.predict(x)
    deep = ProbabilisticUnet(1, 2, F.FILTERS, latent_dim=F.LATENT, no_convs_fcomb=10, image_size=(1, F.H0, F.H0))
    deep.eval()
    with pytest.raises(_ffi.UzError, match="units"):                                # nine units: refused by the library, no fallback
        deep.predict(x)


def test_predict_leaves_training_what_it_was():
    """forward + loss + backward in train mode and in eval mode behind a predict(): the losses and gradients of a fresh model with
    the same state - the eval plan is shared with forward(patch, None) and the decode tape, the state is untouched."""
    no_convs, (B, S, H, W) = 3, F.SHAPES[1]
    c = _case(no_convs, B, S, H, W)
    dev = torch.device("cuda", 0)
    x = c.m.patch.to(dev)
    mask = (x > 0).float()
    eps = c.m.eps[:B].to(dev)
    got = []
    for first_predict in (True, False):
        net = _net(c.m.sd, no_convs)
        if first_predict:
            with torch.no_grad():
                net.predict(x, n_samples=S)
            assert all(torch.equal(v.cpu(), c.m.sd[k]) for k, v in net.state_dict().items())     # running statistics, counters: untouched
        with torch.no_grad():
            net.forward(x, None)
            dec = net._decode(c.out.z[:B])
        net.train()
        net.forward(x, mask, training=True)
        loss = net.loss(mask, eps=eps)
        loss.backward()
        got.append((float(loss.detach()), net._ptab.gflat.clone(), dec))
    assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])


def test_harness_predict_is_the_nets_predict(tmp_path):
    from unet_zoo_amd import train_model as TM
    from unet_zoo_amd.models import ProbabilisticUnet
    from unet_zoo_amd.models.phiseg import Prediction
    cfg = types.SimpleNamespace(experiment_name="t", log_dir_name="t", filter_channels=F.FILTERS, latent_levels=1, n_classes=2, no_convs_fcomb=3,
                                beta=1.0, use_reversible=False, input_channels=1, image_size=(1, F.H0, F.H0), batch_size=2, iterations=2,
                                logging_frequency=2, model=ProbabilisticUnet)
    h = TM.UNetModel(cfg, log_root=str(tmp_path))
    data = TM.SyntheticData(None, cfg, n_train=4, n_val=3)
    images = data.validation.images                                                 # (3, H0, H0) numpy
    h.net.train()
    h.net.set_rng_state(1234)
    a = h.predict(images, n_samples=2)
    assert isinstance(a, Prediction) and not h.net.training and a.soft is None
    keep = (a.labels.clone(), a.mean_soft.clone(), a.mean_label.clone(), a.entropy.clone(), a.levels[0].clone())
    h.net.set_rng_state(1234)
    with torch.no_grad():
        b = h.net.predict(torch.as_tensor(images, dtype=torch.float32).to(h.device).unsqueeze(1), n_samples=2)
    assert torch.equal(keep[0], b.labels) and torch.equal(keep[1], b.mean_soft) and torch.equal(keep[2], b.mean_label)
    assert torch.equal(keep[3], b.entropy) and torch.equal(keep[4], b.levels[0])
    _check_wiring(b, 3, 2)
