"""The training step, the validation forward, the replay and predict() of the 2-D models on images with H != W (the cases of
tests/_nonsquare.py), on the device.  Per case ONE step from the seeded state - forward(training=True), loss, backward - shared
by the tests of the case; everything is compared with the CPU oracle's fp64 run and graded against the oracle's fp32 run on the
same inputs.  The gates are those of tests/test_phiseg_gpu.py (test_phiseg_accuracy_vs_fp64_ground_truth and the "none beyond"
rule of test_phiseg_b32_gradients_vs_fp64_reference), unchanged; a transposed or shifted plane is off by O(1).

Measured on an MI355X (default mode / UZ_CONV_MATH=f32 / split): DESIGN.md section 5, "Non-square images"."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests import _nonsquare as NS

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _inputs(c):
    x, mask, eps = NS.operands(c)
    return (torch.from_numpy(np.array(x)).to(_dev()), torch.from_numpy(np.array(mask)).to(_dev()),
            [torch.from_numpy(np.array(e)).to(_dev()) for e in eps])


def _forward_loss(c, net, x, mask, eps):
    """forward + loss of one training step -> (loss, forward tensors by the oracle's names, loss terms by the oracle's names)."""
    if c.model == "phiseg":
        s = net.forward(x, mask, training=True, eps=eps)
        loss = net.loss(mask)
        fwd = {}
        for l in range(5):
            fwd[f"s{l}"] = s[l]
            fwd[f"posterior_mu{l}"], fwd[f"posterior_sigma{l}"], fwd[f"posterior_z{l}"] = net.posterior_mu[l], net.posterior_sigma[l], net.posterior_latent_space[l]
            fwd[f"prior_mu{l}"], fwd[f"prior_sigma{l}"], fwd[f"prior_z{l}"] = net.prior_mu[l], net.prior_sigma[l], net.prior_latent_space[l]
        return loss, fwd, dict(net.loss_dict)
    if c.model == "unet":
        pred = net.forward(x)
        return net.loss(mask), {"pred": pred}, {}
    last = net.forward(x, mask, training=True)
    loss = net.loss(mask, eps=eps[0])
    fwd = dict(last_conv=last, unet_features=net.unet_features, reconstruction=net.reconstruction,
               posterior_mu=net.posterior_latent_space.mean, posterior_sigma=net.posterior_latent_space.base_dist.scale,
               prior_mu=net.prior_latent_space.mean, prior_sigma=net.prior_latent_space.base_dist.scale)
    return loss, fwd, dict(reconstruction_loss=net.reconstruction_loss, kl=net.kl_divergence_loss)


@functools.lru_cache(maxsize=None)
def _step(name):
    """One training step of the case on the device, everything the tests read copied to the host (read-only, shared)."""
    c = NS.BY_NAME[name]
    net = NS.net(c)
    net.train()
    x, mask, eps = _inputs(c)
    loss, fwd, terms = _forward_loss(c, net, x, mask, eps)
    fwd = {k: v.detach().cpu().clone() for k, v in fwd.items()}
    loss.backward()
    torch.cuda.synchronize()
    bounds = net.check_bounds()
    params = dict(net.named_parameters())
    return types.SimpleNamespace(loss=float(loss.detach()), terms={k: float(v) for k, v in terms.items()}, fwd=fwd,
                                 grads={k: p.grad.detach().cpu().clone() for k, p in params.items() if p.grad is not None},
                                 none_grads=sorted(k for k, p in params.items() if p.grad is None),
                                 buffers={k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k not in params},
                                 bounds=bounds)


def _check_forward(name, got, r32, r64):
    for k, ref in r64.fwd.items():
        assert tuple(got[k].shape) == tuple(ref.shape), (name, k, tuple(got[k].shape), tuple(ref.shape))
        e_hip, e_cpu = NS.maxabs(got[k], ref), NS.maxabs(r32.fwd[k], ref)
        print(f"{name} {k}: HIP {e_hip:.2e} | fp32 oracle {e_cpu:.2e} (max abs against fp64)")
        assert e_hip <= 2.0 * e_cpu + 2e-5 and e_hip <= NS.FWD_CAP, (name, k, e_hip, e_cpu)


# ------------------------------------------------------------------------------------------ one training step per case
@pytest.mark.parametrize("name", NS.IDS)
def test_loss_vs_fp64_oracle(name):
    c = NS.BY_NAME[name]
    got, r32, r64 = _step(name), NS.oracle_run(c, torch.float32), NS.oracle_run(c, torch.float64)
    rel = abs(got.loss - r64.loss) / abs(r64.loss)
    print(f"{name}: loss {got.loss:.6f} fp64 {r64.loss:.6f} rel {rel:.1e} (fp32 oracle {abs(r32.loss - r64.loss) / abs(r64.loss):.1e})")
    assert rel <= NS.LOSS_REL, (name, got.loss, r64.loss)
    assert set(got.terms) == set(r64.terms)
    for k, v in r64.terms.items():
        tol = NS.kl_bound(r32, r64) if (c.model, k) == ("probunet", "kl") else NS.LOSS_REL * abs(v)
        print(f"{name} {k}: {got.terms[k]:.6f} fp64 {v:.6f} off by {abs(got.terms[k] - v):.1e} (gate {tol:.1e})")
        assert abs(got.terms[k] - v) <= tol, (name, k, got.terms[k], v)
    assert got.bounds == 0, name                 # every magnitude bound a split-fp16 kernel was handed covered its tensor


@pytest.mark.parametrize("name", NS.IDS)
def test_forward_tensors_vs_fp64_oracle(name):
    c = NS.BY_NAME[name]
    _check_forward(name, _step(name).fwd, NS.oracle_run(c, torch.float32), NS.oracle_run(c, torch.float64))


@pytest.mark.parametrize("name", NS.IDS)
def test_gradients_vs_fp64_oracle(name):
    """Per tensor r = max |g - g64| / max |g64|.  Gates: median(r_hip) <= 2 median(r_cpu32) + 1e-6; max(r_hip) <= max(3 max(r_cpu32)
    + 1e-4, 0.15); no tensor beyond 25 r_cpu32 + 2e-3."""
    c = NS.BY_NAME[name]
    got, r32, r64 = _step(name), NS.oracle_run(c, torch.float32), NS.oracle_run(c, torch.float64)
    assert got.none_grads == r64.none_grads, (name, set(got.none_grads) ^ set(r64.none_grads))
    keys = NS.grad_keys(r64)
    for k in keys:
        assert tuple(got.grads[k].shape) == tuple(r64.grads[k].shape), (name, k)
    rh, rc = NS.grad_ratios(lambda k: got.grads[k], r64, keys), NS.grad_ratios(lambda k: r32.grads[k], r64, keys)
    worst = int(np.argmax(rh / (3.0 * rc + 2e-5)))
    print(f"{name}: grad err vs fp64 rel. to tensor max  HIP median {np.median(rh):.2e} p90 {np.percentile(rh, 90):.2e} max {rh.max():.2e} | fp32 CPU "
          f"median {np.median(rc):.2e} p90 {np.percentile(rc, 90):.2e} max {rc.max():.2e} | worst per-tensor ratio "
          f"{rh[worst] / (3.0 * rc[worst] + 2e-5):.2f} at {keys[worst]} ({rh[worst]:.2e} vs {rc[worst]:.2e}) over {len(keys)} tensors")
    failed = NS.gradient_gates(rh, rc, keys)
    assert not failed, (name, failed)


@pytest.mark.parametrize("name", [c.name for c in NS.CASES if c.model != "unet"])
def test_batchnorm_buffers_after_the_step(name):
    c = NS.BY_NAME[name]
    got, want = _step(name).buffers, NS.expected_buffers(c, NS.oracle_run(c, torch.float64))
    assert set(got) == set(want) and len(want) > 30
    e_rm = e_rv = 0.0
    for k, v in want.items():
        if k.endswith("running_mean"):
            e_rm = max(e_rm, NS.maxabs(got[k], v))
            assert NS.maxabs(got[k], v) <= NS.RM_TOL, (name, k)
        elif k.endswith("running_var"):
            e = float(((got[k].double() - v.double()).abs() / v.double().abs()).max())
            e_rv = max(e_rv, e)
            assert e <= NS.RV_REL, (name, k, e)
        else:
            assert int(got[k]) == int(v), (name, k, int(got[k]), int(v))
    print(f"{name}: running mean within {e_rm:.1e}, running variance within {e_rv:.1e} (relative) of the fp64 oracle")


# ------------------------------------------------------------------------------------------ validation forward
@pytest.mark.parametrize("name", NS.VALIDATION)
def test_validation_forward_and_labels(name):
    """Eval-mode BatchNorm and the prior's own samples (PHISeg forward(training=False); Unet val=True) against the oracle with
    bn_train=False; the labels equal the fp64 oracle's wherever its two largest accumulated logits are MARGIN apart."""
    c = NS.validation_case(name)
    r32, r64 = NS.oracle_run(c, torch.float32, train=False), NS.oracle_run(c, torch.float64, train=False)
    net = NS.net(c)
    net.eval()
    x, mask, eps = _inputs(c)
    state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        if c.model == "phiseg":
            s = net.forward(x, mask, training=False, eps=eps)
            fwd = {}
            for l in range(5):
                fwd[f"s{l}"] = s[l].clone()
                fwd[f"posterior_mu{l}"], fwd[f"posterior_sigma{l}"], fwd[f"posterior_z{l}"] = net.posterior_mu[l], net.posterior_sigma[l], net.posterior_latent_space[l]
                fwd[f"prior_mu{l}"], fwd[f"prior_sigma{l}"], fwd[f"prior_z{l}"] = net.prior_mu[l], net.prior_sigma[l], net.prior_latent_space[l]
            labels = torch.argmax(net.accumulate_output(s, use_softmax=True), dim=1).cpu()
        else:
            pred = net.forward(x, val=True)
            fwd = {"pred": pred}
            labels = torch.argmax(pred, dim=1).cpu()
            assert net.activation_maps[-1] is pred
    assert net.check_bounds() == 0
    _check_forward(name, fwd, r32, r64)
    acc = NS.accumulated(c, r64)
    frac, sure = NS.unsure_fraction(acc)
    assert frac <= NS.MARGIN_FRACTION and labels.shape == (c.N, c.H, c.W)
    assert torch.equal(labels[sure], acc.argmax(dim=1)[sure]), (name, int((labels != acc.argmax(dim=1))[sure].sum()))
    assert all(torch.equal(v.cpu(), state[k]) for k, v in net.state_dict().items())      # eval mode: statistics and counters untouched


# ------------------------------------------------------------------------------------------ replay
@pytest.mark.parametrize("lanes", ["1", "3"])
@pytest.mark.parametrize("name", NS.REPLAY)
def test_replay_is_bit_identical_to_eager(name, lanes, monkeypatch):
    """Five FusedAdam steps eager and under enable_graphs(True) (one lane: eager warm-up, capture, replay; three: the lane replay
    or the captured DAG): loss, logits and the flat gradient buffer equal bit for bit at every step."""
    from unet_zoo_amd.optim import FusedAdam
    monkeypatch.setenv("UZ_LANES", lanes)
    c = NS.BY_NAME[name]
    x, mask, eps = _inputs(c)
    runs = []
    for graphs in (False, True):
        net = NS.net(c)
        net.train()
        net.enable_graphs(graphs)
        opt = FusedAdam(net, lr=1e-3, weight_decay=1e-5)
        steps = []
        for _ in range(5):
            loss, fwd, _terms = _forward_loss(c, net, x, mask, eps)
            logits = [fwd[k].clone() for k in (("s0", "s1", "s2", "s3", "s4") if c.model == "phiseg" else ("reconstruction", "last_conv"))]
            opt.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
            steps.append((float(loss.detach()), logits, net._ptab.gflat.clone()))
            opt.step()
        assert net.check_bounds() == 0
        runs.append(steps)
    for k, ((l0, s0, g0), (l1, s1, g1)) in enumerate(zip(*runs)):
        assert np.isfinite(l0) and l0 == l1, (name, k, l0, l1)
        assert all(torch.equal(a, b) for a, b in zip(s0, s1)), (name, k)
        assert torch.equal(g0, g1), (name, k)
    assert runs[0][0][0] != runs[0][4][0]                                              # the steps moved the parameters


# ------------------------------------------------------------------------------------------ predict(), tall
def _phiseg_predict_tests():
    from tests import test_predict_gpu as TP
    return TP


def test_phiseg_predict_tall_vs_cpu_oracle():
    """The model-level checks of tests/test_predict_gpu.py - oracle, forward on the repeated patch, one trunk per image - at the
    transpose of their wide shape, with their helpers and gates."""
    TP = _phiseg_predict_tests()
    assert NS.PREDICT_SHAPE not in TP.SHAPES
    TP.test_predict_model_vs_cpu_oracle(*NS.PREDICT_SHAPE)


def test_phiseg_predict_tall_vs_forward_on_the_repeated_patch():
    _phiseg_predict_tests().test_predict_model_vs_forward_on_the_repeated_patch(*NS.PREDICT_SHAPE)


def test_phiseg_predict_tall_gives_every_sample_of_an_image_the_same_trunk():
    _phiseg_predict_tests().test_predict_model_gives_every_sample_of_an_image_the_same_trunk(*NS.PREDICT_SHAPE)


@pytest.mark.parametrize("no_convs", sorted(NS.PROBUNET_PREDICT_SEEDS))
def test_probunet_predict_tall(no_convs):
    """test_fcomb_gpu's test_predict_vs_cpu_oracle and test_predict_vs_forward_and_one_decode_per_sample at the tall shape: the
    same state (tests/_fcomb.model_state), helpers and gates; the case's data seed is this file's (tests/_nonsquare.py)."""
    from tests import _fcomb as F
    from tests import test_fcomb_gpu as TF
    B, S, H, W = NS.PREDICT_SHAPE
    m = NS.probunet_predict_case(no_convs)
    net = TF._net(m.sd, no_convs)
    with torch.no_grad():
        out = net.predict(m.patch.to(_dev()), n_samples=S, eps=m.eps.to(_dev()), return_soft=True)
    torch.cuda.synchronize()
    assert net.check_bounds() == 0
    z = net.z_prior_sample.clone()
    e_l = G.maxabs(out.levels[0].cpu().numpy(), m.logits.numpy())
    e_mu, e_sg = G.maxabs(net.prior_latent_space.mean.cpu().numpy(), m.mu.numpy()), G.maxabs(net.prior_latent_space.stddev.cpu().numpy(), m.sigma.numpy())
    e_z = G.maxabs(z.cpu().numpy(), m.z.numpy())
    print(f"probunet predict fcomb{no_convs} {NS.PREDICT_SHAPE} vs oracle: logits {e_l:.2e} mu {e_mu:.2e} sigma {e_sg:.2e} z {e_z:.2e}")
    assert e_l <= F.LOGIT_TOL_MODEL and e_mu <= 1e-4 and e_sg <= 1e-4 and e_z <= 1e-4
    TF._check_wiring(out, B, S)
    sure = m.sure.numpy()
    assert 1.0 - sure.mean() <= 0.01
    assert np.array_equal(out.labels.cpu().numpy().reshape(S * B, H, W)[sure], m.labels.numpy()[sure])
    logits = out.levels[0].clone()
    # the older route to S distinct samples: forward(patch, None), then the decode tape once per sample with z_s
    old_net = TF._net(m.sd, no_convs)
    with torch.no_grad():
        old_net.forward(m.patch.to(_dev()), None)
        old = torch.cat([old_net._decode(z.reshape(S, B, F.LATENT)[s]) for s in range(S)], dim=0)
    assert old_net.check_bounds() == 0
    e = G.maxabs(old.cpu().numpy(), logits.cpu().numpy())
    print(f"probunet predict fcomb{no_convs} {NS.PREDICT_SHAPE} vs forward + {S} x decode: {e:.2e}")
    assert e <= 2e-4


# ------------------------------------------------------------------------------------------ harness
def test_harness_trains_and_validates_on_a_wide_image(tmp_path):
    """train_model.UNetModel on 64 x 128 images: batch assembly with augmentation, one optimiser step and the validation loop;
    the metrics have the shapes and ranges of the square run of tests/test_harness.py."""
    from unet_zoo_amd import train_model as TM
    from unet_zoo_amd.models import PHISeg
    cfg = types.SimpleNamespace(experiment_name="t", log_dir_name="t", filter_channels=NS.NARROW7, latent_levels=5, n_classes=2, no_convs_fcomb=3,
                                beta=1.0, use_reversible=False, input_channels=1, image_size=(1, 64, 128), batch_size=2, iterations=2,
                                logging_frequency=2, model=PHISeg)
    h = TM.UNetModel(cfg, log_root=str(tmp_path))
    data = TM.SyntheticData(None, cfg, n_train=4, n_val=3)
    # the scale augmentation is defined for square images only (tests/test_nonsquare_cpu.py); the stand-in keeps the rotations
    assert data.train.augmentation_options["do_scaleaug"] is False and data.train.augmentation_options["do_rotations"] is True
    np.random.seed(3)                                                                  # the provider draws from numpy's global RNG
    assert data.validation.images.shape == (3, 64, 128) and data.validation.labels.shape == (3, 64, 128, 4)
    before = {k: v.detach().clone() for k, v in h.net.state_dict().items() if v.dtype.is_floating_point}
    h.train(data)
    assert h.patch.shape == (2, 1, 64, 128) and h.mask.shape == (2, 1, 64, 128)
    assert torch.isfinite(h.loss) and h.net.check_bounds() == 0
    after = h.net.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
    cfg.validation_samples, cfg.num_validation_images = 4, 2
    m = h.validate(data)
    assert set(m) == {"dice", "foreground_dice", "elbo", "ged", "ncc"} and np.isfinite(m["elbo"])
    assert 0.0 <= m["dice"] <= 1.0 and -1.0 <= m["ncc"] <= 1.0 and m["ged"] >= -1e-9
    assert os.path.exists(os.path.join(str(tmp_path), "t", "t", "t_best_ged.pth"))


# ------------------------------------------------------------------------------------------ the other arithmetic modes
@pytest.mark.parametrize("mode", ["f32", "split"])
def test_nonsquare_models_in_the_other_arithmetic_modes(mode):
    """This file's model tests again with the convolutions forced onto the fp32-MFMA kernels and onto the split-fp16 kernels (the
    default mode is this process).  The switch is read once per process, hence the child process; the gates are the same."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, UZ_CONV_MATH=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_nonsquare_gpu.py", "-q", "-x", "-m", "gpu", "-k", "not arithmetic_modes"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
