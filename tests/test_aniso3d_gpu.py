"""The training step, the validation forward, predict() and the replay of PHISeg3D on volumes with three unequal extents (the cases
of tests/_aniso3d.py), on the device.  Per case ONE step from the seeded state - forward(training=True, eps=...), loss, backward -
shared by the tests of the case; everything is compared with the CPU oracle's fp64 run and graded against the oracle's fp32 run on
the same inputs.  The gates are those of tests/test_nonsquare_gpu.py, unchanged; two axes exchanged, a level's extents mixed or a
resize factor taken from the wrong axis is off by O(1) (tests/test_aniso3d_cpu.py shows it on the oracle).

Measured on an MI355X (default mode / UZ_CONV_MATH=f32 / split): DESIGN.md section 5, "Anisotropic volumes"."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import _aniso3d as A

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _inputs(c):
    x, onehot, lab, eps = A.operands(c)
    T = lambda a: torch.from_numpy(np.array(a)).to(_dev())      # noqa: E731
    return T(x), T(onehot), T(lab), [T(e) for e in eps]


def _published(net, s, L):
    """The forward tensors forward() leaves on the model, under the oracle's names."""
    fwd = {}
    for l in range(L):
        fwd[f"s{l}"], fwd[f"s_in{l}"] = s[l], net.s_in_list[l]
        fwd[f"posterior_mu{l}"], fwd[f"posterior_sigma{l}"], fwd[f"posterior_z{l}"] = net.posterior_mu[l], net.posterior_sigma[l], net.posterior_latent_space[l]
        fwd[f"prior_mu{l}"], fwd[f"prior_sigma{l}"], fwd[f"prior_z{l}"] = net.prior_mu[l], net.prior_sigma[l], net.prior_latent_space[l]
    return fwd


@functools.lru_cache(maxsize=None)
def _step(name):
    """One training step of the case on the device, everything the tests read copied to the host (read-only, shared)."""
    c = A.BY_NAME[name]
    net = A.net(c)
    net.train()
    x, onehot, lab, eps = _inputs(c)
    s = net.forward(x, onehot, training=True, eps=eps)
    loss = net.loss(lab)
    fwd = {k: v.detach().cpu().clone() for k, v in _published(net, s, c.latent_levels).items()}
    terms = {k: float(v) for k, v in net.loss_dict.items()}
    loss.backward()
    torch.cuda.synchronize()
    bounds = net.check_bounds()
    params = dict(net.named_parameters())
    return types.SimpleNamespace(loss=float(loss.detach()), terms=terms, fwd=fwd,
                                 grads={k: p.grad.detach().cpu().clone() for k, p in params.items() if p.grad is not None},
                                 none_grads=sorted(k for k, p in params.items() if p.grad is None),
                                 buffers={k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k not in params},
                                 bounds=bounds)


def _check_forward(name, got, r32, r64):
    worst = (0.0, None)
    for k, ref in r64.fwd.items():
        assert tuple(got[k].shape) == tuple(ref.shape), (name, k, tuple(got[k].shape), tuple(ref.shape))
        e_hip, e_cpu = A.maxabs(got[k], ref), A.maxabs(r32.fwd[k], ref)
        print(f"{name} {k}: HIP {e_hip:.2e} | fp32 oracle {e_cpu:.2e} (max abs against fp64)")
        worst = max(worst, (e_hip, k))
        assert e_hip <= 2.0 * e_cpu + 2e-5 and e_hip <= A.FWD_CAP, (name, k, e_hip, e_cpu)
    print(f"{name}: worst forward tensor {worst[1]} at {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------ one training step per case
@pytest.mark.parametrize("name", A.IDS)
def test_loss_vs_fp64_oracle(name):
    c = A.BY_NAME[name]
    got, r32, r64 = _step(name), A.oracle_run(c, torch.float32), A.oracle_run(c, torch.float64)
    rel = abs(got.loss - r64.loss) / abs(r64.loss)
    print(f"{name}: loss {got.loss:.6f} fp64 {r64.loss:.6f} rel {rel:.1e} (fp32 oracle {abs(r32.loss - r64.loss) / abs(r64.loss):.1e})")
    assert rel <= A.LOSS_REL, (name, got.loss, r64.loss)
    assert set(got.terms) == set(r64.terms)
    for k, v in r64.terms.items():
        print(f"{name} {k}: {got.terms[k]:.6f} fp64 {v:.6f} off by {abs(got.terms[k] - v):.1e} (gate {A.LOSS_REL * abs(v):.1e})")
        assert abs(got.terms[k] - v) <= A.LOSS_REL * abs(v), (name, k, got.terms[k], v)
    assert got.bounds == 0, name                 # every magnitude bound a split-fp16 kernel was handed covered its tensor


@pytest.mark.parametrize("name", A.IDS)
def test_forward_tensors_vs_fp64_oracle(name):
    """Every s, s_in, mu, sigma and z of both encoders: the oracle's shape, within min(2 e_cpu32 + 2e-5, FWD_CAP) of fp64; and the
    resized level logits are the nearest resize of the returned un-resized ones bit for bit."""
    c = A.BY_NAME[name]
    got = _step(name).fwd
    _check_forward(name, got, A.oracle_run(c, torch.float32), A.oracle_run(c, torch.float64))
    for l in range(c.latent_levels):
        assert torch.equal(got[f"s{l}"], A.nearest_full(got[f"s_in{l}"], c.dhw)), (name, l)


@pytest.mark.parametrize("name", A.IDS)
def test_gradients_vs_fp64_oracle(name):
    """Per tensor r = max |g - g64| / max |g64|.  Gates: median(r_hip) <= 2 median(r_cpu32) + 1e-6; max(r_hip) <= max(3 max(r_cpu32)
    + 1e-4, 0.15); no tensor beyond 25 r_cpu32 + 2e-3."""
    c = A.BY_NAME[name]
    got, r32, r64 = _step(name), A.oracle_run(c, torch.float32), A.oracle_run(c, torch.float64)
    assert got.none_grads == r64.none_grads, (name, set(got.none_grads) ^ set(r64.none_grads))
    keys = A.grad_keys(r64)
    for k in keys:
        assert tuple(got.grads[k].shape) == tuple(r64.grads[k].shape), (name, k)
    rh, rc = A.grad_ratios(lambda k: got.grads[k], r64, keys), A.grad_ratios(lambda k: r32.grads[k], r64, keys)
    worst = int(np.argmax(rh / (3.0 * rc + 2e-5)))
    print(f"{name}: grad err vs fp64 rel. to tensor max  HIP median {np.median(rh):.2e} p90 {np.percentile(rh, 90):.2e} max {rh.max():.2e} | fp32 CPU "
          f"median {np.median(rc):.2e} p90 {np.percentile(rc, 90):.2e} max {rc.max():.2e} | worst per-tensor ratio "
          f"{rh[worst] / (3.0 * rc[worst] + 2e-5):.2f} at {keys[worst]} ({rh[worst]:.2e} vs {rc[worst]:.2e}) over {len(keys)} tensors")
    failed = A.gradient_gates(rh, rc, keys)
    assert not failed, (name, failed)


@pytest.mark.parametrize("name", A.IDS)
def test_batchnorm_buffers_after_the_step(name):
    c = A.BY_NAME[name]
    got, want = _step(name).buffers, A.expected_buffers(c, A.oracle_run(c, torch.float64))
    assert set(got) == set(want) and len(want) > 30
    e_rm = e_rv = 0.0
    for k, v in want.items():
        if k.endswith("running_mean"):
            e_rm = max(e_rm, A.maxabs(got[k], v))
            assert A.maxabs(got[k], v) <= A.RM_TOL, (name, k)
        elif k.endswith("running_var"):
            e = float(((got[k].double() - v.double()).abs() / v.double().abs()).max())
            e_rv = max(e_rv, e)
            assert e <= A.RV_REL, (name, k, e)
        else:
            assert int(got[k]) == int(v), (name, k, int(got[k]), int(v))
    print(f"{name}: running mean within {e_rm:.1e}, running variance within {e_rv:.1e} (relative) of the fp64 oracle")


# ------------------------------------------------------------------------------------------ validation forward
@pytest.mark.parametrize("name", A.VALIDATION)
def test_validation_forward(name):
    """forward(training=False) in eval mode from the off-identity state - eval-mode BatchNorm, the prior's own samples - against the
    oracle with bn_train=False, at the forward gate; statistics and counters stay untouched."""
    c = A.validation_case(name)
    r32, r64 = A.oracle_run(c, torch.float32, train=False), A.oracle_run(c, torch.float64, train=False)
    net = A.net(c)
    net.eval()
    x, onehot, _, eps = _inputs(c)
    state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        s = net.forward(x, onehot, training=False, eps=eps)
        fwd = {k: v.detach().cpu().clone() for k, v in _published(net, s, c.latent_levels).items()}
    assert net.check_bounds() == 0
    _check_forward(c.name, fwd, r32, r64)
    assert all(torch.equal(v.cpu(), state[k]) for k, v in net.state_dict().items())


# ------------------------------------------------------------------------------------------ predict()
def test_predict_with_injected_noise_vs_oracle():
    """predict(patch, n_samples=3, eps=..., return_levels=True): every sample's un-resized level logits within the forward gate of the
    oracle's s_in, mean_soft within 1e-5 of the mean softmax of the oracle's accumulated logits, and the labels equal to the fp64
    oracle's wherever its two largest accumulated logits are MARGIN apart."""
    m = A.predict_case()
    c = m.case
    D, H, W = c.dhw
    net = A.net(c)
    net.eval()
    with torch.no_grad():
        out = net.predict(m.patch.to(_dev()), n_samples=m.S, eps=[e.to(_dev()) for e in m.eps], return_levels=True)
    torch.cuda.synchronize()
    assert net.check_bounds() == 0
    assert out.labels.shape == (m.S, 1, D, H, W) and out.mean_soft.shape == (1, A.K, D, H, W)
    for l in range(c.latent_levels):
        assert out.levels[l].shape == (m.S, 1, A.K, D >> l, H >> l, W >> l)
        for s in range(m.S):
            ref = m.r64.s_in[s][l]
            e_hip, e_cpu = A.maxabs(out.levels[l][s], ref), A.maxabs(m.r32.s_in[s][l], ref)
            print(f"predict {c.name} level {l} sample {s}: HIP {e_hip:.2e} | fp32 oracle {e_cpu:.2e}")
            assert e_hip <= A.fwd_gate(e_cpu), (l, s, e_hip, e_cpu)
    e = A.maxabs(out.mean_soft, m.r64.mean_soft)
    print(f"predict {c.name}: mean_soft within {e:.2e} of the fp64 oracle")
    assert e <= 1e-5
    assert m.unsure_fraction <= A.MARGIN_FRACTION
    labels = out.labels[:, 0].cpu().long()
    assert torch.equal(labels[m.sure], m.r64.labels[m.sure]), int((labels != m.r64.labels)[m.sure].sum())


# ------------------------------------------------------------------------------------------ replay
@pytest.mark.parametrize("lanes", ["1", "3"])
@pytest.mark.parametrize("name", A.REPLAY)
def test_replay_is_bit_identical_to_eager(name, lanes, monkeypatch):
    """Five FusedAdam steps eager and under enable_graphs(True) (one lane: eager warm-up, capture, replay; three: the lane replay
    or the captured DAG): loss, logits and the flat gradient buffer equal bit for bit at every step, parameters and both moments
    after the last."""
    from unet_zoo_amd.optim import FusedAdam
    monkeypatch.setenv("UZ_LANES", lanes)
    c = A.BY_NAME[name]
    x, onehot, lab, eps = _inputs(c)
    runs, finals = [], []
    for graphs in (False, True):
        net = A.net(c)
        net.train()
        net.enable_graphs(graphs)
        opt = FusedAdam(net, lr=1e-3, weight_decay=1e-5)
        steps = []
        for _ in range(5):
            s = net.forward(x, onehot, training=True, eps=eps)
            loss = net.loss(lab)
            logits = [t.clone() for t in s]
            opt.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
            steps.append((float(loss.detach()), logits, net._ptab.gflat.clone()))
            opt.step()
        torch.cuda.synchronize()
        assert net.check_bounds() == 0
        runs.append(steps)
        finals.append((net._ptab.pflat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()))
    for k, ((l0, s0, g0), (l1, s1, g1)) in enumerate(zip(*runs)):
        assert np.isfinite(l0) and l0 == l1, (name, k, l0, l1)
        assert all(torch.equal(a, b) for a, b in zip(s0, s1)), (name, k)
        assert torch.equal(g0, g1), (name, k)
    assert all(torch.equal(a, b) for a, b in zip(*finals)), name
    assert runs[0][0][0] != runs[0][4][0]                                              # the steps moved the parameters


# ------------------------------------------------------------------------------------------ the other arithmetic modes
_FAILED_CHILDREN = []


@pytest.mark.parametrize("mode", ["f32", "split"])
def test_anisotropic_volumes_in_the_other_arithmetic_modes(mode):
    """This file's model tests again with the convolutions forced onto the fp32-MFMA kernels and onto the split-fp16 kernels (the
    default mode is this process).  The switch is read once per process, hence the child process; the gates are the same."""
    assert not _FAILED_CHILDREN, f"the child run under {_FAILED_CHILDREN} failed: nothing more is started on the device"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, UZ_CONV_MATH=mode)
    _FAILED_CHILDREN.append(mode)                                                     # until it has ended well: a time-out raises
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_aniso3d_gpu.py", "-q", "-x", "-m", "gpu", "-k", "not arithmetic_modes"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    _FAILED_CHILDREN.remove(mode)
