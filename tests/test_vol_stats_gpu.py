"""Mask-free inference on volumes on the device: uz_vol_sample_accum / uz_vol_sample_finish (csrc/predict.hip) on the cases of
tests/_vol_stats.py against fp64 and - bit for bit - against uz_sample_stats on the materialised levels, and PHISeg3D.predict against
the CPU oracle, against forward() in eval mode, and against the numpy twin of the statistics on its own level logits.
Gates: softmax 1e-6, mean and entropy as derived in tests/_predict.py (the 2-D kernel's: the arithmetic is the same); level logits
1e-4 max(1, |ref|) against the oracle (test_native_model_vs_reference_modules), 2e-4 between two device paths that each carry 1e-4."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import refgraph3d as R3
from tests import _golden as G
from tests import _nets as N
from tests import _predict as P
from tests import _vol_stats as VS

pytestmark = pytest.mark.gpu

PAD = 64                                                                            # canary elements on either side of every output
CANARY_F, CANARY_B = -777.0, 255


def _g():
    from tests import _gpu
    return _gpu


# ------------------------------------------------------------------------------------------ op level
class _Out:
    """The outputs of one accum ... accum, finish sequence, each inside a buffer with PAD canary elements in front and behind;
    shift: elements the running sum (and mean_soft) start off their 16-byte boundary."""

    def __init__(self, g, K, S, n, soft=True, shift=0):
        def buf(count, dtype, off=0):
            return g.guarded(count, dtype, PAD, CANARY_B if dtype == torch.uint8 else CANARY_F, off, room=shift)
        self.g, self.n, self.K, self.S = g, n, K, S
        bufs = dict(labels=buf(S * n, torch.uint8), soft=buf(S * K * n, torch.float32) if soft else (None, None),
                    acc=buf(K * n, torch.float64, shift), mean_soft=buf(K * n, torch.float32, shift),
                    mean_label=buf(n, torch.uint8), entropy=buf(n, torch.float32))
        self.raw = {k: b[0] for k, b in bufs.items()}
        self.bodies = {k: b[1] for k, b in bufs.items()}

    def body(self, name):
        return self.bodies[name]

    def ptr(self, name, offset=0):
        t = self.body(name)
        return None if t is None else t.data_ptr() + offset * t.element_size()

    def canaries_intact(self):
        return all(self.g.intact(t, self.bodies[k], CANARY_B if t.dtype == torch.uint8 else CANARY_F) for k, t in self.raw.items() if t is not None)

    def untouched(self):
        return all(bool((t == (CANARY_B if t.dtype == torch.uint8 else CANARY_F)).all()) for t in self.raw.values() if t is not None)

    def result(self, dhw):
        D, H, W = dhw
        K, S = self.K, self.S
        r = dict(labels=self.body("labels").view(S, D, H, W), acc=self.body("acc").view(K, D, H, W), mean_soft=self.body("mean_soft").view(K, D, H, W),
                 mean_label=self.body("mean_label").view(D, H, W), entropy=self.body("entropy").view(D, H, W))
        if self.raw["soft"] is not None:
            r["soft"] = self.body("soft").view(S, K, D, H, W)
        return {k: v.clone() for k, v in r.items()}


def _dev_levels(g, c, levels, s, K, fill):
    """Sample s of every level as a volume in plan layout - [D_l + 2][K + extra][H_l][W_l], the classes at channel c0 - whose border
    slices and other channels hold `fill`; returns the buffers and the host tables of the call."""
    bufs, ptrs = [], []
    for l, lv in enumerate(levels):
        d, h, w = VS.level_shape(c, l)
        b = torch.full((d + 2, K + c.extra, h, w), fill, device=g.dev())
        b[1:d + 1, c.c0:c.c0 + K] = torch.from_numpy(lv[s].copy()).permute(1, 0, 2, 3).to(g.dev())
        bufs.append(b)
        ptrs.append(b[1:, c.c0:].data_ptr())
    n = len(levels)
    tabs = ((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[K + c.extra] * n), (ctypes.c_int * n)(*[f for f, _ in c.factors]),
            (ctypes.c_int * n)(*[fz for _, fz in c.factors]))
    return bufs, tabs


def _run_pair(g, c, levels, K, S, fill=float("nan"), soft=True, shift=0):
    D, H, W = c.dhw
    n = D * H * W
    out = _Out(g, K, S, n, soft=soft, shift=shift)
    for s in range(S):
        bufs, tabs = _dev_levels(g, c, levels, s, K, fill)
        g.call("uz_vol_sample_accum", *tabs, len(levels), K, D, H, W, out.ptr("labels", s * n), out.ptr("soft", s * K * n) if soft else None,
               out.ptr("acc"), int(s == 0))
        for b, lv in zip(bufs, levels):                                              # the logits are read, never written
            d = b.shape[0] - 2
            assert np.array_equal(b[1:d + 1, c.c0:c.c0 + K].permute(1, 0, 2, 3).cpu().numpy(), lv[s])
    g.call("uz_vol_sample_finish", out.ptr("acc"), K, S, D, H, W, out.ptr("mean_soft"), out.ptr("mean_label"), out.ptr("entropy"))
    assert out.canaries_intact(), (VS.case_id(c), K, S, shift)
    return out.result(c.dhw)


def _sample_stats_2d(g, flat, K, S, n):
    """uz_sample_stats fed the materialised, nearest-resized levels in one go: B = 1, H W := D H W."""
    dev = g.dev()
    lv = [torch.from_numpy(a.copy()).to(dev) for a in flat]
    tab = torch.tensor([t.data_ptr() for t in lv], dtype=torch.int64, device=dev)
    out = dict(soft=torch.empty(S, K, 1, n, device=dev), labels=torch.empty(S, 1, n, dtype=torch.uint8, device=dev),
               mean_soft=torch.empty(1, K, 1, n, device=dev), mean_label=torch.empty(1, 1, n, dtype=torch.uint8, device=dev),
               entropy=torch.empty(1, 1, n, device=dev))
    g.call("uz_sample_stats", tab, len(lv), K, 1, S, 1, n, out["soft"], out["labels"], out["mean_soft"], out["mean_label"], out["entropy"])
    return out


@pytest.mark.parametrize("i", range(len(VS.CASES)), ids=[VS.case_id(c) for c in VS.CASES])
def test_vol_stats_vs_fp64_and_bit_equal_to_sample_stats(i):
    g, c = _g(), VS.CASES[i]
    D, H, W = c.dhw
    n = D * H * W
    for K in VS.STATS_K:
        for S in VS.STATS_S:
            levels, flat, ref = VS.vol_case(i, K, S)
            case = (VS.case_id(c), K, S)
            got = _run_pair(g, c, levels, K, S)                                     # NaN in the border slices and the other channels
            e = {k: G.maxabs(got[k].cpu().numpy(), ref[k]) for k in ("soft", "mean_soft", "entropy")}
            print(f"vol_stats {case}: soft {e['soft']:.2e} mean_soft {e['mean_soft']:.2e} entropy {e['entropy']:.2e}")
            assert np.array_equal(got["labels"].cpu().numpy(), ref["labels"]), case  # everywhere: the inputs make sums and ties exact
            assert np.array_equal(got["mean_label"].cpu().numpy(), ref["mean_label"]), case
            assert e["soft"] <= P.SOFT_TOL and e["mean_soft"] <= P.mean_soft_tol(S) and e["entropy"] <= P.ENTROPY_TOL, (case, e)
            # S accum calls and one finish = the 2-D kernel fed every sample in one go, bit for bit
            two = _sample_stats_2d(g, flat, K, S, n)
            for k in ("soft", "labels", "mean_soft", "mean_label", "entropy"):
                assert torch.equal(got[k].reshape(-1), two[k].reshape(-1)), (case, k)
            # what lies around the operands is never read: a finite filler instead of NaN gives the same bits; so does a second launch
            for again in (_run_pair(g, c, levels, K, S, fill=3.0e30), _run_pair(g, c, levels, K, S)):
                assert all(torch.equal(got[k], again[k]) for k in got), case
            # no alignment beyond the element's is assumed (the running sum 8, mean_soft 4 bytes off a 16-byte boundary); a null soft
            other = _run_pair(g, c, levels, K, S, shift=1)
            assert all(torch.equal(got[k], other[k]) for k in got), case
            bare = _run_pair(g, c, levels, K, S, soft=False)
            assert all(torch.equal(got[k], bare[k]) for k in bare), case


def test_vol_stats_ties_and_zero_probabilities():
    g = _g()
    c = VS.Case((1, 1, 1), ((1, 1),), 0, 0)
    got = _run_pair(g, c, [np.array([[1.0, 2.5, 2.5, -1.0]], np.float32).reshape(1, 4, 1, 1, 1)], 4, 1)
    assert int(got["labels"]) == 1 and int(got["mean_label"]) == 1                  # first maximum wins
    for big in (60.0, 500.0):                                                       # a mean probability of 7.7e-53, and of 0 exactly
        got = _run_pair(g, c, [np.array([[big, -big]], np.float32).reshape(1, 2, 1, 1, 1)], 2, 1)
        assert torch.isfinite(got["entropy"]).all() and float(got["entropy"].abs().max()) <= 1e-30
        assert got["mean_soft"].flatten().tolist() == [1.0, 0.0] and int(got["mean_label"]) == 0


def test_vol_stats_refusals_write_nothing():
    from unet_zoo_amd import _ffi
    g = _g()
    c, K, S = VS.CASES[6], 3, 1                                                     # (4, 8, 8), levels at (1, 1) and (2, 1)
    D, H, W = c.dhw
    n = D * H * W
    levels, _, _ = VS.vol_case(6, K, S)
    bufs, (ptrs, ctot, f, fz) = _dev_levels(g, c, levels, 0, K, float("nan"))
    out = _Out(g, K, S, n)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                                   # noqa: E731
    good = dict(ptrs=ptrs, ctot=ctot, f=f, fz=fz, L=2, K=K, dhw=(D, H, W), labels=out.ptr("labels"), soft=out.ptr("soft"), acc=out.ptr("acc"))
    bad = [dict(K=0), dict(K=9), dict(L=0), dict(L=9), dict(ptrs=None), dict(ctot=None), dict(f=None), dict(fz=None), dict(labels=None),
           dict(acc=None), dict(ptrs=(ctypes.c_void_p * 2)(ptrs[0], None)), dict(f=ints(1, 0)), dict(fz=ints(0, 1)), dict(ctot=ints(3, 2)),
           dict(f=ints(1, 3)), dict(fz=ints(1, 3)), dict(dhw=(D, H, W + 1)), dict(dhw=(2048, 1024, 1024)), dict(dhw=(0, H, W))]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(_ffi.UzError):
            g.call("uz_vol_sample_accum", a["ptrs"], a["ctot"], a["f"], a["fz"], a["L"], a["K"], *a["dhw"], a["labels"], a["soft"], a["acc"], 1)
    for args in ((None, K, S, D, H, W, out.ptr("mean_soft"), None, None), (out.ptr("acc"), K, S, D, H, W, None, None, None),
                 (out.ptr("acc"), 0, S, D, H, W, out.ptr("mean_soft"), None, None), (out.ptr("acc"), 9, S, D, H, W, out.ptr("mean_soft"), None, None),
                 (out.ptr("acc"), K, 0, D, H, W, out.ptr("mean_soft"), None, None), (out.ptr("acc"), K, S, D, 0, W, out.ptr("mean_soft"), None, None),
                 (out.ptr("acc"), K, S, 2048, 1024, 1024, out.ptr("mean_soft"), None, None)):
        with pytest.raises(_ffi.UzError):
            g.call("uz_vol_sample_finish", *args)
    torch.cuda.synchronize()
    assert out.untouched()
    # ... and the null outputs of finish are optional: mean_soft alone
    g.call("uz_vol_sample_accum", ptrs, ctot, f, fz, 2, K, D, H, W, out.ptr("labels"), None, out.ptr("acc"), 1)
    g.call("uz_vol_sample_finish", out.ptr("acc"), K, S, D, H, W, out.ptr("mean_soft"), None, None)
    full = _run_pair(g, c, levels, K, S)
    assert torch.equal(out.body("mean_soft").view(K, D, H, W), full["mean_soft"]) and out.canaries_intact()
    assert bool((out.raw["mean_label"] == CANARY_B).all()) and bool((out.raw["entropy"] == CANARY_F).all()) and bool((out.raw["soft"] == CANARY_F).all())


# ------------------------------------------------------------------------------------------ model level
SAMPLES = 3


_state, _net = N.off_identity_state, N.small_phiseg3d


def _predict(net, c, eps=None, **kw):
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        out = net.predict(c.patch.to(dev), n_samples=c.S, eps=None if eps is None else [e.to(dev) for e in eps], **kw)
    torch.cuda.synchronize()
    return out


def _keep(net, out):
    return types.SimpleNamespace(labels=out.labels.clone(), mean_soft=out.mean_soft.clone(), mean_label=out.mean_label.clone(),
                                 entropy=out.entropy.clone(), soft=None if out.soft is None else out.soft.clone(),
                                 levels=None if out.levels is None else [t.clone() for t in out.levels],
                                 mu=[t.clone() for t in net.prior_mu], sigma=[t.clone() for t in net.prior_sigma],
                                 z=[t.clone() for t in net.prior_latent_space])


def _oracle(c):
    """Per sample the CPU oracle's prior pass and likelihood: the un-resized level logits and the last sample's moments."""
    lv = G.leaves(c.sd)
    s_in, last = [], None
    with torch.no_grad():
        for s in range(c.S):
            z, mu, sigma = R3.encoder3d(lv, "prior", c.patch, [e[s:s + 1] for e in c.eps], False)
            _, si = R3.likelihood3d(lv, z, False, c.dhw)
            s_in.append(si)
            last = dict(z=z, mu=mu, sigma=sigma)
    return s_in, last


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, the CPU oracle's answer and one predict() of a fresh net, shared by the tests of this fixture (read-only)."""
    arrays, meta = G.load(name)
    D, H, W = dhw = tuple(meta["dhw"])
    R, L, S = len(meta["filters"]), meta["latent_levels"], SAMPLES
    gen = torch.Generator().manual_seed(17 + L)
    eps = [torch.randn(*shape, generator=gen) for shape in R3.phiseg3d_eps_shapes(D, H, W, R, L, batch=S)]      # deepest level first
    c = types.SimpleNamespace(name=name, meta=meta, arrays=arrays, sd=_state(meta), patch=torch.from_numpy(arrays["patch"]), eps=eps, S=S,
                              L=L, K=meta["num_classes"], dhw=dhw)
    c.ref_s_in, c.ref_last = _oracle(c)
    c.net = _net(meta, c.sd)
    out = _predict(c.net, c, eps, return_soft=True, return_levels=True)
    c.out, c.bounds = _keep(c.net, out), c.net.check_bounds()
    return c


def _check_shapes(c, out):
    (D, H, W), S, K = c.dhw, c.S, c.K
    assert out.labels.shape == (S, 1, D, H, W) and out.labels.dtype == torch.uint8
    assert out.mean_soft.shape == (1, K, D, H, W) and out.mean_label.shape == (1, D, H, W) and out.mean_label.dtype == torch.uint8
    assert out.entropy.shape == (1, D, H, W)
    if out.soft is not None:
        assert out.soft.shape == (S, 1, K, D, H, W)
    if out.levels is not None:
        assert [tuple(t.shape) for t in out.levels] == [(S, 1, K, D >> l, H >> l, W >> l) for l in range(c.L)]


def _check_wiring(c, out):
    """labels / mean_soft / mean_label / entropy / soft = the twin of the statistics on predict's OWN level logits."""
    (D, H, W), S = c.dhw, c.S
    _check_shapes(c, out)
    vc = VS.Case(c.dhw, tuple((H // t.shape[-2], D // t.shape[-3]) for t in out.levels), 0, 0)
    tw = VS.vol_stats_twin(vc, [t[:, 0].cpu().numpy() for t in out.levels], S)
    assert np.array_equal(out.labels[:, 0].cpu().numpy(), tw["labels"]) and np.array_equal(out.mean_label[0].cpu().numpy(), tw["mean_label"])
    e = (G.maxabs(out.mean_soft[0].cpu().numpy(), tw["mean_soft"]), G.maxabs(out.entropy[0].cpu().numpy(), tw["entropy"]),
         G.maxabs(out.soft[:, 0].cpu().numpy(), tw["soft"]) if out.soft is not None else 0.0)
    print(f"predict3d {c.name} wiring: mean_soft {e[0]:.2e} entropy {e[1]:.2e} soft {e[2]:.2e}")
    assert e[0] <= P.mean_soft_tol(S) and e[1] <= P.ENTROPY_TOL and e[2] <= P.SOFT_TOL, e


def _check_vs_oracle(c, out):
    tol = lambda ref: 1e-4 * max(1.0, float(ref.abs().max()))                       # noqa: E731
    for l in range(c.L):
        for s in range(c.S):
            ref = c.ref_s_in[s][l]
            err = G.maxabs(out.levels[l][s].cpu().numpy(), ref.numpy())
            assert err <= tol(ref), ("s_in", l, s, err)
        errs = []
        for got, key in ((out.mu, "mu"), (out.sigma, "sigma"), (out.z, "z")):       # the last sample drawn
            ref = c.ref_last[key][l]
            assert got[l].shape == ref.shape, (key, l, got[l].shape, ref.shape)
            errs.append(G.maxabs(got[l].cpu().numpy(), ref.numpy()))
            assert errs[-1] <= tol(ref), (key, l, errs[-1])
        print(f"predict3d {c.name} level {l}: logits (last sample) {err:.2e} mu {errs[0]:.2e} sigma {errs[1]:.2e} z {errs[2]:.2e}")


@pytest.mark.parametrize("name", ["phiseg3d_small", "phiseg3d_l3"])
def test_predict3d_vs_cpu_oracle_and_wiring(name):
    c = _case(name)
    assert c.bounds == 0
    _check_vs_oracle(c, c.out)                                                      # (a)
    _check_wiring(c, c.out)                                                         # (b)


@pytest.mark.parametrize("name", ["phiseg3d_small", "phiseg3d_l3"])
def test_predict3d_vs_forward_in_eval_mode(name):
    """The parent commit's way: forward(patch, some mask, training=False) per sample - whose prior half must not depend on the mask."""
    c = _case(name)
    dev = torch.device("cuda", 0)
    net = _net(c.meta, c.sd)
    onehot = torch.from_numpy(c.arrays["mask_onehot"]).to(dev)
    masks = (onehot, onehot.flip(1))
    post = [torch.randn(1, *e.shape[1:], generator=torch.Generator().manual_seed(5 + k)) for k, e in enumerate(c.eps)]
    for s in range(c.S):
        eps = [t.to(dev) for t in post] + [e[s:s + 1].to(dev) for e in c.eps]
        runs = []
        for mask in masks:
            with torch.no_grad():
                runs.append([t.clone() for t in net.forward(c.patch.to(dev), mask, training=False, eps=eps)])
        for l in range(c.L):
            assert torch.equal(runs[0][l], runs[1][l]), (s, l)
            want = F.interpolate(c.out.levels[l][s], size=list(c.dhw), mode="nearest")
            e = G.maxabs(runs[0][l].cpu().numpy(), want.cpu().numpy())
            print(f"predict3d vs forward {name} sample {s} level {l}: {e:.2e}")
            assert runs[0][l].shape == want.shape and e <= 2e-4 * max(1.0, float(want.abs().max())), (s, l, e)
    assert net.check_bounds() == 0


def test_predict3d_gives_equal_noise_equal_samples():
    c = _case("phiseg3d_small")
    eps = [e[:1].repeat(c.S, 1, 1, 1, 1) for e in c.eps]
    out = _predict(c.net, c, eps, return_levels=True)
    for t in out.levels:
        assert all(torch.equal(t[s], t[0]) for s in range(1, c.S))
    assert all(torch.equal(out.labels[s], out.labels[0]) for s in range(1, c.S)) and out.soft is None
    assert all(torch.equal(a[0], b[0]) for a, b in zip(out.levels, c.out.levels))    # sample 0 had this noise in the shared run too
    assert c.net.check_bounds() == 0
    _check_wiring(c, out)


@pytest.mark.parametrize("graphs", [False, True])
def test_predict3d_is_repeatable_and_replays(graphs):
    """Four times the same eps -> the same bits, eager and under enable_graphs(True), equal to the shared eager run; plans are reused."""
    c = _case("phiseg3d_small")
    net = _net(c.meta, c.sd, graphs=graphs)
    for _ in range(4):
        out = _predict(net, c, c.eps, return_soft=True, return_levels=True)
        assert net.check_bounds() == 0
        assert all(torch.equal(a, b) for a, b in zip(out.levels, c.out.levels))
        assert torch.equal(out.labels, c.out.labels) and torch.equal(out.mean_soft, c.out.mean_soft) and torch.equal(out.soft, c.out.soft)
        assert torch.equal(out.mean_label, c.out.mean_label) and torch.equal(out.entropy, c.out.entropy)
    assert sorted(k[0] for k in net._plans) == ["draw", "trunk"]
    bare = _predict(net, c, c.eps)                                                  # neither soft nor levels: the same statistics
    assert bare.soft is None and bare.levels is None and torch.equal(bare.labels, c.out.labels) and torch.equal(bare.entropy, c.out.entropy)


def test_predict3d_draws_its_own_noise():
    c = _case("phiseg3d_small")
    net = _net(c.meta, c.sd)
    a = _keep(net, _predict(net, c, return_levels=True))
    b = _predict(net, c, return_levels=True)
    assert net.check_bounds() == 0
    assert not torch.equal(a.levels[0], b.levels[0]) and not torch.equal(a.mean_soft, b.mean_soft)
    assert all(not torch.equal(b.levels[0][s], b.levels[0][0]) for s in range(1, c.S))
    sh = len(c.meta["filters"]) - c.L                                             # latent level l lives sh + l halvings below the volume
    for lst in (net.prior_mu, net.prior_sigma, net.prior_latent_space):
        assert [tuple(t.shape) for t in lst] == [(1, 2, *(n >> (sh + l) for n in c.dhw)) for l in range(c.L)]
    _check_wiring(c, b)


def test_predict3d_errors_and_leaves_the_mode_alone():
    c = _case("phiseg3d_small")
    dev = torch.device("cuda", 0)
    net = _net(c.meta, c.sd)
    x = c.patch.to(dev)
    D, H, W = c.dhw
    with pytest.raises(NotImplementedError, match="one volume per call"):
        net.predict(torch.cat([x, x]))
    with pytest.raises(ValueError):
        net.predict(x, n_samples=0)
    with pytest.raises(ValueError):
        net.predict(x[..., :W - 1])
    with pytest.raises(ValueError):
        net.predict(x[:, :, :D - 2])
    with pytest.raises(ValueError):
        net.predict(x, n_samples=2, eps=[e[:2].to(dev) for e in c.eps][:1] * (c.L + 1))
    assert not net.training
    net.train()
    with pytest.raises(RuntimeError):
        net.predict(x)
    assert net.training
    rev = _net(c.meta, None, reversible=True)
    with pytest.raises(NotImplementedError):
        rev.predict(x)
    assert not rev.training
    assert all(torch.equal(v.cpu(), c.sd[k]) for k, v in c.net.state_dict().items())  # running statistics, counters: untouched by predict()


def test_harness_predict_hands_a_volume_batch_through(tmp_path):
    from unet_zoo_amd import train_model as TM
    from unet_zoo_amd.models.phiseg import Prediction
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    c = _case("phiseg3d_small")
    m = c.meta
    cfg = types.SimpleNamespace(experiment_name="t", log_dir_name="t", filter_channels=m["filters"], latent_levels=m["latent_levels"],
                                n_classes=m["num_classes"], no_convs_fcomb=3, beta=1.0, use_reversible=False, input_channels=m["input_channels"],
                                image_size=(m["input_channels"], *m["dhw"]), batch_size=1, iterations=2, logging_frequency=2, model=PHISeg3D)
    h = TM.UNetModel(cfg, log_root=str(tmp_path))
    h.net.load_state_dict(c.sd)
    h.net.train()
    h.net.set_rng_state(1234)
    a = h.predict(c.arrays["patch"], n_samples=2)                                   # (1, C, D, H, W) numpy
    assert type(a) is Prediction and not h.net.training and a.soft is None and a.levels is None
    keep = (a.labels.clone(), a.mean_soft.clone(), a.mean_label.clone(), a.entropy.clone())
    h.net.set_rng_state(1234)
    with torch.no_grad():
        b = h.net.predict(torch.from_numpy(c.arrays["patch"]).to(h.device), n_samples=2)
    assert a.labels.shape == (2, 1, *c.dhw)
    assert torch.equal(keep[0], b.labels) and torch.equal(keep[1], b.mean_soft) and torch.equal(keep[2], b.mean_label) and torch.equal(keep[3], b.entropy)


@pytest.mark.parametrize("name", ["phiseg3d_small", "phiseg3d_l3"])
def test_predict3d_with_every_convolution_on_the_split_kernels(name):
    """(a) and (b) once more under uz_set_conv_math(2); the gates are the same."""
    from unet_zoo_amd import _ffi
    c = _case(name)
    _ffi.lib().uz_set_conv_math(2)
    try:
        net = _net(c.meta, c.sd)
        out = _keep(net, _predict(net, c, c.eps, return_soft=True, return_levels=True))
        assert net.check_bounds() == 0
        packed = sum(len(p._packs["fwd"]) for p in net._plans.values())
    finally:
        _ffi.lib().uz_set_conv_math(-1)
    assert packed > 5
    _check_vs_oracle(c, out)
    _check_wiring(c, out)
