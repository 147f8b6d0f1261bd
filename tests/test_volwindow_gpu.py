"""Whole volumes from blended windows on the device: uz_vol_window_gather / _accum / _finish (csrc/volwindow.hip) on the cases of
tests/_volwindow.py - labels under the tie rule against the numpy twin, probabilities, their mean and the entropy against the
extended-precision reference within the gates of tests/_predict.py - and PHISeg3D.predict_volume against predict() per window,
against predict() on a single window, on the padded volume, and through the harness and metrics.score_volume.
The kernels read no arithmetic mode, so one mode suffices."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests import _nets as N
from tests import _volwindow as VW

pytestmark = pytest.mark.gpu

PAD = 64                                                                            # canary elements on either side of every buffer
CANARY_F, CANARY_B = -777.0, 255
FIELDS = ("labels", "soft", "mean_soft", "mean_label", "entropy")


def _dev():
    return torch.device("cuda", 0)


def _call(name, *args):
    """A C-ABI call on the current stream, not synchronised; tensors become device pointers."""
    from unet_zoo_amd import _ffi
    fn = getattr(_ffi.lib(), name)
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    assert len(conv) + 1 == len(fn.argtypes), name
    _ffi.check(fn(*conv, torch.cuda.current_stream().cuda_stream), name)


# ------------------------------------------------------------------------------------------ op level
class _Bufs:
    """Accumulators and outputs of one call sequence, each with PAD canary elements in front and behind."""

    def __init__(self, K, S, n, soft=True, mean_label=True, entropy=True):
        from tests import _gpu

        def buf(count, dtype):
            return _gpu.guarded(count, dtype, PAD, CANARY_B if dtype == torch.uint8 else CANARY_F)
        none = (None, None)
        bufs = dict(acc=buf(S * K * n, torch.float64), wsum=buf(n, torch.float64), labels=buf(S * n, torch.uint8),
                    soft=buf(S * K * n, torch.float32) if soft else none, mean_soft=buf(K * n, torch.float32),
                    mean_label=buf(n, torch.uint8) if mean_label else none, entropy=buf(n, torch.float32) if entropy else none)
        self.intact = _gpu.intact
        self.raw = {k: b[0] for k, b in bufs.items()}
        self.bodies = {k: b[1] for k, b in bufs.items()}

    def body(self, name):
        return self.bodies[name]

    def canaries_intact(self):
        return all(self.intact(t, self.bodies[k], CANARY_B if t.dtype == torch.uint8 else CANARY_F) for k, t in self.raw.items() if t is not None)


def _run_case(d, K, S, soft=True, mean_label=True, entropy=True, fill=float("nan")):
    """The call sequence of predict_volume on one case: per window, per sample one accum; one finish.  Level s of a window lives in a
    plan-layout volume [d_l + 2][K + extra][h_l][w_l] whose border slices and other channels hold `fill`."""
    c = d["c"]
    (D, H, W), (ed, eh, ew), dev = c.dhw, d["extent"], _dev()
    n, L = D * H * W, len(c.factors)
    b = _Bufs(K, S, n, soft, mean_label, entropy)
    b.body("acc").zero_()
    b.body("wsum").zero_()
    tabs = [torch.from_numpy(t).to(dev) for t in d["tables"]]
    ctot, f, fz = ((ctypes.c_int * L)(*v) for v in ([K + c.extra] * L, [q[0] for q in c.factors], [q[1] for q in c.factors]))
    held = []
    for o, levels in zip(d["origins"], d["wins"]):
        bufs = []
        for lv in levels:
            t = torch.full((S, lv.shape[2] + 2, K + c.extra, lv.shape[3], lv.shape[4]), fill, device=dev)
            t[:, 1:-1, c.c0:c.c0 + K] = torch.from_numpy(lv.copy()).permute(0, 2, 1, 3, 4).to(dev)
            bufs.append(t)
        held.append(bufs)
        for s in range(S):
            ptrs = (ctypes.c_void_p * L)(*[t[s, 1:, c.c0:].data_ptr() for t in bufs])
            _call("uz_vol_window_accum", ptrs, ctot, f, fz, L, K, ed, eh, ew, *o, D, H, W, *tabs, b.body("acc")[s * K * n:], b.body("wsum"), int(s == 0))
    _call("uz_vol_window_finish", b.body("acc"), b.body("wsum"), K, S, D, H, W, b.body("labels"), b.body("soft"), b.body("mean_soft"),
          b.body("mean_label"), b.body("entropy"))
    torch.cuda.synchronize()
    assert b.canaries_intact(), (VW.case_id(c), K, S)
    for bufs, levels in zip(held, d["wins"]):                                       # the logits are read, never written
        for t, lv in zip(bufs, levels):
            assert np.array_equal(t[:, 1:-1, c.c0:c.c0 + K].permute(0, 2, 1, 3, 4).cpu().numpy(), lv)
    for t, r in zip(tabs, d["tables"]):
        assert np.array_equal(t.cpu().numpy(), r)
    shapes = dict(labels=(S, D, H, W), soft=(S, K, D, H, W), mean_soft=(K, D, H, W), mean_label=(D, H, W), entropy=(D, H, W), acc=(S, K, D, H, W),
                  wsum=(D, H, W))
    return {k: None if b.raw[k] is None else b.body(k).view(shapes[k]).clone() for k in shapes}


def _np(r):
    return {k: None if v is None else v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("i", range(len(VW.CASES)), ids=[VW.case_id(c) for c in VW.CASES])
def test_window_accum_finish_vs_twin_and_reference(i):
    c = VW.CASES[i]
    for K in VW.STATS_K:
        for S in VW.STATS_S:
            for blend in VW.BLENDS:
                d = VW.case(i, K, S, blend)
                key = (VW.case_id(c), K, S, blend)
                got = _run_case(d, K, S)                                            # NaN around the operands
                failed, fig = VW.gates(_np(got), d["twin"], d["ref"], d["pins"], S)
                exempt = max(float(np.mean(~d["pins"][0][s])) for s in range(S))
                print(f"vol_window {key}: soft {fig['soft']:.2e} mean_soft {fig['mean_soft']:.2e} entropy {fig['entropy']:.2e} "
                      f"label mismatches {fig['labels']} + {fig['mean_label']}, exempt share {exempt:.4f}")
                assert not failed, (key, failed, fig)
                # the weight sum is what the windows laid down, whatever the sample count
                assert np.array_equal(got["wsum"].cpu().numpy(), _wsum(d)), key
                if (K, S) != (3, 3):
                    continue
                # a second call is bit-equal; a finite filler around the operands instead of NaN gives the same bits
                for again in (_run_case(d, K, S), _run_case(d, K, S, fill=3.0e30)):
                    assert all(torch.equal(got[k], again[k]) for k in got), key
                # nullable outputs left null do not change the others
                bare = _run_case(d, K, S, soft=False, mean_label=False, entropy=False)
                assert bare["soft"] is None and bare["mean_label"] is None and bare["entropy"] is None
                assert all(torch.equal(got[k], bare[k]) for k in ("labels", "mean_soft", "acc", "wsum")), key


def _wsum(d):
    """The weight sum of a case in fp64, the windows added in the order of the visits."""
    t = d["tables"]
    wt = (t[0][:, None, None] * t[1][None, :, None]) * t[2][None, None, :]
    out = np.zeros(d["c"].dhw)
    for o in d["origins"]:
        hi = [min(n - q, w) for n, q, w in zip(d["c"].dhw, o, d["extent"])]
        if min(hi) > 0:
            out[o[0]:o[0] + hi[0], o[1]:o[1] + hi[1], o[2]:o[2] + hi[2]] += wt[:hi[0], :hi[1], :hi[2]]
    return out


def test_a_voxel_no_window_reached_is_zero_not_nan():
    dev = _dev()
    K, S, n = 3, 2, 8
    acc, wsum = torch.zeros(S * K * n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    out = dict(labels=torch.full((S * n,), 9, dtype=torch.uint8, device=dev), soft=torch.full((S * K * n,), 9.0, device=dev),
               mean_soft=torch.full((K * n,), 9.0, device=dev), mean_label=torch.full((n,), 9, dtype=torch.uint8, device=dev),
               entropy=torch.full((n,), 9.0, device=dev))
    _call("uz_vol_window_finish", acc, wsum, K, S, 2, 2, 2, *[out[k] for k in FIELDS])
    torch.cuda.synchronize()
    assert all(bool((t == 0).all()) for t in out.values())


@pytest.mark.parametrize("ctot,c0", [(2, 0), (5, 2)])
def test_window_gather_is_a_zero_padded_crop(ctot, c0):
    dev, C = _dev(), 2
    for c in VW.CASES:
        _, extent, origins = VW.window_grid(c.dhw, c.window, c.stride, c.g)
        src = np.random.default_rng(sum(c.dhw)).standard_normal((C, *c.dhw)).astype(np.float32)
        src_d = torch.from_numpy(src).to(dev)
        for o in origins + [tuple(n + 3 for n in c.dhw)]:                           # ... and a window wholly beyond the volume: all zeros
            dst = torch.full((extent[0] + 2, ctot, extent[1], extent[2]), float("nan"), device=dev)
            _call("uz_vol_window_gather", src_d, C, *c.dhw, *o, dst[1:, c0:], ctot, *extent)
            torch.cuda.synchronize()
            want = VW.gather_twin(src, o, extent)
            assert np.array_equal(dst[1:-1, c0:c0 + C].permute(1, 0, 2, 3).cpu().numpy(), want), (VW.case_id(c), o)
            rest = torch.ones_like(dst, dtype=torch.bool)
            rest[1:-1, c0:c0 + C] = False
            assert bool(torch.isnan(dst[rest]).all())                               # border slices and the other channels: never written
        assert np.array_equal(src_d.cpu().numpy(), src)


# ------------------------------------------------------------------------------------------ model level
SAMPLES = 3
NETS = {"phiseg3d_small": dict(volume=(21, 18, 13), stride=(8, 8, 4)), "phiseg3d_l3": dict(volume=(13, 18, 21), stride=(4, 8, 8))}


_state, _net = N.off_identity_state, N.small_phiseg3d


def _eps_shapes(c, padded, S):
    R = len(c.meta["filters"])
    return [(S, 2, *(n >> (R - 1 - k) for n in padded)) for k in range(c.L)]        # deepest level first


def _randn(shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen).to(_dev()) for s in shapes]


def _fields(out):
    return dict(labels=out.labels[:, 0], soft=None if out.soft is None else out.soft[:, 0], mean_soft=out.mean_soft[0], mean_label=out.mean_label[0],
                entropy=out.entropy[0])


def _keep(out):
    return types.SimpleNamespace(**{k: None if getattr(out, k) is None else getattr(out, k).clone() for k in FIELDS}, levels=out.levels)


def _same(a, b, fields=FIELDS):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in fields if getattr(a, k) is not None and getattr(b, k) is not None)


def _volume(c, dhw, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(1, c.meta["input_channels"], *dhw, generator=gen) - 0.5).to(_dev())   # the value range of the fixtures' patch


def _pv(net, vol, **kw):
    with torch.no_grad():
        out = net.predict_volume(vol, **kw)
    torch.cuda.synchronize()
    return out


def _predict(net, patch, **kw):
    with torch.no_grad():
        out = net.predict(patch, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """The net, a volume larger than its window with injected global noise, and one predict_volume of it (shared, read-only)."""
    _, meta = G.load(name)
    c = types.SimpleNamespace(name=name, meta=meta, sd=_state(meta), S=SAMPLES, L=meta["latent_levels"], K=meta["num_classes"],
                              window=tuple(meta["dhw"]), g=1 << (len(meta["filters"]) - 1), **NETS[name])
    c.net = _net(meta, c.sd)
    c.vol = _volume(c, c.volume)
    c.padded, c.extent, c.origins = VW.window_grid(c.volume, c.window, c.stride, c.g)
    c.eps = _randn(_eps_shapes(c, c.padded, c.S), 17 + c.L)
    c.out = _keep(_pv(c.net, c.vol, n_samples=c.S, stride=c.stride, eps=c.eps, return_soft=True))
    c.bounds = c.net.check_bounds()
    return c


def _twin_of_windows(c, dhw, extent, origins, eps, blend, vol):
    """predict() per window on the zero-padded crop with the cropped noise; the twin on the level logits it returns."""
    R = len(c.meta["filters"])
    wins, factors = [], None
    for o in origins:
        crop = torch.from_numpy(VW.gather_twin(vol[0].cpu().numpy(), o, extent)).unsqueeze(0).to(_dev())
        noise = [e[:, :, o[0] >> (R - 1 - k):(o[0] + extent[0]) >> (R - 1 - k), o[1] >> (R - 1 - k):(o[1] + extent[1]) >> (R - 1 - k),
                   o[2] >> (R - 1 - k):(o[2] + extent[2]) >> (R - 1 - k)].contiguous() for k, e in enumerate(eps)]
        lv = _predict(c.net, crop, n_samples=c.S, eps=noise, return_levels=True).levels
        wins.append([t[:, 0].cpu().numpy() for t in lv])
        factors = tuple((extent[1] // t.shape[-2], extent[0] // t.shape[-3]) for t in lv)
    args = (dhw, extent, origins, VW.blend_tables(extent, blend), factors, wins, c.S)
    tw = VW.evaluate(*args, "twin")
    return tw, VW.must_match(dhw, extent, origins, factors, wins, c.S, tw, dt=np.float32)


def _check_against_twin(c, out, tw, pins, what):
    failed, fig = VW.gates(_np(_fields(out)), tw, tw, pins, c.S)
    exempt = max(float(np.mean(~pins[0][s])) for s in range(c.S))
    print(f"predict_volume {c.name} {what}: soft {fig.get('soft', 0):.2e} mean_soft {fig['mean_soft']:.2e} entropy {fig['entropy']:.2e} "
          f"label mismatches {fig['labels']} + {fig['mean_label']}, exempt share {exempt:.4f}")
    assert not failed, (c.name, what, failed, fig)
    assert exempt <= VW.EXEMPT_CAP


def _check_shapes(c, out, dhw, soft):
    S, K = c.S, c.K
    assert out.labels.shape == (S, 1, *dhw) and out.labels.dtype == torch.uint8
    assert out.mean_soft.shape == (1, K, *dhw) and out.mean_label.shape == (1, *dhw) and out.mean_label.dtype == torch.uint8
    assert out.entropy.shape == (1, *dhw) and out.levels is None
    assert (out.soft.shape == (S, 1, K, *dhw)) if soft else out.soft is None


@pytest.mark.parametrize("name", list(NETS))
def test_predict_volume_wiring(name):
    c = _case(name)
    assert len(c.origins) == 12 and c.bounds == 0
    _check_shapes(c, c.out, c.volume, True)
    tw, pins = _twin_of_windows(c, c.volume, c.extent, c.origins, c.eps, "gaussian", c.vol)
    _check_against_twin(c, c.out, tw, pins, "12 windows")
    assert {("trunk", *c.extent), ("draw", *c.extent)} <= set(c.net._plans) and {k[0] for k in c.net._plans} == {"trunk", "draw"}   # predict()'s plans
    again = _pv(c.net, c.vol, n_samples=c.S, stride=c.stride, eps=c.eps, return_soft=True)            # a second call is bit-equal
    assert _same(again, c.out)
    bare = _pv(c.net, c.vol, n_samples=c.S, stride=c.stride, eps=c.eps)
    _check_shapes(c, bare, c.volume, False)
    assert _same(bare, c.out)
    assert all(torch.equal(v.cpu(), c.sd[k]) for k, v in c.net.state_dict().items()) and c.net.check_bounds() == 0


@pytest.mark.parametrize("name", list(NETS))
def test_a_single_window_is_predict(name):
    c = _case(name)
    arrays, _ = G.load(name)
    patch = torch.from_numpy(arrays["patch"]).to(_dev())
    eps = _randn(_eps_shapes(c, c.window, c.S), 23)
    one = _keep(_predict(c.net, patch, n_samples=c.S, eps=eps, return_soft=True, return_levels=True))
    uni = _pv(c.net, patch, n_samples=c.S, blend="uniform", eps=eps, return_soft=True)
    assert _same(uni, one), name                                                    # bit for bit, every field
    gau = _pv(c.net, patch, n_samples=c.S, eps=eps, return_soft=True)
    wins = [[t[:, 0].cpu().numpy() for t in one.levels]]
    factors = tuple((c.window[1] // t.shape[-2], c.window[0] // t.shape[-3]) for t in one.levels)
    args = (c.window, c.window, [(0, 0, 0)], VW.blend_tables(c.window, "gaussian"), factors, wins, c.S)
    tw = VW.evaluate(*args, "twin")
    _check_against_twin(c, gau, tw, VW.must_match(c.window, c.window, [(0, 0, 0)], factors, wins, c.S, tw, dt=np.float32), "one window, gaussian")


def test_padding_only_is_predict_on_the_padded_volume():
    c = _case("phiseg3d_small")
    dhw, padded = (13, 10, 7), (16, 12, 8)
    vol = _volume(c, dhw, seed=6)
    eps = _randn(_eps_shapes(c, padded, c.S), 29)
    got = _pv(c.net, vol, n_samples=c.S, blend="uniform", eps=eps, return_soft=True)
    _check_shapes(c, got, dhw, True)
    big = torch.zeros(1, vol.shape[1], *padded, device=_dev())
    big[:, :, :13, :10, :7] = vol
    ref = _predict(_net(c.meta, c.sd), big, n_samples=c.S, eps=eps, return_soft=True)
    for k in FIELDS:
        assert torch.equal(getattr(got, k), getattr(ref, k)[..., :13, :10, :7]), k


def test_predict_volume_draws_coherent_noise_of_its_own():
    c = _case("phiseg3d_small")
    net = _net(c.meta, c.sd)
    a = _keep(_pv(net, c.vol, n_samples=c.S, stride=c.stride, return_soft=True))
    b = _pv(net, c.vol, n_samples=c.S, stride=c.stride, return_soft=True)
    assert not torch.equal(a.soft, b.soft) and not torch.equal(a.mean_soft, b.mean_soft)              # two calls differ
    assert all(not torch.equal(b.soft[s], b.soft[0]) for s in range(1, c.S))                         # the samples of a call differ
    net.set_rng_state(77)
    x = _keep(_pv(net, c.vol, n_samples=c.S, stride=c.stride, return_soft=True))
    net.set_rng_state(77)
    assert _same(_pv(net, c.vol, n_samples=c.S, stride=c.stride, return_soft=True), x)               # predict()'s generator
    assert net.check_bounds() == 0


def test_predict_volume_refusals_and_state():
    c = _case("phiseg3d_small")
    net = _net(c.meta, c.sd)
    with pytest.raises(ValueError):
        net.predict_volume(c.vol, window=(16, 16, 6))
    with pytest.raises(ValueError):
        net.predict_volume(c.vol, n_samples=c.S, eps=c.eps[:1])
    with pytest.raises(ValueError):
        net.predict_volume(c.vol, blend="cosine")
    net.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        net.predict_volume(c.vol)
    assert net.training and not net._plans
    rev = _net(c.meta, None, reversible=True)
    with pytest.raises(NotImplementedError, match="reversible"):
        rev.predict_volume(c.vol)
    assert all(torch.equal(v.cpu(), c.sd[k]) for k, v in c.net.state_dict().items())


def test_predict_volume_replays_graphs_bit_for_bit():
    c = _case("phiseg3d_small")
    net = _net(c.meta, c.sd, graphs=True)
    for _ in range(3):
        out = _pv(net, c.vol, n_samples=c.S, stride=c.stride, eps=c.eps, return_soft=True)
        assert _same(out, c.out) and net.check_bounds() == 0
    assert sorted(k[0] for k in net._plans) == ["draw", "trunk"]


def test_harness_routes_a_window_to_predict_volume(tmp_path):
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
    a = h.predict(c.vol.cpu().numpy(), n_samples=2, window=c.window, stride=c.stride, blend="uniform")
    assert type(a) is Prediction and not h.net.training and a.soft is None and a.levels is None and a.labels.shape == (2, 1, *c.volume)
    keep = _keep(a)
    h.net.set_rng_state(1234)
    b = _pv(h.net, c.vol, n_samples=2, window=c.window, stride=c.stride, blend="uniform")
    assert _same(keep, b, ("labels", "mean_soft", "mean_label", "entropy"))
    assert not _same(keep, _pv(h.net, c.vol, n_samples=2, window=c.window, stride=c.stride), ("mean_soft",))   # the blend is handed on


def test_a_prediction_of_a_volume_goes_into_score_volume():
    from unet_zoo_amd import metrics
    c = _case("phiseg3d_small")
    out = _pv(c.net, c.vol, n_samples=c.S, stride=c.stride, eps=c.eps)
    gen = torch.Generator().manual_seed(3)
    ref = torch.randint(0, c.K, c.volume, generator=gen, dtype=torch.uint8).to(_dev())
    regions = ((1, 2), (1,), (2,))
    sc = metrics.score_volume(out, ref, regions, hd95=True)
    torch.cuda.synchronize()
    assert tuple(sc.dice.shape) == tuple(sc.hd95.shape) == (c.S + 1, len(regions)) and tuple(sc.counts.shape) == (c.S + 1, len(regions), 4)
    assert not bool(torch.isnan(sc.hd95).any()) and bool(((sc.dice >= 0) & (sc.dice <= 1)).all())
    assert bool((sc.counts[:, :, 3] == int(np.prod(c.volume))).all())
    rows = torch.cat([out.labels[:, 0], out.mean_label], 0).cpu().numpy()
    for n in range(c.S + 1):
        for r, reg in enumerate(regions):
            assert int(sc.counts[n, r, 1]) == int(np.isin(rows[n], reg).sum())
