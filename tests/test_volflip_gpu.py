"""Mirrored passes of PHISeg3D.predict_volume on the device: uz_vol_window_gather_ex / uz_vol_window_noise byte for byte against the
numpy twins of tests/_volflip.py, uz_vol_window_accum_ex against the old call (flip = 0), against torch.flip of the old call (one
window that is the whole volume) and, over windows x masks, against the twin through the gates of tests/_volwindow.py; the refusals;
and predict_volume(flips=...) end to end on the small model.  The kernels read no arithmetic mode; the end-to-end tests compare
the model with itself, so they hold in every mode."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests import _gpu
from tests import _nets as N
from tests import _volflip as VF

pytestmark = pytest.mark.gpu

IDS = [VF.case_id(c) for c in VF.CASES]
FIELDS = ("labels", "soft", "mean_soft", "mean_label", "entropy")
SENTINEL = _gpu.CANARY[torch.float32]


def _call(name, *args):
    """A C-ABI call on the current stream, not synchronised; tensors become device pointers.  Returns the call's status."""
    from unet_zoo_amd import _ffi
    fn = getattr(_ffi.lib(), name)
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    assert len(conv) + 1 == len(fn.argtypes), name
    return fn(*conv, torch.cuda.current_stream().cuda_stream)


def _ok(name, *args):
    from unet_zoo_amd import _ffi
    _ffi.check(_call(name, *args), name)


class _Slice:
    """The C-channel slice at channel c0 of a plan volume [n + 2][ctot][h][w] inside a guarded buffer, everything holding the sentinel;
    `off` moves the volume that many elements off the buffer's 16-byte boundary."""

    def __init__(self, n, C, h, w, ctot, c0, off):
        self.raw, body = _gpu.guarded((n + 2) * ctot * h * w, torch.float32, off=off)
        self.vol = body.view(n + 2, ctot, h, w)
        self.ptr, self.C, self.c0 = self.vol[1:, c0:], C, c0

    def reset(self):
        self.raw.fill_(SENTINEL)

    def written(self):
        """(C, n, h, w) as numpy - after checking that nothing but the slice was written."""
        assert _gpu.intact(self.raw, self.vol)
        rest = torch.ones_like(self.vol, dtype=torch.bool)
        rest[1:-1, self.c0:self.c0 + self.C] = False
        assert bool((self.vol[rest] == SENTINEL).all())
        return self.vol[1:-1, self.c0:self.c0 + self.C].permute(1, 0, 2, 3).contiguous().cpu().numpy()


def _side_stream(i):
    """Every other case runs on a second stream."""
    if i % 2 == 0:
        return torch.cuda.stream(torch.cuda.current_stream())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    return torch.cuda.stream(side)


# ------------------------------------------------------------------------------------------ gather and noise
@pytest.mark.parametrize("i", range(len(VF.CASES)), ids=IDS)
def test_gather_ex_equals_the_twin_byte_for_byte(i):
    c = VF.CASES[i]
    padded, extent, origins = VF.window_grid(c.dhw, c.window, c.stride, c.g)
    C = 2
    src = VF.ramp_noise((C, *c.dhw), 11 + i)
    with _side_stream(i):
        src_d = torch.from_numpy(src).to(_gpu.dev())
        new, old = (_Slice(extent[0], C, extent[1], extent[2], C + c.extra, c.c0, off) for off in (1 + i % 3, 0))
        for o in origins + [tuple(n + 3 for n in c.dhw)]:                           # ... and a window wholly beyond the volume: all zeros
            for m in VF.ALL:
                new.reset()
                _ok("uz_vol_window_gather_ex", src_d, C, *c.dhw, *o, new.ptr, C + c.extra, *extent, m)
                got = new.written()
                assert got.tobytes() == VF.gather_flip(src, o, extent, m, padded=padded).tobytes(), (IDS[i], o, m)
                if m == 0:
                    old.reset()
                    _ok("uz_vol_window_gather", src_d, C, *c.dhw, *o, old.ptr, C + c.extra, *extent)
                    assert old.written().tobytes() == got.tobytes(), (IDS[i], o)
        assert np.array_equal(src_d.cpu().numpy(), src)
        torch.cuda.current_stream().synchronize()


@pytest.mark.parametrize("i", range(len(VF.CASES)), ids=IDS)
def test_noise_equals_the_twin_byte_for_byte(i):
    c = VF.CASES[i]
    padded, extent, origins = VF.window_grid(c.dhw, c.window, c.stride, c.g)
    with _side_stream(i + 1):
        for l, fac in enumerate(c.factors):
            size, _, ext, _ = VF.level_geometry(c, padded, extent, origins[0], fac)
            field = VF.ramp_noise((3, 2, *size), 23 + l)                            # three samples' rows; the call takes one
            field_d = torch.from_numpy(field).to(_gpu.dev())
            dst = _Slice(ext[0], 2, ext[1], ext[2], 2 + c.extra, c.c0, (i + l) % 4)
            for o in origins:
                _, lo, _, _ = VF.level_geometry(c, padded, extent, o, fac)
                for m in VF.ALL:
                    dst.reset()
                    _ok("uz_vol_window_noise", field_d[1], 2, *size, *lo, *ext, m, dst.ptr, 2 + c.extra)
                    got = dst.written()
                    assert got.tobytes() == VF.noise_crop(field[1], lo, ext, m).tobytes(), (IDS[i], l, o, m)
                    if m == 0:                                                      # today's slice-and-copy (PHISeg3D._draw)
                        crop = field_d[1:2, :, lo[0]:lo[0] + ext[0], lo[1]:lo[1] + ext[1], lo[2]:lo[2] + ext[2]]
                        dst.reset()
                        dst.vol[1:-1, c.c0:c.c0 + 2].copy_(crop[0].permute(1, 0, 2, 3))
                        assert dst.written().tobytes() == got.tobytes(), (IDS[i], l, o)
            assert np.array_equal(field_d.cpu().numpy(), field)
        torch.cuda.current_stream().synchronize()


# ------------------------------------------------------------------------------------------ accumulate
def _run(c, extent, origins, masks, tables, pass_levels, K, S, old=False, fill=float("nan")):
    """The call sequence of predict_volume(flips=masks): per window, per mask, per sample one accum; one finish.  The levels of a pass
    live in plan-layout volumes [d_l + 2][K + extra][h_l][w_l] whose border slices and other channels hold `fill`.  old: the
    unmirrored entry point (masks must be (0,)).  Guarded accumulators and outputs; acc one element off its 16-byte boundary."""
    (D, H, W), (ed, eh, ew), dev = c.dhw, extent, _gpu.dev()
    n, L = D * H * W, len(c.factors)
    bufs = dict(acc=_gpu.guarded(S * K * n, torch.float64, off=1), wsum=_gpu.guarded(n, torch.float64), labels=_gpu.guarded(S * n, torch.uint8),
                soft=_gpu.guarded(S * K * n, torch.float32), mean_soft=_gpu.guarded(K * n, torch.float32), mean_label=_gpu.guarded(n, torch.uint8),
                entropy=_gpu.guarded(n, torch.float32))
    b = {k: v[1] for k, v in bufs.items()}
    b["acc"].zero_()
    b["wsum"].zero_()
    tabs = [torch.from_numpy(t).to(dev) for t in tables]
    ctot, f, fz = ((ctypes.c_int * L)(*v) for v in ([K + c.extra] * L, [q[0] for q in c.factors], [q[1] for q in c.factors]))
    held = []
    for i, o in enumerate(origins):
        for j, m in enumerate(masks):
            lv_d = []
            for lv in pass_levels[i][j]:
                t = torch.full((S, lv.shape[2] + 2, K + c.extra, lv.shape[3], lv.shape[4]), fill, device=dev)
                t[:, 1:-1, c.c0:c.c0 + K] = torch.from_numpy(lv.copy()).permute(0, 2, 1, 3, 4).to(dev)
                lv_d.append(t)
            held.append(lv_d)
            for s in range(S):
                ptrs = (ctypes.c_void_p * L)(*[t[s, 1:, c.c0:].data_ptr() for t in lv_d])
                head = (ptrs, ctot, f, fz, L, K, ed, eh, ew, *o, D, H, W, *tabs, b["acc"][s * K * n:], b["wsum"], int(s == 0))
                if old:
                    assert m == 0
                    _ok("uz_vol_window_accum", *head)
                else:
                    _ok("uz_vol_window_accum_ex", *head, m)
    _ok("uz_vol_window_finish", b["acc"], b["wsum"], K, S, D, H, W, b["labels"], b["soft"], b["mean_soft"], b["mean_label"], b["entropy"])
    torch.cuda.current_stream().synchronize()
    assert all(_gpu.intact(raw, body) for raw, body in bufs.values()), (VF.case_id(c), K)
    shapes = dict(labels=(S, D, H, W), soft=(S, K, D, H, W), mean_soft=(K, D, H, W), mean_label=(D, H, W), entropy=(D, H, W), acc=(S, K, D, H, W),
                  wsum=(D, H, W))
    return {k: b[k].view(shapes[k]).clone() for k in shapes}


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("i", range(len(VF.CASES)), ids=IDS)
def test_accum_ex_without_a_mirror_is_the_old_call_bit_for_bit(i):
    c = VF.CASES[i]
    for K in VF.STATS_K:
        d = VF.case(i, K)
        first = [[w[0]] for w in d["levels"]]
        with _side_stream(i):
            new = _run(c, d["extent"], d["origins"], (0,), d["tables"], first, K, c.S)
            old = _run(c, d["extent"], d["origins"], (0,), d["tables"], first, K, c.S, old=True)
        assert all(torch.equal(new[k], old[k]) for k in new), (IDS[i], K)


@pytest.mark.parametrize("K", VF.STATS_K)
def test_one_window_mirrored_is_torch_flip_of_the_old_call(K):
    """Case 0: one window that is the whole volume.  With symmetric weight tables the mirrored pass adds, voxel by voxel, what the
    unmirrored pass adds at the mirror image - the same products of the same operands."""
    c, d = VF.CASES[0], VF.case(0, K)
    assert d["origins"] == [(0, 0, 0)] and d["extent"] == c.dhw
    tables = VF.blend_tables(d["extent"], "gaussian")
    assert all(np.array_equal(t, t[::-1]) for t in tables)
    one = [[d["levels"][0][0]]]
    old = _run(c, d["extent"], d["origins"], (0,), tables, one, K, c.S, old=True)
    for m in VF.ALL:
        new = _run(c, d["extent"], d["origins"], (m,), tables, one, K, c.S)
        assert all(torch.equal(new[k], VF.mirrored(old[k], m)) for k in new), (K, m)


@pytest.mark.parametrize("i", range(len(VF.CASES)), ids=IDS)
def test_accum_ex_over_windows_and_masks_vs_twin_and_reference(i):
    c = VF.CASES[i]
    for K in VF.STATS_K:
        d = VF.case(i, K)
        with _side_stream(i + 1):
            got = _run(c, d["extent"], d["origins"], d["masks"], d["tables"], d["levels"], K, c.S)
        failed, fig = VF.gates(_np(got), d["twin"], d["ref"], d["pins"], c.S)
        exempt = max(float(np.mean(~d["pins"][0][s])) for s in range(c.S))
        print(f"vol_window flips {IDS[i]} K={K}: soft {fig['soft']:.2e} mean_soft {fig['mean_soft']:.2e} entropy {fig['entropy']:.2e} "
              f"label mismatches {fig['labels']} + {fig['mean_label']}, exempt share {exempt:.4f}")
        assert not failed, (IDS[i], K, failed, fig)
        assert exempt <= VF.EXEMPT_CAP
        assert np.array_equal(got["wsum"].cpu().numpy(), d["twin"]["wsum"]), (IDS[i], K)       # one add per (window, mask), in their order
        if K == 3:                                                                  # a second run is bit-equal, whatever surrounds the operands
            again = _run(c, d["extent"], d["origins"], d["masks"], d["tables"], d["levels"], K, c.S, fill=3.0e30)
            assert all(torch.equal(got[k], again[k]) for k in got), (IDS[i], K)


def test_a_refused_call_leaves_the_outputs_untouched():
    from unet_zoo_amd import _ffi
    dev, L = _gpu.dev(), _ffi.lib()
    src = torch.zeros(2 * 5 * 6 * 7, device=dev)
    dst = torch.full((6 * 2 * 4 * 4,), SENTINEL, device=dev)
    acc = torch.full((3 * 5 * 6 * 7,), SENTINEL, dtype=torch.float64, device=dev)
    wsum = torch.full((5 * 6 * 7,), SENTINEL, dtype=torch.float64, device=dev)
    lv = torch.zeros(6 * 3 * 4 * 4, device=dev)
    tab = torch.ones(4, dtype=torch.float64, device=dev)
    one = lambda v: (ctypes.c_int * 1)(v)                                           # noqa: E731
    ptrs = (ctypes.c_void_p * 1)(lv.data_ptr())
    accum = lambda flip, win=(4, 4, 4): _call("uz_vol_window_accum_ex", ptrs, one(3), one(1), one(1), 1, 3, *win, 0, 0, 0, 5, 6, 7, tab, tab, tab,   # noqa: E731
                                              acc, wsum, 1, flip)
    refused = [
        _call("uz_vol_window_gather_ex", src, 2, 5, 6, 7, 0, 0, 0, dst, 2, 4, 4, 4, 8),                # the mask
        _call("uz_vol_window_gather_ex", src, 2, 5, 6, 7, 0, 0, 0, dst, 2, 4, 4, 4, -1),
        _call("uz_vol_window_gather_ex", src, 2, 5, 6, 7, 0, -4, 0, dst, 2, 4, 4, 4, 7),               # an origin below 0
        _call("uz_vol_window_noise", src, 2, 5, 6, 7, 0, 0, 0, 4, 4, 4, 8, dst, 2),
        _call("uz_vol_window_noise", src, 2, 5, 6, 7, 2, 0, 0, 4, 4, 4, 1, dst, 2),                    # the crop leaves its field
        _call("uz_vol_window_noise", src, 2, 5, 6, 7, 0, 0, 4, 4, 4, 4, 4, dst, 2),
        _call("uz_vol_window_noise", src, 2, 5, 6, 7, 0, 0, 0, 4, 0, 4, 2, dst, 2),                    # an empty crop
        _call("uz_vol_window_noise", None, 2, 5, 6, 7, 0, 0, 0, 4, 4, 4, 2, dst, 2),                   # a null pointer
        accum(8), accum(-2), accum(3, (4, 4, 0)),
    ]
    assert refused == [-1] * len(refused), refused
    assert _call("uz_vol_window_noise", src, 2, 5, 6, 7, 2, 0, 0, 4, 4, 4, 1, dst, 2) == -1 and b"leaves its field" in L.uz_last_error()
    assert accum(8) == -1 and b"flip" in L.uz_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (dst, acc, wsum))


# ------------------------------------------------------------------------------------------ model level
NAME, VOLUME, STRIDE, S = "phiseg3d_small", (21, 18, 13), (8, 8, 4), 2


def _randn(shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen).to(_gpu.dev()) for s in shapes]


def _volume(m, dhw, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(1, m.meta["input_channels"], *dhw, generator=gen) - 0.5).to(_gpu.dev())


def _eps_shapes(m, padded, S_):
    R = len(m.meta["filters"])
    return [(S_, 2, *(n >> (R - 1 - k) for n in padded)) for k in range(m.meta["latent_levels"])]       # deepest level first


def _pv(net, vol, **kw):
    with torch.no_grad():
        out = net.predict_volume(vol, **kw)
    torch.cuda.synchronize()
    return types.SimpleNamespace(**{k: None if getattr(out, k) is None else getattr(out, k).clone() for k in FIELDS})


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in FIELDS)


@functools.lru_cache(maxsize=None)
def _model():
    """The small net, a volume larger than its window (12 windows) with injected noise, and a volume that is exactly one window."""
    _, meta = G.load(NAME)
    m = types.SimpleNamespace(meta=meta, sd=N.off_identity_state(meta), window=tuple(meta["dhw"]), g=1 << (len(meta["filters"]) - 1))
    m.net = N.small_phiseg3d(meta, m.sd)
    m.vol = _volume(m, VOLUME, 5)
    m.padded, m.extent, m.origins = VF.window_grid(VOLUME, m.window, STRIDE, m.g)
    assert len(m.origins) == 12
    m.eps = _randn(_eps_shapes(m, m.padded, S), 41)
    m.kw = dict(n_samples=S, stride=STRIDE, eps=m.eps, return_soft=True)
    m.one = _volume(m, m.window, 6)
    m.one_eps = _randn(_eps_shapes(m, m.window, S), 43)
    return m


def test_flips_none_and_the_unmirrored_mask_alone_are_bit_equal():
    m = _model()
    plain = _pv(m.net, m.vol, **m.kw)
    assert _same(plain, _pv(m.net, m.vol, flips=(0,), **m.kw))
    assert _same(plain, _pv(m.net, m.vol, flips=None, **m.kw))
    assert not _same(plain, _pv(m.net, m.vol, flips=(0, 7), **m.kw)) and m.net.check_bounds() == 0


@pytest.mark.parametrize("mask", (1, 2, 4, 7))
def test_one_window_under_a_mask_is_the_mirrored_call_mirrored_back(mask):
    """predict_volume(v, flips=(m,)) == flip(predict_volume(flip(v), eps=flip(eps))), bit for bit: on a volume that is exactly one
    window, and on one shorter than its padded extent - the mirror is about the WINDOW, so the host pads with zeros first, mirrors,
    and crops after mirroring back."""
    m = _model()
    got = _pv(m.net, m.one, n_samples=S, eps=m.one_eps, return_soft=True, flips=(mask,))
    ref = _pv(m.net, VF.mirrored(m.one, mask).contiguous(), n_samples=S, eps=[VF.mirrored(e, mask).contiguous() for e in m.one_eps], return_soft=True)
    for k in FIELDS:
        assert torch.equal(getattr(got, k), VF.mirrored(getattr(ref, k), mask)), (mask, k)
    dhw, padded = (13, 10, 7), (16, 12, 8)
    assert VF.window_grid(dhw, m.window, None, m.g) == (padded, padded, [(0, 0, 0)])
    vol, eps = _volume(m, dhw, 7), _randn(_eps_shapes(m, padded, S), 47)
    got = _pv(m.net, vol, n_samples=S, eps=eps, return_soft=True, flips=(mask,))
    big = torch.zeros(1, vol.shape[1], *padded, device=_gpu.dev())
    big[:, :, :13, :10, :7] = vol
    ref = _pv(m.net, VF.mirrored(big, mask).contiguous(), n_samples=S, eps=[VF.mirrored(e, mask).contiguous() for e in eps], return_soft=True)
    for k in FIELDS:
        assert torch.equal(getattr(got, k), VF.mirrored(getattr(ref, k), mask)[..., :13, :10, :7]), (mask, k)


def test_all_masks_repeat_bit_for_bit():
    m = _model()
    a = _pv(m.net, m.vol, flips="all", **m.kw)
    assert _same(a, _pv(m.net, m.vol, flips="all", **m.kw)) and _same(a, _pv(m.net, m.vol, flips=range(8), **m.kw))
    assert not _same(a, _pv(m.net, m.vol, **m.kw)) and m.net.check_bounds() == 0
    assert float(a.soft.sum(dim=2).sub(1).abs().max()) < 1e-6                        # the weight sum took every (window, mask) pair


def test_two_masks_are_the_mean_of_the_single_mask_calls():
    """Both masks lay the same weight on a voxel, so p_ab = (p_a + p_b) / 2 exactly; the fp64 paths differ by a few 2^-53 relative,
    the fp32 rounding of the result is at most 2^-24 and the mean of two rounded inputs at most 2^-25 off: within 2^-23."""
    m = _model()
    worst = 0.0
    for a, b in ((0, 7), (3, 4), (5, 6)):
        both = _pv(m.net, m.vol, flips=(a, b), **m.kw).soft.double()
        mean = (_pv(m.net, m.vol, flips=(a,), **m.kw).soft.double() + _pv(m.net, m.vol, flips=(b,), **m.kw).soft.double()) / 2
        err = float((both - mean).abs().max())
        print(f"flips=({a}, {b}) against the mean of the single-mask calls: max |difference| {err:.3e} (bound {2.0 ** -23:.3e})")
        worst = max(worst, err)
    assert worst <= 2.0 ** -23


def test_harness_hands_flips_to_predict_volume(tmp_path):
    from unet_zoo_amd import train_model as TM
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    m = _model()
    q = m.meta
    cfg = types.SimpleNamespace(experiment_name="t", log_dir_name="t", filter_channels=q["filters"], latent_levels=q["latent_levels"],
                                n_classes=q["num_classes"], no_convs_fcomb=3, beta=1.0, use_reversible=False, input_channels=q["input_channels"],
                                image_size=(q["input_channels"], *q["dhw"]), batch_size=1, iterations=2, logging_frequency=2, model=PHISeg3D)
    h = TM.UNetModel(cfg, log_root=str(tmp_path))
    h.net.load_state_dict(m.sd)
    h.net.set_rng_state(1234)
    a = h.predict(m.vol.cpu().numpy(), n_samples=2, window=m.window, stride=STRIDE, flips="all")
    keep = {k: getattr(a, k).clone() for k in FIELDS if k != "soft"}
    h.net.set_rng_state(1234)
    b = _pv(h.net, m.vol, n_samples=2, window=m.window, stride=STRIDE, flips="all")
    assert all(torch.equal(keep[k], getattr(b, k)) for k in keep)
    h.net.set_rng_state(1234)
    assert not torch.equal(keep["mean_soft"], _pv(h.net, m.vol, n_samples=2, window=m.window, stride=STRIDE).mean_soft)   # the masks are handed on
    with pytest.raises(ValueError, match="window"):
        h.predict(m.vol.cpu().numpy(), n_samples=2, flips="all")
