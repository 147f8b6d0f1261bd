"""PHiSeg3D on the native HIP path - counterpart of the reference ``models/phiseg3D.py`` ``PHISeg3D`` (constructor keywords
:413-425; ``forward(patch, mask, training)`` :454-467; the same loss helpers as the 2-D model :469-611): Conv3d 3x3x3 +
BatchNorm3d + ReLU units (:13-35), AvgPool3d(2, ceil) (:101), trilinear x2 with align_corners=True (:146,306,376), 1x1x1 latent
heads (:184-186), optional ReversibleSequence with reversible_depth 1 (:61-86,104,142,176,341,352), resolution levels =
len(num_filters) and `latent_levels` free (:245-248 - unlike the 2-D model nothing is hard-wired to 7 / 5).  The plan builder and the
reference API on top of a plan are shared with PHISeg (models/_hier.py); this file holds the 3-D geometry and the volume staging.

First slice, with these limits stated up front:
  * ONE sample per call (the reference's BraTS experiment runs batch_size 1, phiseg_brats.py:28): a volume is held as
    [D + 2][C][H][W], i.e. its depth slices are the batch of the 2-D kernels (csrc/vol.hip, _plan.Plan.vol);
  * fp32 storage; the 3x3x3 convolutions run on the split-fp16 matrix-pipe kernels of the 2-D path with K = 27 Cin (BASELINE
    config 5 asks for bf16 storage, which would make the model HBM-bound: next);
  * the reference's own forward raises at its last line (:398 hands a 2-element `size` to a 5-D `interpolate`); the evident
    intent - nearest resize of every level to the full volume - is what runs here, and parity is pinned on everything up to
    the un-resized level logits `s_in` (Posterior, prior, Likelihood), which the reference does execute.
Beyond the reference: predict(patch, n_samples) - samples, mean probabilities and an uncertainty map of a volume without a label mask -
and predict_volume(volume, n_samples, window, stride, blend): the same for a volume of any size, from blended windows.
"""
import ctypes as C
import operator

import torch

from .. import _ffi
from ._hier import HierarchicalModel, hier_spec, lift3
from .phiseg import Prediction


def phiseg3d_spec(input_channels, num_classes, num_filters, latent_levels, reversible=False):
    nf = list(num_filters)
    return lift3(hier_spec(input_channels, num_classes, num_classes, nf, len(nf), latent_levels, reversible, PHISeg3D.rev_depths))


BLENDS = ("gaussian", "uniform")


def default_stride(window, g):
    """Half the window per axis, rounded down to a multiple of g, and at least g."""
    return tuple(max(g, (int(w) // 2) // g * g) for w in window)


def window_grid(dhw, window, stride, g):
    """The windows predict_volume() visits on a volume of size dhw = (D, H, W); pure host arithmetic.  g = 2^(levels-1): what every
    side of a plan's volume must divide by.  window: three positive multiples of g; stride: three multiples of g with
    g <= stride <= window, or None for default_stride.  Per axis of length n, with P = ceil(n / g) g: if P <= w ONE window of extent P
    at origin 0 (the window shrinks); else windows of extent w at 0, s, 2s, ... < P - w and at P - w.  Returns (padded, extent,
    origins): the padded size (P_D, P_H, P_W), the extent of every window and the origins (oz, oy, ox) in the order of the visits - D
    slowest, W fastest.  Every origin is a multiple of g, the windows cover the padded volume and the last one of an axis ends at P."""
    if g < 1 or g & (g - 1):
        raise ValueError(f"window_grid: g must be a power of two, got {g}")
    if len(dhw) != 3 or any(int(n) < 1 for n in dhw):
        raise ValueError(f"window_grid: the volume needs three sides >= 1, got {tuple(dhw)}")
    if window is None or len(window) != 3 or any(int(w) != w or w < g or w % g for w in window):
        raise ValueError(f"window_grid: every side of the window must be a positive multiple of {g}, got {window}")
    window = tuple(int(w) for w in window)
    if stride is None:
        stride = default_stride(window, g)
    if len(stride) != 3 or any(int(s) != s or s % g or s < g or s > w for s, w in zip(stride, window)):
        raise ValueError(f"window_grid: every stride must be a multiple of {g} with {g} <= stride <= window {window}, got {tuple(stride)}")
    padded, extent, axes = [], [], []
    for n, w, s in zip(dhw, window, stride):
        P = -(-int(n) // g) * g
        padded.append(P)
        if P <= w:
            extent.append(P)
            axes.append([0])
        else:
            extent.append(w)
            axes.append(list(range(0, P - w, int(s))) + [P - w])
    return tuple(padded), tuple(extent), [(z, y, x) for z in axes[0] for y in axes[1] for x in axes[2]]


def blend_tables(extent, blend):
    """Per axis the fp64 weight table of a window of this extent: "gaussian" t[i] = exp(-0.5 ((i - (w - 1) / 2) / (w / 8))^2),
    "uniform" t[i] = 1.  A voxel's weight is (tz * ty) * tx."""
    import numpy as np
    if blend not in BLENDS:
        raise ValueError(f"blend must be one of {BLENDS}, got {blend!r}")
    out = []
    for w in extent:
        i = np.arange(int(w), dtype=np.float64)
        out.append(np.exp(-0.5 * ((i - (w - 1) / 2.0) / (w / 8.0)) ** 2) if blend == "gaussian" else np.ones(int(w), np.float64))
    return out


def flip_masks(flips):
    """The flip masks of predict_volume(flips=...) in the order of the passes: "all" -> 0 .. 7; else a non-empty sequence of distinct
    ints in 0 .. 7 (bit 0, 1, 2 mirror D, H, W).  Anything else is a ValueError."""
    if isinstance(flips, str) and flips == "all":
        return tuple(range(8))
    try:
        if isinstance(flips, str) or any(isinstance(m, bool) for m in flips):
            raise TypeError
        masks = tuple(operator.index(m) for m in flips)
    except TypeError:
        masks = ()
    if not masks or any(not 0 <= m <= 7 for m in masks) or len(set(masks)) != len(masks):
        raise ValueError(f'flips must be None, "all" or a non-empty sequence of distinct integer masks in 0 .. 7, got {flips!r}')
    return masks


class PHISeg3D(HierarchicalModel):
    rev_depths = (1, 1)        # reversible_depth 1 everywhere (phiseg3D.py:61-86)

    def __init__(self, input_channels, num_classes, num_filters, latent_levels=5, initializers=None, no_convs_fcomb=4, beta=10.0,
                 image_size=(128, 128, 1), reversible=False, apply_last_layer=True, exponential_weighting=True, padding=True, device=None):
        if len(num_filters) < latent_levels:
            raise ValueError("PHISeg3D needs at least `latent_levels` filters")
        diff = len(num_filters) - latent_levels
        if latent_levels > 1 and num_filters[latent_levels - 1] != num_filters[latent_levels - 1 + diff]:
            # likelihood_post_c_path's first convolution is built for num_filters[i] + num_filters[i + 1 + lvl_diff] inputs
            # (:343) but is fed post_z[latent_levels - 1], which has num_filters[latent_levels - 1] channels (:372): the
            # reference raises on such a configuration at its first forward pass
            raise ValueError("PHISeg3D: num_filters[latent_levels-1] must equal num_filters[-1] (reference channel arithmetic, phiseg3D.py:343,372)")
        # the reference's Posterior concatenates a TWO-label one-hot whatever num_classes is (:275) while its first convolution
        # takes input_channels + num_classes (:218): only num_classes == 2 runs there; here the one-hot has num_classes labels
        super().__init__(phiseg3d_spec(input_channels, num_classes, num_filters, latent_levels, bool(reversible)), len(num_filters), latent_levels,
                         input_channels, num_classes, num_filters, latent_levels, image_size, reversible, exponential_weighting, device)

    # ------------------------------------------------------------------ plan construction: the 3-D geometry (HierarchicalModel)
    @staticmethod
    def _dims(t, shift=0):
        _, _, D, H, W = t.shape
        return D << shift, H << shift, W << shift

    @staticmethod
    def _new_buf(plan, name, C, size, requires_grad=True):
        return plan.vol(name, C, *size, requires_grad=requires_grad)

    @staticmethod
    def _size(v):
        return v.N, v.H, v.W

    @staticmethod
    def _pool(plan, x, name):
        return plan.avgpool3d(x, name)

    @staticmethod
    def _up2(plan, x, stem, t="", out=None):
        return plan.trilinear(x, name=f"{stem}.tri{t}", out=out)

    @staticmethod
    def _nearest_full(plan, s_in, full, name):
        f = full[1] // s_in.H
        return plan.nearest3d(s_in, f, full[0] // s_in.N, name) if f > 1 else s_in

    @staticmethod
    def _ce_post_scale(full):
        """The CE kernel averages over its batch axis, which here are the D slices of ONE sample: scale back to a sum over voxels."""
        return float(full[0])

    def _inputs(self, plan, io, full):
        io["eps"] = self._latent_bufs(plan, "eps", 2 * self.latent_levels, full)
        # cat(patch, one-hot mask - 0.5) (:275-279) is staged by forward(); the prior reads its first input_channels channels
        xin = io["input"] = plan.vol("posterior.input", self.input_channels + self.num_classes, *full, requires_grad=False)
        io["patch"] = xin.slice(0, self.input_channels)
        return xin

    def _check_size(self, D, H, W):
        R = len(self.num_filters)
        if D % (1 << (R - 1)) or H % (1 << (R - 1)) or W % (1 << (R - 1)):
            raise ValueError("PHISeg3D needs every spatial size divisible by 2^(levels-1)")

    def _build(self, D, H, W, training, bn_training, decode_only=False):
        self._check_size(D, H, W)
        return self._build_plan(D, (D, H, W), training, bn_training, decode_only)

    def _build_predict(self, D, H, W, part):
        """The two plans of predict() for one volume (HierarchicalModel._build_predict_plan): eval-mode BatchNorm, no loss or backward
        tape, fp32 storage (_passes._b16_pass skips plans that are not bn_training).  part = "trunk": patch -> the prior's contracting
        path; part = "draw": the prior's latent path and the likelihood up to the un-resized level logits io["s_in"] - no
        UZ_OP_NEAREST3D_FWD: uz_vol_sample_accum reads the levels at their own resolution."""
        self._check_size(D, H, W)
        return self._build_predict_plan(D, (D, H, W), part, resize=False)

    # ------------------------------------------------------------------ reference API (volumes are NCDHW at the boundary)
    @staticmethod
    def _to_slices(t):
        return t[0].permute(1, 0, 2, 3)                       # (1, C, D, H, W) -> (D, C, H, W)

    @staticmethod
    def _to_volume(t):
        return t.permute(1, 0, 2, 3).unsqueeze(0)             # (D, C, H, W) -> (1, C, D, H, W)

    def _boundary(self, plan):
        T = plan.tensor
        return lambda v: self._to_volume(T(v))

    def forward(self, patch, mask, training=True, eps=None):
        self._require_gpu()
        if patch.shape[0] != 1:
            raise NotImplementedError("native PHISeg3D runs one volume per call (the reference's BraTS config uses batch_size 1)")
        D, H, W = self._dims(patch)
        key = (D, H, W, bool(training), bool(self.training))
        plan = self._plan(key, lambda: self._build(D, H, W, bool(training), bool(self.training)))
        io, T = plan.io, plan.tensor
        K = self.num_classes
        T(io["patch"]).copy_(self._to_slices(patch))
        if mask.dim() == 5 and mask.shape[1] == K:            # already one-hot, as the reference's BraTS path hands it over (utils.py:296-298)
            onehot = self._to_slices(mask).to(torch.int64).to(torch.float32)
        else:                                                 # a label volume: one-hot encode it here
            lab = mask.reshape(D, 1, H, W)
            onehot = torch.cat([(lab == k) for k in range(K)], dim=1).to(torch.float32)
        T(io["input"].slice(self.input_channels, K)).copy_(onehot - 0.5)
        for k, e in enumerate(io["eps"]):
            if eps is None:
                self._fill_normal(T(e))
            else:
                T(e).copy_(self._to_slices(eps[k]))
        self._run(plan, "fwd")
        if self.training:
            self._bump_nbt(plan)
        self._cur = plan
        V = self._boundary(plan)
        self.s_in_list = [V(v) for v in io["s_in"]]
        return self._publish(plan)

    def _level_tables(self, draw, D, H, W):
        """The host tables of uz_vol_sample_accum / uz_vol_window_accum for a draw plan of extent (D, H, W), kept with the plan
        (plan.host): level pointers, channel counts and the two resize factors, finest level first."""
        tb = draw.host.get("vol_levels")
        if tb is None:
            lv = draw.io["s_in"]
            n = len(lv)
            tb = draw.host["vol_levels"] = dict(
                ptrs=(C.c_void_p * n)(*[draw._resolve(v) for v in lv]), ctot=(C.c_int * n)(*[v.Ctot for v in lv]),
                f=(C.c_int * n)(*[H // v.H for v in lv]), fz=(C.c_int * n)(*[D // v.N for v in lv]))
        return tb

    def _predict_state(self, draw, D, H, W):
        """What predict() keeps with its draw plan between calls (plan.host): the fp64 running sum and the level tables."""
        st = draw.host.get("vol_stats")
        if st is None:
            st = draw.host["vol_stats"] = dict(self._level_tables(draw, D, H, W),
                                               acc=torch.empty(self.num_classes, D, H, W, dtype=torch.float64, device=self.device))
        return st

    def _predict_plans(self, D, H, W):
        return (self._plan(("trunk", D, H, W), lambda: self._build_predict(D, H, W, "trunk")),
                self._plan(("draw", D, H, W), lambda: self._build_predict(D, H, W, "draw")))

    def _run_trunk(self, trunk, draw):
        """The trunk plan on the patch its input holds, and its feature maps handed to the draw plan (predict(), predict_volume())."""
        L, st = _ffi.lib(), C.c_void_p(self._stream())
        self._run(trunk, "fwd")
        for src, dst in zip(trunk.io["feats"], draw.io["feats"]):
            _ffi.check(L.uz_batch_repeat_fwd(trunk._resolve(src), src.C, src.Ctot, draw._resolve(dst), dst.Ctot, src.N, 1, src.H, src.W, st),
                       "batch_repeat_fwd")

    def _draw(self, draw, noise):
        """One sample: the noise - drawn on the device, or `noise`, L tensors (1, 2, d_k, h_k, w_k), deepest first - and the draw plan."""
        T = draw.tensor
        for k, e in enumerate(draw.io["eps"]):
            if noise is None:
                self._fill_normal(T(e))
            else:
                T(e).copy_(self._to_slices(noise[k]))
        self._run(draw, "fwd")

    def predict(self, patch, n_samples=1, eps=None, return_soft=False, return_levels=False):
        """Segment the volume `patch` (1, C, D, H, W) without a label mask: n_samples draws from the prior, from ONE pass of its
        contracting path (in eval mode it does not depend on the noise).  The trunk plan runs once and hands its feature maps to the
        draw plan (uz_batch_repeat_fwd with S = 1: a strided slice copy; nothing in the draw plan writes them, so they survive all its
        runs); then per sample: noise, the draw plan, uz_vol_sample_accum - which reads the level logits at their own resolution,
        writes the sample's labels and adds its probabilities to an fp64 running sum kept with the plan -, and at the end
        uz_vol_sample_finish.  `eps` (optional, L tensors, deepest level first, each (n_samples, 2, d_k, h_k, w_k)) injects the noise;
        default draws it on the device.  Returns a Prediction with one more spatial axis: labels (S, 1, D, H, W) uint8, mean_soft
        (1, K, D, H, W), mean_label and entropy (1, D, H, W), soft (S, 1, K, D, H, W) or None, and levels - with return_levels=True
        (meant for small volumes and tests) L tensors (S, 1, K, d_l, h_l, w_l) of every sample's UN-RESIZED level logits, finest
        first, copied per sample; else None.  prior_mu / prior_sigma / prior_latent_space are set as forward() sets them, for the
        LAST sample drawn (views of the plan's buffers)."""
        self._require_gpu()
        if self.training:
            raise RuntimeError("predict() needs eval mode: with batch statistics the contracting path of a volume is not shared by its samples")
        if self.reversible:
            raise NotImplementedError("predict() is not built for the reversible variant")
        if patch.shape[0] != 1:
            raise NotImplementedError("native PHISeg3D runs one volume per call (the reference's BraTS config uses batch_size 1)")
        S, nl, K, dev = int(n_samples), self.latent_levels, self.num_classes, self.device
        if S < 1:
            raise ValueError("predict() needs n_samples >= 1")
        D, H, W = self._dims(patch)
        self._check_size(D, H, W)
        if eps is not None and len(eps) != nl:
            raise ValueError(f"predict() takes {nl} eps tensors (deepest level first), got {len(eps)}")
        trunk, draw = self._predict_plans(D, H, W)
        L, st = _ffi.lib(), C.c_void_p(self._stream())
        T, io = draw.tensor, draw.io
        trunk.tensor(trunk.io["patch"]).copy_(self._to_slices(patch))
        self._run_trunk(trunk, draw)
        host = self._predict_state(draw, D, H, W)
        out = Prediction(labels=torch.empty(S, 1, D, H, W, dtype=torch.uint8, device=dev), mean_soft=torch.empty(1, K, D, H, W, device=dev),
                         mean_label=torch.empty(1, D, H, W, dtype=torch.uint8, device=dev), entropy=torch.empty(1, D, H, W, device=dev),
                         levels=[torch.empty(S, 1, v.C, v.N, v.H, v.W, device=dev) for v in io["s_in"]] if return_levels else None,
                         soft=torch.empty(S, 1, K, D, H, W, device=dev) if return_soft else None)
        for s in range(S):
            self._draw(draw, None if eps is None else [e[s:s + 1] for e in eps])
            _ffi.check(L.uz_vol_sample_accum(host["ptrs"], host["ctot"], host["f"], host["fz"], nl, K, D, H, W, out.labels[s].data_ptr(),
                                             out.soft[s].data_ptr() if return_soft else None, host["acc"].data_ptr(), int(s == 0), st),
                       "vol_sample_accum")
            if return_levels:
                for l, v in enumerate(io["s_in"]):
                    out.levels[l][s].copy_(self._to_volume(T(v)))
        _ffi.check(L.uz_vol_sample_finish(host["acc"].data_ptr(), K, S, D, H, W, out.mean_soft.data_ptr(), out.mean_label.data_ptr(),
                                          out.entropy.data_ptr(), st), "vol_sample_finish")
        order = [nl - 1 - lvl for lvl in range(nl)]        # level -> draw index
        V = self._boundary(draw)
        self.prior_mu = [V(io["prior"][k].mu) for k in order]
        self.prior_sigma = [V(io["prior"][k].sigma) for k in order]
        self.prior_latent_space = [V(io["prior_z"][k]) for k in order]
        return out

    def window_plan(self, dhw, window=None, stride=None):
        """window_grid() with this model's defaults: window = image_size[1:], stride = half of it (default_stride), g = 2^(levels-1)."""
        g = 1 << (len(self.num_filters) - 1)
        if window is None:
            window = tuple(self.image_size[1:])
            if len(window) != 3:
                raise ValueError(f"predict_volume() needs a window: image_size {tuple(self.image_size)} names no (D, H, W)")
        return window_grid(dhw, window, stride, g)

    def predict_volume(self, volume, n_samples=1, window=None, stride=None, blend="gaussian", eps=None, return_soft=False, flips=None):
        """predict() for a volume of ANY size (1, C, D, H, W): the net runs on overlapping windows of the size it was trained at and
        the windows' probabilities are blended.  window defaults to image_size[1:], stride to half of it; window_grid() says where the
        windows lie (a window no smaller than the volume rounded up to 2^(levels-1) is the plain pad-to-divisible route: one window),
        blend_tables() how they are weighted ("gaussian" | "uniform").  Voxels of a window beyond the volume are read as 0 and never
        written.  The samples are coherent across windows: ONE noise field per latent level is drawn per call - with predict()'s
        generator, shaped as predict() takes `eps` for the padded volume, n_samples rows - and every window receives its crop; `eps`
        (L tensors, deepest first, those shapes) injects the fields.  Order of work: per window the gather (uz_vol_window_gather), the
        trunk plan ONCE and the hand-over of its features, then per sample the noise crop, the draw plan and uz_vol_window_accum; after
        the last window one uz_vol_window_finish.  The plans are predict()'s, keyed by the window's extent.  Kept with the draw plan
        between calls and zeroed at the start of each: S accumulators (K, D, H, W) and one weight sum (D, H, W), all fp64 =
        8 (S K + 1) D H W bytes - the accumulators 3.4 GB, the weight sum 71 MB at 240 x 240 x 155, K = 3, S = 16.  Returns predict()'s Prediction for (D, H, W) (levels = None);
        sample s: p_s = sum_windows weight * softmax / sum_windows weight, labels its first maximum, mean_soft the mean over the samples,
        mean_label / entropy from the unrounded mean.  prior_mu / prior_sigma / prior_latent_space are left as they are.
        flips: mirrored passes (flip test-time augmentation; the net is trained with random flips on all three axes).  None - the
        default - is the call above.  "all" = the masks 0 .. 7, or a sequence of distinct masks in 0 .. 7, in the order of the passes
        (it may leave out 0, the unmirrored pass); bit 0, 1, 2 of a mask mirror D, H, W.  A pass with mask m mirrors every window
        WITHIN ITSELF - grid, order of the visits and coverage stay: net-frame voxel (z, y, x) of a window of extent (wd, wh, ww) at
        (oz, oy, ox) is volume voxel (oz + z', oy + y', ox + x'), z' = wd - 1 - z where bit 0 is set, else z (likewise y', x').  The net
        reads that voxel (0 beyond the volume); the window's crop of every level's noise field, cut as without a mirror, is mirrored
        within the crop at the level's resolution, so a sample's noise stays attached to the anatomy under every mask; the net's
        probabilities at (z, y, x) are added at that volume voxel with the weight (tz[z'] ty[y']) tx[x'].  Order of work: per window,
        per mask: the mirrored gather (uz_vol_window_gather_ex) and the trunk plan once, then per sample the mirrored noise crop
        (uz_vol_window_noise, straight into the draw plan), the draw plan and uz_vol_window_accum_ex into the SAME accumulators; the
        weight sum takes every (window, mask) pair once, so p_s = sum_windows sum_masks weight * softmax / sum weight, averaged before
        any rounding.  One stream, no atomics: a repeated call is bit-equal.  Cost: n masks = n times the trunk and draw plans; no
        memory beyond the call without flips."""
        S, nl, K, R = int(n_samples), self.latent_levels, self.num_classes, len(self.num_filters)
        if S < 1:
            raise ValueError("predict_volume() needs n_samples >= 1")
        if volume.dim() != 5 or volume.shape[0] != 1 or volume.shape[1] != self.input_channels:
            raise ValueError(f"predict_volume() takes one volume (1, {self.input_channels}, D, H, W), got {tuple(volume.shape)}")
        D, H, W = self._dims(volume)
        padded, extent, origins = self.window_plan((D, H, W), window, stride)
        tables = blend_tables(extent, blend)
        masks = None if flips is None else flip_masks(flips)
        shapes = [(S, 2, *(n >> (R - 1 - k) for n in padded)) for k in range(nl)]             # deepest level first
        if eps is not None and (len(eps) != nl or [tuple(e.shape) for e in eps] != shapes):
            raise ValueError(f"predict_volume() takes {nl} eps tensors of the shapes {shapes} (deepest level first), got "
                             f"{[tuple(e.shape) for e in eps]}")
        self._require_gpu()
        if self.training:
            raise RuntimeError("predict() needs eval mode: with batch statistics the contracting path of a volume is not shared by its samples")
        if self.reversible:
            raise NotImplementedError("predict() is not built for the reversible variant")
        dev = self.device
        ed, eh, ew = extent
        trunk, draw = self._predict_plans(ed, eh, ew)
        L, st = _ffi.lib(), C.c_void_p(self._stream())
        tb = self._level_tables(draw, ed, eh, ew)
        state = draw.host.get("vol_window")
        if state is None or state["key"] != (S, D, H, W):
            state = None                                                                        # free the old ones first
            draw.host.pop("vol_window", None)
            state = draw.host["vol_window"] = dict(key=(S, D, H, W), acc=torch.empty(S, K, D, H, W, dtype=torch.float64, device=dev),
                                                   wsum=torch.empty(D, H, W, dtype=torch.float64, device=dev))
        wt = draw.host.setdefault("vol_blend", {}).get(blend)
        if wt is None:
            wt = draw.host["vol_blend"][blend] = [torch.from_numpy(t).to(dev) for t in tables]
        acc, wsum = state["acc"], state["wsum"]
        acc.zero_()
        wsum.zero_()
        src = volume[0].to(torch.float32).contiguous()
        if eps is None:
            eps = [self._fill_normal(torch.empty(shape, device=dev)) for shape in shapes]
        patch = trunk.io["patch"]
        if masks is not None:
            eps = [e.to(device=dev, dtype=torch.float32).contiguous() for e in eps]
        for oz, oy, ox in origins:
            for m in (None,) if masks is None else masks:
                if m is None:
                    _ffi.check(L.uz_vol_window_gather(src.data_ptr(), self.input_channels, D, H, W, oz, oy, ox, trunk._resolve(patch), patch.Ctot,
                                                      ed, eh, ew, st), "vol_window_gather")
                else:
                    _ffi.check(L.uz_vol_window_gather_ex(src.data_ptr(), self.input_channels, D, H, W, oz, oy, ox, trunk._resolve(patch),
                                                         patch.Ctot, ed, eh, ew, m, st), "vol_window_gather_ex")
                self._run_trunk(trunk, draw)
                for s in range(S):
                    if m is None:
                        noise = []
                        for k, e in enumerate(eps):
                            sh = R - 1 - k                                                      # origins are multiples of 2^(R-1)
                            noise.append(e[s:s + 1, :, oz >> sh:(oz + ed) >> sh, oy >> sh:(oy + eh) >> sh, ox >> sh:(ox + ew) >> sh])
                        self._draw(draw, noise)
                        _ffi.check(L.uz_vol_window_accum(tb["ptrs"], tb["ctot"], tb["f"], tb["fz"], nl, K, ed, eh, ew, oz, oy, ox, D, H, W,
                                                         wt[0].data_ptr(), wt[1].data_ptr(), wt[2].data_ptr(), acc[s].data_ptr(), wsum.data_ptr(),
                                                         int(s == 0), st), "vol_window_accum")
                        continue
                    for k, (e, v) in enumerate(zip(eps, draw.io["eps"])):
                        sh = R - 1 - k
                        _ffi.check(L.uz_vol_window_noise(e[s].data_ptr(), 2, *e.shape[2:], oz >> sh, oy >> sh, ox >> sh, ed >> sh, eh >> sh, ew >> sh,
                                                         m, draw._resolve(v), v.Ctot, st), "vol_window_noise")
                    self._run(draw, "fwd")
                    _ffi.check(L.uz_vol_window_accum_ex(tb["ptrs"], tb["ctot"], tb["f"], tb["fz"], nl, K, ed, eh, ew, oz, oy, ox, D, H, W,
                                                        wt[0].data_ptr(), wt[1].data_ptr(), wt[2].data_ptr(), acc[s].data_ptr(), wsum.data_ptr(),
                                                        int(s == 0), m, st), "vol_window_accum_ex")
        out = Prediction(labels=torch.empty(S, 1, D, H, W, dtype=torch.uint8, device=dev), mean_soft=torch.empty(1, K, D, H, W, device=dev),
                         mean_label=torch.empty(1, D, H, W, dtype=torch.uint8, device=dev), entropy=torch.empty(1, D, H, W, device=dev),
                         levels=None, soft=torch.empty(S, 1, K, D, H, W, device=dev) if return_soft else None)
        _ffi.check(L.uz_vol_window_finish(acc.data_ptr(), wsum.data_ptr(), K, S, D, H, W, out.labels.data_ptr(),
                                          out.soft.data_ptr() if return_soft else None, out.mean_soft.data_ptr(), out.mean_label.data_ptr(),
                                          out.entropy.data_ptr(), st), "vol_window_finish")
        return out

    def _publish_loss(self, total, terms):
        # the reference accumulates both parts into loss_tot and returns the running total from each helper (:547-555,:582-583,
        # :597-604): kl_divergence_loss is the weighted KL sum, reconstruction_loss the grand total
        self.kl_divergence_loss = terms[:self.latent_levels].sum()
        self.loss_tot = self.reconstruction_loss = total

    def accumulate_output(self, output_list, use_softmax=False):
        """phiseg3D.py:469-475 (in place on the last level, as the reference)."""
        s_accum = output_list[-1]
        for i in range(len(output_list) - 1):
            s_accum += output_list[i]
        return torch.softmax(s_accum, dim=1) if use_softmax else s_accum
