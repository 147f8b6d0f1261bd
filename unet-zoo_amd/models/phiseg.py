"""PHiSeg (7 resolution levels / 5 latent levels) on the native HIP path.

Drop-in for the reference ``models/phiseg.py`` ``PHISeg`` class: same constructor keywords
(phiseg.py:336-349), same ``forward(patch, mask, training)`` / ``loss(mask)`` /
``accumulate_output`` / ``sample`` / ``reconstruct`` surface, same ``state_dict`` keys (820 for
the standard filter list) and the same quirks:
  * the architecture is always 7/5 whatever ``latent_levels`` says (phiseg.py:131-132);
  * ``kl_divergence_loss`` and ``reconstruction_loss`` alias the total loss (phiseg.py:519-534);
  * KL uses ``sigma1*sigma0`` (phiseg.py:438-439);
  * ``upsampling_path.4`` of posterior and prior is never executed, so its parameters keep
    ``grad is None`` (phiseg.py:161-164,198-199);
  * ``accumulate_output`` sums the levels in place into ``output_list[-1]`` (phiseg.py:428-434).
The forward/backward arithmetic itself runs in libuz_hip.so (see _plan.py for the op tape).  The plan builder and the reference API
on top of a plan are shared with PHISeg3D (models/_hier.py); this file holds the 2-D geometry and what only the 2-D model has.
Beyond the reference: predict(patch, n_samples) - samples, mean probabilities and an uncertainty map without a label mask.
"""
import ctypes as C

import torch

from .. import _ffi
from ._hier import HierarchicalModel, hier_spec

RES_LEVELS = 7
LAT_LEVELS = 5


def phiseg_spec(input_channels, num_classes, num_filters, reversible=False):
    """The posterior sees a two-label one-hot whatever num_classes is (phiseg.py:209-214)."""
    return hier_spec(input_channels, 2, num_classes, list(num_filters), RES_LEVELS, LAT_LEVELS, reversible, PHISeg.rev_depths)


class Prediction:
    """What PHISeg.predict returns for S samples of B images: labels (S, B, H, W) uint8, mean_soft (B, K, H, W) - the mean class
    probabilities over the samples -, mean_label (B, H, W) uint8 = argmax of mean_soft, entropy (B, H, W) of mean_soft (natural log),
    levels - the five level logits (S * B, K, H, W) as views of the plan's buffers, valid until the next predict() of that shape -
    and soft (S, B, K, H, W), the per-sample probabilities, or None unless asked for.  PHISeg3D.predict returns the same object for one
    volume, with (D, H, W) in the place of (H, W) and other `levels` (see there)."""
    __slots__ = ("labels", "mean_soft", "mean_label", "entropy", "levels", "soft")

    def __init__(self, labels, mean_soft, mean_label, entropy, levels, soft=None):
        self.labels, self.mean_soft, self.mean_label, self.entropy, self.levels, self.soft = labels, mean_soft, mean_label, entropy, levels, soft


class PHISeg(HierarchicalModel):
    wgrad_workgroups = 128                     # NativeModel.wgrad_workgroups: 256 -> 1 907, 192 -> 1 946, 128 -> 1 970, 96 -> 1 916, 64 -> 1 778 images/s (one box)
    default_lanes_by_mode = {"lanes": 3}     # host-issued lane replay: 2 lanes 17.7 ms, 3: 16.3, 4: 16.2 (one box, round 5)
    decouple_wgrad_px = 8192       # see NativeModel.decouple_wgrad_px: the 16 x 16 ... 2 x 2 levels at batch 32
    decouple_wgrad_prefixes = ("likelihood",)      # its backward is a single chain (posterior / prior pair up): A/B 1 726 -> 1 744 images/s
    predict_rows_budget = 128  # UNetModel.score: predict()'s draw plan runs at batch images x samples, 87 MB of arena per row at the headline filters (profiles/NOTES_predict.md)
    rev_depths = (3, 2)        # reversible_depth of the contracting / sample_z stacks and of the up / likelihood stacks (phiseg.py:25-26,53-54,87-88)

    def __init__(self, input_channels, num_classes, num_filters, latent_levels=5, latent_dim=2, initializers=None,
                 no_convs_fcomb=4, beta=10.0, image_size=(128, 128, 1), reversible=False, apply_last_layer=True,
                 exponential_weighting=True, padding=True, device=None):
        if len(num_filters) < RES_LEVELS or num_filters[4] != num_filters[6]:
            raise ValueError("PHISeg needs >= 7 filters with num_filters[4] == num_filters[6] (phiseg.py:131-132,258-270)")
        super().__init__(phiseg_spec(input_channels, num_classes, num_filters, bool(reversible)), RES_LEVELS, LAT_LEVELS, input_channels,
                         num_classes, num_filters, latent_levels, image_size, reversible, exponential_weighting, device)
        self.padding, self.activation_maps, self.apply_last_layer = padding, [], apply_last_layer

    # ------------------------------------------------------------------ plan construction: the 2-D geometry (HierarchicalModel)
    @staticmethod
    def _dims(t, shift=0):
        N, _, H, W = t.shape
        return N, H << shift, W << shift

    @staticmethod
    def _new_buf(plan, name, C, size, requires_grad=True):
        return plan.buf(name, C, *size, requires_grad=requires_grad)

    @staticmethod
    def _size(v):
        return v.H, v.W

    @staticmethod
    def _pool(plan, x, name):
        return plan.avgpool(x, name)

    @staticmethod
    def _up2(plan, x, stem, t="", out=None):
        return plan.bilinear(x, True, name=f"{stem}.bil{t}", out=out)

    @staticmethod
    def _nearest_full(plan, s_in, full, name):
        return plan.nearest(s_in, full[0] // s_in.H, name)

    def _inputs(self, plan, io, full):
        io["patch"] = plan.buf("patch", self.input_channels, *full, requires_grad=False)
        io["mask"] = plan.buf("mask", 1, *full, requires_grad=False)
        io["eps"] = self._latent_bufs(plan, "eps", 2 * LAT_LEVELS, full)
        return plan.posterior_input(io["patch"], io["mask"], 2, "posterior.input")

    def _build(self, N, H, W, training, bn_training, decode_only=False):
        if H % 64 or W % 64:
            raise ValueError("PHISeg needs H and W divisible by 64 (7 resolution levels)")
        return self._build_plan(N, (H, W), training, bn_training, decode_only)

    def _build_predict(self, N, H, W, part):
        """The two plans of predict() (HierarchicalModel._build_predict_plan): part = "trunk" at the batch of the images, part = "draw"
        at the batch of images x samples, ending at the five level logits resized to the image.  io["feats"] lists the five hand-over
        views, levels 2 .. 5 and the deepest, in the same order in both plans."""
        if H % 64 or W % 64:
            raise ValueError("PHISeg needs H and W divisible by 64 (7 resolution levels)")
        return self._build_predict_plan(N, (H, W), part)

    # ------------------------------------------------------------------ reference API
    def forward(self, patch, mask, training=True, eps=None):
        """PHISeg.forward (phiseg.py:414-426).  `eps` (optional, list of 10 tensors: 5 posterior draws
        deepest first, then 5 prior draws) injects the latent noise; default draws it on the device."""
        self._require_gpu()
        N, _, H, W = patch.shape
        key = (N, H, W, bool(training), bool(self.training))
        plan = self._plan(key, lambda: self._build(N, H, W, bool(training), bool(self.training)))
        plan.tensor(plan.io["patch"]).copy_(patch)
        plan.tensor(plan.io["mask"]).copy_(mask.reshape(N, 1, H, W))
        self._noise(plan, eps)
        self._run(plan, "fwd")
        if self.training:
            self._bump_nbt(plan)
        self._cur = plan
        return self._publish(plan)

    def _noise(self, plan, eps):
        """The plan's noise buffers: copies of `eps`, or drawn on the device - in ONE launch where the buffers are neighbours in the arena."""
        bufs = plan.io["eps"]
        if eps is not None:
            for e, src in zip(bufs, eps):
                plan.tensor(e).copy_(src)
            return
        if "eps_span" not in plan.host:
            plan.host["eps_span"] = plan.span(bufs)
        flat = plan.host["eps_span"]
        if flat is not None:
            self._fill_normal(flat)
        else:
            for e in bufs:
                self._fill_normal(plan.tensor(e))

    def predict(self, patch, n_samples=1, eps=None, return_soft=False):
        """Segment `patch` (B, C, H, W) without a label mask: n_samples draws from the prior, from ONE pass of its contracting path.
        In eval mode BatchNorm is a per-channel affine map of its input, so the contracting path gives every copy of an image in
        patch.repeat(n_samples, 1, 1, 1) the same feature maps: it runs once, at batch B, and its five outputs are repeated into the
        plan that draws (uz_batch_repeat_fwd) - the rows of that plan are ordered s * B + b like the repeated patch.  `eps`
        (optional, 5 tensors, deepest level first, each (n_samples * B, 2, h, w): the prior half of forward()'s eps) injects the
        noise; default draws it on the device.  Returns a Prediction; also sets prior_mu / prior_sigma / prior_latent_space for
        the n_samples * B rows, as forward() does."""
        self._require_gpu()
        if self.training:
            raise RuntimeError("predict() needs eval mode: with batch statistics the contracting path of one image is not shared by its samples")
        if self.reversible:
            raise NotImplementedError("predict() is not built for the reversible variant")
        B, _, H, W = patch.shape
        S = int(n_samples)
        if S < 1:
            raise ValueError("predict() needs n_samples >= 1")
        if H % 64 or W % 64:
            raise ValueError("PHISeg needs H and W divisible by 64 (7 resolution levels)")
        trunk = self._plan(("trunk", B, H, W), lambda: self._build_predict(B, H, W, "trunk"))
        draw = self._plan(("draw", B * S, H, W), lambda: self._build_predict(B * S, H, W, "draw"))
        L, st = _ffi.lib(), C.c_void_p(self._stream())
        trunk.tensor(trunk.io["patch"]).copy_(patch)
        self._run(trunk, "fwd")
        for src, dst in zip(trunk.io["feats"], draw.io["feats"]):
            _ffi.check(L.uz_batch_repeat_fwd(trunk._resolve(src), src.C, src.Ctot, draw._resolve(dst), dst.Ctot, B, S, src.H, src.W, st),
                       "batch_repeat_fwd")
        io = draw.io
        if eps is not None and len(eps) != LAT_LEVELS:
            raise ValueError(f"predict() takes {LAT_LEVELS} eps tensors (deepest level first), got {len(eps)}")
        self._noise(draw, eps)
        self._run(draw, "fwd")
        T = draw.tensor
        order = [LAT_LEVELS - 1 - lvl for lvl in range(LAT_LEVELS)]        # level -> draw index
        self.prior_mu = [T(io["prior"][k].mu) for k in order]
        self.prior_sigma = [T(io["prior"][k].sigma) for k in order]
        self.prior_latent_space = [T(io["prior_z"][k]) for k in order]
        levels = [T(v) for v in io["s"]]
        tab = draw.host.get("s_tab")
        if tab is None:
            tab = draw.host["s_tab"] = torch.tensor([t.data_ptr() for t in levels], dtype=torch.int64, device=self.device)
        K, dev = self.num_classes, self.device
        out = Prediction(labels=torch.empty(S, B, H, W, dtype=torch.uint8, device=dev), mean_soft=torch.empty(B, K, H, W, device=dev),
                         mean_label=torch.empty(B, H, W, dtype=torch.uint8, device=dev), entropy=torch.empty(B, H, W, device=dev),
                         levels=levels, soft=torch.empty(S, B, K, H, W, device=dev) if return_soft else None)
        _ffi.check(L.uz_sample_stats(tab.data_ptr(), len(levels), K, B, S, H, W, out.soft.data_ptr() if return_soft else None,
                                     out.labels.data_ptr(), out.mean_soft.data_ptr(), out.mean_label.data_ptr(), out.entropy.data_ptr(), st),
                   "sample_stats")
        return out

    def _publish_loss(self, total, terms):
        # the reference accumulates everything into ONE tensor object (phiseg.py:523,477,512)
        self.loss_tot = self.kl_divergence_loss = self.reconstruction_loss = total

    # ---- the reference's public loss helpers (phiseg.py:436-513) as stand-alone device evaluations.  They return
    # plain values (no autograd graph): gradients of the training loss come from the backward tape of loss().
    def KL_two_gauss_with_diag_cov(self, mu0, sigma0, mu1, sigma1):
        """phiseg.py:436-453 incl. the sigma1*sigma0 quirk; (N, ...) device tensors -> 0-d tensor."""
        self._require_gpu()
        t = [x.detach().to(self.device, torch.float32).contiguous() for x in (mu0, sigma0, mu1, sigma1)]
        N = t[0].shape[0]
        out = torch.empty(1, device=self.device)
        _ffi.check(_ffi.lib().uz_kl_fwd(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), N,
                                        t[0].numel() // N, 1.0, out.data_ptr(), self._stream()), "kl_fwd")
        return out.reshape(())

    def calculate_hierarchical_KL_div_loss(self):
        """phiseg.py:455-479 on the cached posterior / prior moments of the last forward()."""
        w = [self.exponential_weight ** i if self.exponential_weighting else 1 for i in range(self.latent_levels)]
        for ii in reversed(range(self.latent_levels)):
            self.loss_dict["KL_divergence_loss_lvl%d" % ii] = w[ii] * self.KL_two_gauss_with_diag_cov(
                self.posterior_mu[ii], self.posterior_sigma[ii], self.prior_mu[ii], self.prior_sigma[ii])
            self.loss_tot = self.loss_tot + self.kl_divergence_loss_weight * self.loss_dict["KL_divergence_loss_lvl%d" % ii]
        return self.loss_tot

    def _ce_levels(self, logits, target):
        self._require_gpu()
        logits = [x.detach().to(self.device, torch.float32).contiguous() for x in logits]
        N, K, H, W = logits[0].shape
        L = _ffi.lib()
        tgt = target.detach().to(self.device, torch.float32).reshape(N, 1, H, W).contiguous()
        tab = torch.tensor([x.data_ptr() for x in logits], dtype=torch.int64, device=self.device)
        ws = torch.empty(L.uz_ce_workspace(N, H, W, len(logits)) // 4 + 16, device=self.device)
        out = torch.empty(len(logits), device=self.device)
        _ffi.check(L.uz_residual_ce_fwd(tab.data_ptr(), len(logits), K, tgt.data_ptr(), N, H, W, out.data_ptr(), ws.data_ptr(),
                                        self._stream()), "residual_ce_fwd")
        return out

    def multinoulli_loss(self, reconstruction, target):
        """phiseg.py:481-490: per-pixel CE summed over pixels, mean over the batch."""
        return self._ce_levels([reconstruction], target)[0]

    def residual_multinoulli_loss(self, reconstruction, target):
        """phiseg.py:492-513 on a list of level logits (finest first)."""
        terms = self._ce_levels(list(reconstruction), target)
        for ii in reversed(range(len(reconstruction))):
            self.loss_dict["residual_multinoulli_loss_lvl%d" % ii] = terms[ii]
            self.loss_tot = self.loss_tot + self.residual_multinoulli_loss_weight * terms[ii]
        return self.loss_tot

    def accumulate_output(self, output_list, use_softmax=False):
        """phiseg.py:428-434 incl. the in-place accumulation into output_list[-1]."""
        self._require_gpu()
        last = output_list[-1]
        N, K, H, W = last.shape
        assert all(t.is_contiguous() for t in output_list)
        tab = torch.tensor([t.data_ptr() for t in output_list], dtype=torch.int64, device=self.device)
        soft = torch.empty_like(last) if use_softmax else None
        _ffi.check(_ffi.lib().uz_accumulate_softmax_argmax(tab.data_ptr(), len(output_list), K, N, H, W, last.data_ptr(),
                                                           soft.data_ptr() if use_softmax else None, None, self._stream()), "accumulate_output")
        return soft if use_softmax else last
