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
"""
import torch

from ._hier import HierarchicalModel, hier_spec, lift3


def phiseg3d_spec(input_channels, num_classes, num_filters, latent_levels, reversible=False):
    nf = list(num_filters)
    return lift3(hier_spec(input_channels, num_classes, num_classes, nf, len(nf), latent_levels, reversible, PHISeg3D.rev_depths))


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

    def _build(self, D, H, W, training, bn_training, decode_only=False):
        R = len(self.num_filters)
        if D % (1 << (R - 1)) or H % (1 << (R - 1)) or W % (1 << (R - 1)):
            raise ValueError("PHISeg3D needs every spatial size divisible by 2^(levels-1)")
        return self._build_plan(D, (D, H, W), training, bn_training, decode_only)

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
