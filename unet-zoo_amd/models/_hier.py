"""What PHISeg (models/phiseg.py) and PHISeg3D (models/phiseg3D.py) share: the hierarchical probabilistic U-Net of the reference's
``phiseg.py`` / ``phiseg3D.py`` on R resolution and L latent levels - its parameter spec and, in HierarchicalModel, the plan builder
(contracting path, latent path, likelihood, ELBO tape, decode-only plan) and the reference API on top of a built plan.  The two
models differ in their geometry only, which HierarchicalModel reads through a handful of hooks (see the end of the class).
"""
import torch

from .._engine import NativeModel, conv_unit
from .._modtree import conv_unit_spec, plain_conv_spec, rev_sequence_spec, init_default


def _stack_spec(prefixes, rev_prefix, cin, cout, reversible, depth):
    """len(prefixes) Conv units - or ReversibleSequence(cin, cout, reversible_depth=depth): the spec of HierarchicalModel._stack."""
    if reversible:
        return rev_sequence_spec(rev_prefix, cin, cout, depth)
    out = []
    for j, p in enumerate(prefixes):
        out += conv_unit_spec(p, cin if j == 0 else cout, cout)
    return out


def _encoder_spec(root, in_ch, nf, R, L, reversible, depths):
    """Posterior / prior entries in the reference's registration order (phiseg.py:144-173)."""
    out = []
    for i in range(R):
        p = f"{root}.contracting_path.{i}.layers."
        base = 0 if i == 0 else 1          # layers.0 is the AvgPool when pooling
        out += _stack_spec([p + str(base + j) for j in range(3)], p + str(base), in_ch if i == 0 else nf[i - 1], nf[i], reversible, depths[0])
    for k in range(L):
        p = f"{root}.upsampling_path.{k}.upconv_layer"
        out += _stack_spec([p + ".0", p + ".1"], p, 2, 2 * nf[0], reversible, depths[1])
    for k in range(L):
        i = L - 1 - k + R - L
        cin = nf[i] if k == 0 else 2 * nf[0] + nf[i]
        p = f"{root}.sample_z_path.{k}"
        out += _stack_spec([p + ".conv.0", p + ".conv.1"], p + ".conv.0", cin, cin, reversible, depths[0])
        out += plain_conv_spec(p + ".mu_conv.0", cin, 2, 1) + plain_conv_spec(p + ".sigma_conv.0", cin, 2, 1)
    return out


def _likelihood_spec(nf, R, L, num_classes, reversible, depths):
    """Likelihood entries (phiseg.py:252-284): both ModuleLists of the first loop are registered before the loop, so all ups_path
    entries precede all post_ups_path entries."""
    root, diff, out = "likelihood", R - L, []
    for k in range(L):
        p, c = f"{root}.likelihood_ups_path.{k}", nf[L - 1 - k]
        out += _stack_spec([p + ".convolution.0", p + ".convolution.1"], p, 2, c, reversible, depths[1])
    for k in range(L):
        c = nf[L - 1 - k]
        for t in range(diff):
            out += conv_unit_spec(f"{root}.likelihood_post_ups_path.{k}.{2 * t + 1}.convolution.0", c, c)
    for i in range(L - 1):
        p = f"{root}.likelihood_post_c_path.{i}"
        out += _stack_spec([p + ".convolution.0", p + ".convolution.1"], p, nf[i] + nf[i + 1 + diff], nf[i + diff], reversible, depths[1])
    for k in range(L):
        out += conv_unit_spec(f"{root}.s_layer.{k}.convolution.0", nf[L - 1 - k + diff], num_classes, k=1, norm=False)
    return out


def hier_spec(input_channels, label_channels, num_classes, nf, R, L, reversible, depths):
    """posterior + likelihood + prior.  label_channels: what the posterior sees beside the image; depths: reversible_depth of the
    (contracting / sample_z, up / likelihood) stacks."""
    return (_encoder_spec("posterior", input_channels + label_channels, nf, R, L, reversible, depths)
            + _likelihood_spec(nf, R, L, num_classes, reversible, depths)
            + _encoder_spec("prior", input_channels, nf, R, L, reversible, depths))


def lift3(spec):
    """The Conv3d form of a spec: every convolution weight gains a third kernel dimension."""
    return [(key, shape + (shape[-1],) if kind == "conv_w" else shape, kind) for key, shape, kind in spec]


class HierarchicalModel(NativeModel):
    def __init__(self, spec, R, L, input_channels, num_classes, num_filters, latent_levels, image_size, reversible, exponential_weighting, device):
        super().__init__()
        self._R, self._L = R, L
        self.reversible = bool(reversible)
        self.input_channels, self.num_classes, self.num_filters = input_channels, num_classes, list(num_filters)
        self.latent_levels, self.image_size = latent_levels, image_size
        self.loss_tot, self.loss_dict = 0, {}
        self.kl_divergence_loss_weight, self.beta = 1.0, 1.0
        self.exponential_weighting, self.exponential_weight = exponential_weighting, 4
        self.residual_multinoulli_loss_weight = 1.0
        self.kl_divergence_loss = self.reconstruction_loss = 0
        self.s_out_list = [None] * latent_levels
        self._init_storage(spec, device)
        init_default(self._ptab)

    # ------------------------------------------------------------------ plan construction
    def _stack(self, plan, x, prefixes, rev_prefix, cout, depth, out=None):
        """len(prefixes) Conv units - or, in the reversible variant, ReversibleSequence(cin, cout, reversible_depth=depth)
        (phiseg.py:25-26,53-54,87-88)."""
        if self.reversible:
            return plan.rev_sequence(x, rev_prefix, cout, depth, conv_unit, out=out)
        for p in prefixes[:-1]:
            x = conv_unit(plan, x, p)
        return conv_unit(plan, x, prefixes[-1], out=out)

    def _latent_bufs(self, plan, stem, n, full):
        """n plan inputs of two channels at the latent levels' sizes, deepest first (the noise; decode: the latent samples)."""
        R, L = self._R, self._L
        return [self._new_buf(plan, f"{stem}{k}", 2, tuple(s >> (R - 1 - k % L) for s in full), requires_grad=False) for k in range(n)]

    def _encoder(self, plan, root, x, eps, z_override, want_z):
        skips, pre = self._contracting(plan, root, x)
        return self._latent_path(plan, root, skips, pre, eps, z_override, want_z)

    def _contracting(self, plan, root, x):
        """The R Conv stacks of an encoder (phiseg.py:191-194).  Returns the concat buffers of levels R-L .. R-2, their skip slice
        written, and the deepest feature map: what the latent path reads."""
        nf, R, L = self.num_filters, self._R, self._L
        skips = {}
        for i in range(R):
            base = 0
            if i != 0:
                x = self._pool(plan, x, f"{root}.pool{i}")
                base = 1
            out = None
            if R - L <= i <= R - 2:     # these blocks feed torch.cat([up, bridge]) (phiseg.py:71): write them in place
                cat = skips[i] = self._new_buf(plan, f"{root}.cat{i}", 2 * nf[0] + nf[i], self._size(x))
                out = cat.slice(2 * nf[0], nf[i])
            p = f"{root}.contracting_path.{i}.layers."
            x = self._stack(plan, x, [p + str(base + j) for j in range(3)], p + str(base), nf[i], self.rev_depths[0], out=out)
        return skips, x

    def _latent_path(self, plan, root, skips, pre, eps, z_override, want_z):
        """The L SampleZBlocks and the up path between them (phiseg.py:196-202), deepest level first."""
        nf, R, L = self.num_filters, self._R, self._L
        lats, zs = [], []
        for k in range(L):
            if k != 0:
                cat = skips[R - 1 - k]
                u = self._up2(plan, zs[k - 1], f"{root}.up{k}")
                p = f"{root}.upsampling_path.{k - 1}.upconv_layer"
                self._stack(plan, u, [p + ".0", p + ".1"], p, 2 * nf[0], self.rev_depths[1], out=cat.slice(0, 2 * nf[0]))
                pre = cat
            p = f"{root}.sample_z_path.{k}"
            h = self._stack(plan, pre, [p + ".conv.0", p + ".conv.1"], p + ".conv.0", pre.C, self.rev_depths[0])
            lat = plan.latent_heads(h, p + ".mu_conv.0", p + ".sigma_conv.0", eps[k], f"{root}.lat{k}", want_z=want_z, act=0)
            lats.append(lat)
            zs.append(z_override[k] if z_override is not None else lat.z)
        return lats, zs

    def _likelihood(self, plan, zs, full, resize=True):
        """zs in draw order (k = 0 deepest), full: the size of the image / volume.  Returns the level logits resized to `full` and
        as the s_layers give them, both by level (index 0 finest).  resize=False emits no resize op and returns None for the first."""
        nf, L, root = self.num_filters, self._L, "likelihood"
        diff, depth = self._R - L, self.rev_depths[1]
        cats, post_c = {}, [None] * L

        def join(lvl, like):
            """Below the deepest level post_z[lvl]'s branch ends in a concat buffer (with the up-sampled post_c[lvl + 1],
            phiseg.py:303-305), sized like `like`: create it and return the branch's slice."""
            if lvl == L - 1:
                return None
            cats[lvl] = self._new_buf(plan, f"{root}.cat{lvl}", nf[lvl] + nf[lvl + 1 + diff], self._size(like))
            return cats[lvl].slice(0, nf[lvl])
        for k in range(L):
            lvl = L - 1 - k
            p = f"{root}.likelihood_ups_path.{k}"
            h = self._stack(plan, zs[k], [p + ".convolution.0", p + ".convolution.1"], p, nf[lvl], depth, out=join(lvl, zs[k]) if diff == 0 else None)
            for t in range(diff):
                h = self._up2(plan, h, f"{root}.ups{k}", t)
                h = conv_unit(plan, h, f"{root}.likelihood_post_ups_path.{k}.{2 * t + 1}.convolution.0", out=join(lvl, h) if t == diff - 1 else None)
            if lvl == L - 1:
                post_c[lvl] = h
        for lvl in reversed(range(L - 1)):
            cat = cats[lvl]
            self._up2(plan, post_c[lvl + 1], f"{root}.cat{lvl}", out=cat.slice(nf[lvl], nf[lvl + 1 + diff]))
            p = f"{root}.likelihood_post_c_path.{lvl}"
            post_c[lvl] = self._stack(plan, cat, [p + ".convolution.0", p + ".convolution.1"], p, nf[lvl + diff], depth)
        s, s_in = [None] * L, [None] * L
        for k in range(L):
            lvl = L - 1 - k
            s_in[lvl] = plan.conv_bare(post_c[lvl], f"{root}.s_layer.{k}.convolution.0.convolution.0")
            if resize:
                s[lvl] = self._nearest_full(plan, s_in[lvl], full, f"{root}.s{lvl}")
        return (s if resize else None), s_in

    def _build_predict_plan(self, N, full, part, resize=True):
        """The two plans of predict() at plan batch N for an image / volume of size `full`, both with eval-mode BatchNorm, fp32 storage
        and no loss or backward tape (_passes._b16_pass leaves a plan that is not bn_training alone, so neither is ever in bf16
        storage).  part = "trunk": patch -> the prior's contracting path (nothing in it depends on the noise).  part = "draw": the
        prior's latent path and the likelihood; the skip slices of its concat buffers and the deepest feature map are plan inputs that
        predict() fills from the trunk plan (no producer of this plan keeps a magnitude bound for them, so Plan.amax_in answers None
        for the mixed buffers and the split convolutions measure those tensors themselves).  io["feats"] lists the hand-over views,
        levels R-L .. R-2 and the deepest, in the same order in both plans.  resize=False: the draw plan ends at the un-resized level
        logits io["s_in"] and holds no resize op (io["s"] is None)."""
        nf, R, L, root = self.num_filters, self._R, self._L, "prior"
        plan = self._new_plan(N, False)
        plan.bn_prefixes_nbt = []
        io = {}
        if part == "trunk":
            io["patch"] = self._new_buf(plan, "patch", self.input_channels, full, requires_grad=False)
            skips, pre = self._contracting(plan, root, io["patch"])
        else:
            io["eps"] = self._latent_bufs(plan, "eps", L, full)
            skips = {i: self._new_buf(plan, f"{root}.cat{i}", 2 * nf[0] + nf[i], tuple(s >> i for s in full), requires_grad=False)
                     for i in range(R - L, R - 1)}
            pre = self._new_buf(plan, f"{root}.deepest", nf[R - 1], tuple(s >> (R - 1) for s in full), requires_grad=False)
            io["prior"], io["prior_z"] = self._latent_path(plan, root, skips, pre, io["eps"], None, True)
            io["s"], io["s_in"] = self._likelihood(plan, io["prior_z"], full, resize)
        io["feats"] = [skips[i].slice(2 * nf[0], nf[i]) for i in range(R - L, R - 1)] + [pre]
        plan.total = plan.vec("total", 1)
        plan.finalize(want_backward=False)
        plan.io = io
        return plan

    def _build_plan(self, N, full, training, bn_training, decode_only):
        """The plan of forward() + loss() at plan batch N for an image / volume of size `full`; decode_only: the likelihood alone on
        given latent samples (reconstruct() / sample())."""
        L = self._L
        plan = self._new_plan(N, bn_training)
        plan.bn_prefixes_nbt = []
        io = {}
        if decode_only:
            io["z_in"] = self._latent_bufs(plan, "z_in", L, full)
            io["s"], io["s_in"] = self._likelihood(plan, io["z_in"], full)
            plan.total = plan.vec("total", 1)
            plan.finalize(want_backward=False)
            plan.io = io
            return plan
        xin = self._inputs(plan, io, full)
        eps = io["eps"]
        post, post_z = self._encoder(plan, "posterior", xin, eps[:L], None, True)
        if training:       # prior sees the posterior samples (phiseg.py:417-418, 201-202)
            prior, prior_z = self._encoder(plan, "prior", io["patch"], eps[L:], post_z, False)
            s, s_in = self._likelihood(plan, post_z, full)
        else:
            prior, prior_z = self._encoder(plan, "prior", io["patch"], eps[L:], None, True)
            s, s_in = self._likelihood(plan, prior_z, full)
        io.update(s=s, s_in=s_in, post=post, prior=prior, post_z=post_z, prior_z=prior_z)
        # ---- loss: sum_l 4^l KL_l + sum_l CE_l (phiseg.py:455-513)
        plan.loss_phase()
        io["terms"] = plan.vec("loss_terms", 2 * L)
        plan.total = plan.vec("total", 1)
        io["loss_mask"] = self._new_buf(plan, "loss_mask", 1, full, requires_grad=False)
        for lvl in range(L):
            k = L - 1 - lvl
            w = float(self.exponential_weight ** lvl) if self.exponential_weighting else 1.0
            plan.kl(post[k], prior[k], w * self.kl_divergence_loss_weight, io["terms"].slice(lvl, 1))
        plan.residual_ce(s, io["loss_mask"], io["terms"].slice(L, L), post_scale=self._ce_post_scale(full))
        plan.sum_terms(io["terms"], 2 * L, plan.total)
        plan.finalize(want_backward=bn_training)
        plan.io = io
        return plan

    # ------------------------------------------------------------------ reference API
    def _publish(self, plan):
        """What forward() leaves on the model (phiseg.py:414-426): moments, samples and level logits by level, finest first."""
        io = plan.io
        order = [self._L - 1 - lvl for lvl in range(self._L)]        # level -> draw index
        V = self._boundary(plan)
        self.posterior_mu = [V(io["post"][k].mu) for k in order]
        self.posterior_sigma = [V(io["post"][k].sigma) for k in order]
        self.posterior_latent_space = [V(io["post_z"][k]) for k in order]
        self.prior_mu = [V(io["prior"][k].mu) for k in order]
        self.prior_sigma = [V(io["prior"][k].sigma) for k in order]
        self.prior_latent_space = [V(io["prior_z"][k]) for k in order]
        self.s_out_list = [V(v) for v in io["s"]]
        return self.s_out_list

    def loss(self, segm):
        return self.elbo(segm)

    def elbo(self, segm, reconstruct_posterior_mean=False):
        """phiseg.py:519-537.  Returns a 0-d tensor whose backward() runs the backward tape."""
        plan = self._cur
        if plan is None or "terms" not in plan.io:
            raise RuntimeError("call forward() before loss()")
        m = plan.tensor(plan.io["loss_mask"])
        m.copy_(self._to_slices(segm.reshape(self._to_volume(m).shape)))
        total = self._loss_value(plan)
        terms = plan.tensor(plan.io["terms"]).reshape(-1).clone()
        L = self._L
        self.loss_dict = {}
        for lvl in reversed(range(L)):
            self.loss_dict["KL_divergence_loss_lvl%d" % lvl] = terms[lvl]
        for lvl in reversed(range(L)):
            self.loss_dict["residual_multinoulli_loss_lvl%d" % lvl] = terms[L + lvl]
        self._publish_loss(total, terms)
        return total

    def kl_divergence(self):
        return self.kl_divergence_loss

    def sample_posterior(self):
        return [m + s * torch.randn_like(s) for m, s in zip(self.posterior_mu, self.posterior_sigma)]

    def sample_prior(self):
        return [m + s * torch.randn_like(s) for m, s in zip(self.prior_mu, self.prior_sigma)]

    def reconstruct(self, z_posterior, use_softmax=True):
        """Decode a list of latent samples (finest level first) through the likelihood (phiseg.py:403-405)."""
        self._require_gpu()
        dims = self._dims(z_posterior[0], self._R - self._L)
        plan = self._plan(("decode", *dims, bool(self.training)), lambda: self._build(*dims, False, bool(self.training), decode_only=True))
        for lvl, z in enumerate(z_posterior):
            plan.tensor(plan.io["z_in"][self._L - 1 - lvl]).copy_(self._to_slices(z))
        self._run(plan, "fwd")
        if self.training:
            self._bump_nbt(plan)
        V = self._boundary(plan)
        layer_recon = [V(v).clone() for v in plan.io["s"]]
        return self.accumulate_output(layer_recon, use_softmax=use_softmax), layer_recon

    def sample(self, testing=True):
        if testing:
            sample, _ = self.reconstruct(self.sample_prior(), use_softmax=False)
            return sample
        raise NotImplementedError

    # ------------------------------------------------------------------ the geometry: what a subclass supplies
    # rev_depths: reversible_depth of the (contracting / sample_z, up / likelihood) stacks;
    # _build(a, b, c, training, bn_training, decode_only=False) -> _build_plan;  _dims(t, shift=0): _build's (a, b, c) for a tensor `t`
    # at the API boundary whose spatial sizes are 2^shift below the image's;  _new_buf(plan, name, C, size, requires_grad=True);
    # _size(view);  _pool(plan, x, name);  _up2(plan, x, stem, t="", out=None): x2 up-sampling named stem + its tag + t;
    # _nearest_full(plan, s_in, full, name);  _inputs(plan, io, full): creates io["patch"], io["eps"] (2 L _latent_bufs) and returns
    # the posterior's input;  _publish_loss(total, terms);  accumulate_output(output_list, use_softmax).
    @staticmethod
    def _to_slices(t):
        """API boundary -> plan layout (the identity for images)."""
        return t

    _to_volume = _to_slices       # plan layout -> API boundary

    def _boundary(self, plan):
        """The function that takes a view of the plan to its tensor at the API boundary (forward() publishes 7 L of them per step)."""
        return plan.tensor

    @staticmethod
    def _ce_post_scale(full):
        return None
