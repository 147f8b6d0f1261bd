"""Operand layout of the tape ops: the ONE place that knows a slot number.

A tape op is a ``uz_op`` (include/uz_api.h): a code, 15 ints ``i[]``, 4 floats ``f[]``, a count ``n`` and 12 pointers ``p[]``.
What a slot means is defined by ``run_one()`` in csrc/tape.hip, which hands the slots to the C entry points; the table below
mirrors it op by op, in wire order, and everything on the Python side addresses operands through the names declared here.
Per op the table also says which ``p`` slots the op WRITES (every other one is read - the lane scheduler's hazards), which
``i`` slots select an optional form of the kernel (``opts``: all zero = the base form), and for the ops with a bf16-storage
form which tensor operand each bit of the ``b16`` slot describes.

Ops stay what they always were - dicts with the keys code / i / p / f / n / gid (/ lane) and plain positional lists, which
is what bench.py, the tools and the tests read.  ``Op`` adds access by name on top:

    op.i("x_packed")            op.i("N", "H", "W") -> [N, H, W]            op.p("y")
    op.set(i={"x_packed": 1, "x_seg2_c0": seg}, p={"x_amax2": s2})

``make()`` pads i / f with zeros and p with None to the schema's length - what the wire carries for an unset slot anyway - so
no reader ever has to ask how long an operand list is.
"""
from collections import namedtuple

Schema = namedtuple("Schema", "i p f writes opts b16 ix px fx")
SCHEMA = {}
B16_SLOT = 13          # i[] slot of the storage-format bits, the same in every op that has a bf16-storage form


def _op(code, i="", p="", f="", writes="", opts="", b16=""):
    i, p, f = i.split(), p.split(), f.split()
    if b16:
        i += [f"rsv{k}" for k in range(len(i), B16_SLOT)] + ["b16"]
    ix, px, fx = ({nm: k for k, nm in enumerate(lst)} for lst in (i, p, f))
    SCHEMA["UZ_OP_" + code] = Schema(tuple(i), tuple(p), tuple(f), tuple(px[w] for w in writes.split()), tuple(opts.split()),
                                     tuple(b16.split()), ix, px, fx)


# ---- convolutions (dy / dx: gradients w.r.t. the output / input; *_amax: magnitude-bound slots; w_image: pre-packed weights)
_op("CONV_FWD", i="cin ctot_x cout ctot_y N H W ks relu slabs_only x_packed x_seg2_c0 bn_in",
    p="x w bias y workspace x_amax w_amax y_amax w_image bn_partials x_amax2 bn_stats",
    writes="y bn_partials", opts="relu slabs_only x_packed x_seg2_c0 bn_in", b16="x y")
# fold: 1 = ReLU mask of the unit that produced x (fold_arg = its activation), 2 = + its BatchNorm-backward reduction (fold_arg = its
# pre-normalisation output, bn_stats / fold_relu = its statistics table / relu flag), 3 = slabs only INTO fold_arg (see writes())
_op("CONV_BWD_DATA", i="cout ctot_dy cin ctot_dx N H W ks accumulate ctot_fold fold dy_packed fold_relu",
    p="dy w dx workspace dy_amax w_amax w_image fold_arg partials dx_amax bn_stats",
    writes="dx partials dx_amax", opts="ctot_fold fold dy_packed fold_relu", b16="dy dx")
# nslab: the slab count `slabs` was sized for (checked at launch)
_op("CONV_BWD_WEIGHT", i="cin ctot_x cout ctot_dy N H W ks x_packed x_seg2_c0 dy_packed slabs_only nslab",
    p="x dy dw db workspace x_amax dy_amax x_amax2 slabs",
    writes="dw db slabs", opts="x_packed x_seg2_c0 dy_packed slabs_only nslab", b16="x dy")
# ---- BatchNorm + ReLU (phase: 1 = statistics only, 2 = apply only; slabs / conv_bias: the convolution's split-K slabs it adds)
_op("BN_RELU_FWD", i="C ctot_y ctot_a N H W training relu npart nslab a_packed phase", f="eps momentum",
    p="y gamma beta running_mean running_var save a workspace a_amax bn_partials slabs conv_bias",
    writes="running_mean running_var save a", opts="nslab a_packed phase", b16="y a")
# da_partials: reduction partials (npart) or split-K slabs of dA (nslab) left by the data gradient that wrote dA
_op("BN_RELU_BWD", i="ctot_da C ctot_y ctot_dy N H W relu npart dy_packed dbias_rows nslab",
    p="da y gamma beta save dy dgamma dbeta dbias workspace dy_amax da_partials",
    writes="dy dgamma dbeta dbias", opts="npart dy_packed dbias_rows nslab", b16="da y dy")
_op("RELU_BWD", i="ctot_da C ctot_a ctot_dy N H W", p="da a dy dbias workspace dy_amax", writes="dy dbias")
# ---- resampling (a / partials / dx_amax: folded ReLU backward of the unit that produced x)
_op("AVGPOOL_FWD", i="C ctot_x ctot_y N H W y_packed", p="x y x_amax y_amax", writes="y")
_op("AVGPOOL_BWD", i="C ctot_dy ctot_dx N H W accumulate ctot_a", p="dy dx a partials dx_amax", writes="dx partials dx_amax")
_op("BILINEAR_FWD", i="C ctot_x ctot_y N H W align_corners y_packed", p="x y x_amax y_amax", writes="y", opts="y_packed", b16="x y")
_op("BILINEAR_BWD", i="C ctot_dy ctot_dx N H W align_corners accumulate ctot_a", p="dy dx a partials dx_amax",
    writes="dx partials dx_amax", opts="ctot_a", b16="dy dx")
_op("NEAREST_FWD", i="C ctot_x ctot_y N H W factor", p="x y", writes="y")
_op("NEAREST_BWD", i="C ctot_dy ctot_dx N H W factor accumulate", p="dy dx", writes="dx")
_op("SPATIAL_MEAN_FWD", i="C ctot_x N H W", p="x y", writes="y")
_op("SPATIAL_MEAN_BWD", i="C ctot_dx N H W accumulate", p="dy dx", writes="dx")
_op("AVGPOOL3D_FWD", i="C ctot_x ctot_y D H W", p="x y", writes="y", b16="x y")
_op("AVGPOOL3D_BWD", i="C ctot_dy ctot_dx D H W accumulate", p="dy dx", writes="dx", b16="dy dx")
_op("DEPTH_LERP_FWD", i="C ctot_x ctot_y D H W", p="x y", writes="y", b16="x y")
_op("DEPTH_LERP_BWD", i="C ctot_dy ctot_dx D H W accumulate", p="dy dx", writes="dx", b16="dy dx")
_op("NEAREST3D_FWD", i="C ctot_x ctot_y D H W factor factor_z", p="x y", writes="y")
_op("NEAREST3D_BWD", i="C ctot_dy ctot_dx D H W factor factor_z accumulate", p="dy dx", writes="dx")
_op("ADD_VIEWS", i="ctot_a ctot_b ctot_y C N H W accumulate", f="alpha", p="a b y a_amax b_amax y_amax", writes="y")
_op("BCAST_CHANNELS", i="L ctot_out N H W", p="z out", writes="out")
_op("BCAST_CHANNELS_BWD", i="ctot_dout L N H W", p="dout dz", writes="dz")
_op("W3D_PERMUTE", i="cout cin mode", p="src dst", writes="dst")
# ---- inputs, latents, losses
_op("POSTERIOR_INPUT", i="C nlabels N H W", p="patch mask out", writes="out")
_op("LATENT_FWD", i="act", p="mu pre eps sigma z", writes="sigma z")
_op("LATENT_BWD", i="act", p="kl_dmu kl_dsigma dz eps sigma dmu dpre", writes="dmu dpre")
_op("LATENT_HEADS_FWD", i="cin ctot_h L N H W act", p="h w_mu b_mu w_sigma b_sigma eps mu pre sigma z", writes="mu pre sigma z")
_op("LATENT_HEADS_BWD_DATA", i="L cin ctot_h N H W accumulate", p="dy_a dy_b w_a w_b dh", writes="dh")
_op("LATENT_HEADS_BWD_WEIGHT", i="cin ctot_h L N H W", p="h dy_a dy_b dw_a db_a dw_b db_b workspace", writes="dw_a db_a dw_b db_b")
_op("KL_FWD", i="n per", f="weight", p="q_mu q_sigma p_mu p_sigma term workspace", writes="term")
_op("KL_BWD", i="n per", f="weight", p="q_mu q_sigma p_mu p_sigma scale dq_mu dq_sigma dp_mu dp_sigma", writes="dq_mu dq_sigma dp_mu dp_sigma")
_op("CE_FWD", i="L K N H W", p="logits mask terms workspace", writes="terms")
_op("CE_BWD", i="L K N H W", p="logits dlogits mask scale", writes="dlogits")
_op("SUM_TERMS", i="n", p="terms total", writes="total")
_op("ACC_SOFTMAX_ARGMAX", i="L K N H W", p="logits acc soft label", writes="acc soft label")
_op("L2_NORMS", i="n", p="params table norms", writes="norms")
_op("L2_NORMS_BWD", i="n", p="params table norms scale grads", writes="grads")           # grads: the gradient ranges it adds to
# ---- element-wise / bookkeeping (n = element or byte count)
_op("ADAM", i="step lr_bits", f="beta1 beta2 eps weight_decay", p="params grads exp_avg exp_avg_sq", writes="params exp_avg exp_avg_sq")
_op("AXPY", f="alpha", p="y x", writes="y")
_op("SCALE", f="alpha", p="x", writes="x")
_op("MEMSET", p="dst", writes="dst")
_op("COPY", p="dst src", writes="dst")
_op("ABSMAX", p="src slot", writes="slot")
_op("ABSMAX_COPY", p="src_slot dst_slot")
_op("EVENT_RECORD", p="event range", writes="event")                                     # range: the gradient range the event stands for (scheduling only)
_op("PACK_WEIGHTS", i="n_layers total_rows", p="table w_amax images", writes="images")
_op("CHAN_SUM_TABLE", i="n_entries max_channels", p="table grads", writes="grads")
_op("WGRAD_REDUCE_TABLE", i="n_layers total_blocks", p="table grads", writes="grads")
_op("CHAN_SUM_PARTIALS", i="n_rows C doubles", p="partials out", writes="out")
_op("CHAIN", i="n_phases n_workgroups n_sub_ops", p="ops phases state")                  # (its accesses: the union of its sub-ops', Plan._access)
_op("CHAIN_PACK", i="n_layers total_blocks", p="table w_amax images", writes="images")

CONV_KIND = {"UZ_OP_CONV_FWD": 0, "UZ_OP_CONV_BWD_DATA": 1, "UZ_OP_CONV_BWD_WEIGHT": 2}      # the `kind` of uz_conv_route
# Split storage (csrc/split_f16.h): ops that may WRITE a buffer kept as operand pieces - (view, bound it scales by, flag) - and ops
# that may READ one: (view, bound, bound and first channel of the second scale segment, flag)
SPLIT_WRITERS = {"UZ_OP_BN_RELU_FWD": ("a", "a_amax", "a_packed"), "UZ_OP_BILINEAR_FWD": ("y", "y_amax", "y_packed"),
                 "UZ_OP_AVGPOOL_FWD": ("y", "y_amax", "y_packed")}
SPLIT_READERS = {"UZ_OP_CONV_FWD": ("x", "x_amax", "x_amax2", "x_seg2_c0", "x_packed"),
                 "UZ_OP_CONV_BWD_WEIGHT": ("x", "x_amax", "x_amax2", "x_seg2_c0", "x_packed")}
WRITES = {code: s.writes for code, s in SCHEMA.items()}                                 # static part of writes()


class Op(dict):
    """One tape op: the plain dict everybody reads, plus access to its operands by schema name."""
    __slots__ = ()

    def _get(self, key, index, names):
        lst = self[key]
        return lst[index[names[0]]] if len(names) == 1 else [lst[index[nm]] for nm in names]

    def i(self, *names):
        return self._get("i", SCHEMA[self["code"]].ix, names)

    def p(self, *names):
        return self._get("p", SCHEMA[self["code"]].px, names)

    def f(self, *names):
        return self._get("f", SCHEMA[self["code"]].fx, names)

    def set(self, i=None, p=None):
        s = SCHEMA[self["code"]]
        for nm, v in (i or {}).items():
            self["i"][s.ix[nm]] = int(v)
        for nm, v in (p or {}).items():
            self["p"][s.px[nm]] = v
        return self

    def clone(self, **extra):
        """A new op with operand lists of its own; every other key is shared unless `extra` replaces it."""
        return Op(self, i=list(self["i"]), p=list(self["p"]), f=list(self["f"]), **extra)

    def base_form(self):
        """No optional form of the kernel selected."""
        return not any(self["i"][SCHEMA[self["code"]].ix[nm]] for nm in SCHEMA[self["code"]].opts)


def _fill(given, names, index, pad, conv):
    if isinstance(given, dict):
        out = [pad] * len(names)
        for nm, v in given.items():
            out[index[nm]] = conv(v)
        return out
    out = [conv(v) for v in given]
    assert len(out) <= len(names), (names, out)
    return out + [pad] * (len(names) - len(out))


def make(code, p=(), i=(), f=(), n=0, gid=None, **extra):
    """New op; p / i / f in wire order or as {name: value}, padded to the schema's length (None / 0 / 0.0)."""
    s = SCHEMA[code]
    return Op(code=code, p=_fill(p, s.p, s.px, None, lambda r: r), i=_fill(i, s.i, s.ix, 0, int), f=_fill(f, s.f, s.fx, 0.0, float),
              n=int(n), gid=gid, **extra)


def writes(op):
    """p[] slots op `op` writes: the schema's, except for a slabs-only data gradient (partial sums into fold_arg; its gradient view dx
    is NOT written - the consumer's BatchNorm backward reads the slabs instead) and the two phases of a split BatchNorm forward
    (1: statistics table + running buffers, 2: the activation only)."""
    code = op["code"]
    s = SCHEMA[code]
    if code == "UZ_OP_CONV_BWD_DATA" and op.i("fold") == 3:
        return (s.px["fold_arg"],)
    if code == "UZ_OP_BN_RELU_FWD" and op.i("phase"):
        return tuple(s.px[nm] for nm in (("running_mean", "running_var", "save") if op.i("phase") == 1 else ("a",)))
    return s.writes


def b16_slots(op):
    """(p[] slot, bit of the b16 slot) of the tensor operands of `op` that may be bf16; () = no bf16-storage form.  A 1x1 head
    takes only its many-channel side (x / dx) in bf16, the in-plane interpolation only its high-resolution side."""
    code = op["code"]
    s = SCHEMA[code]
    names = s.b16
    if code in CONV_KIND and names and op.i("ks") == 1:
        names = {0: ("x",), 1: (None, "dx"), 2: ("x",)}[CONV_KIND[code]]
    elif code == "UZ_OP_BILINEAR_FWD":
        names = (None, "y")
    elif code == "UZ_OP_BILINEAR_BWD":
        names = ("dy",)
    return tuple((s.px[nm], bit) for bit, nm in enumerate(names) if nm is not None)


def conv_dims(op):
    """(kind, cin, cout, N, H, W, ks) of a convolution op, cin / cout those of the LAYER whatever the direction."""
    return (CONV_KIND[op["code"]], *op.i("cin", "cout", "N", "H", "W", "ks"))
