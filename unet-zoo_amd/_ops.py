"""Operand layout of the tape ops, read from include/uz_ops.def: the table is the single source of the tape encoding.

A tape op is a ``uz_op`` (include/uz_api.h): a code, 15 ints ``i[]``, 4 floats ``f[]``, a count ``n`` and 12 pointers ``p[]``.
What a slot means is written down once, in the table include/uz_ops.def: ``run_one()`` in csrc/tape.hip hands the slots to the C
entry points by the table's names, and everything on the Python side addresses operands through the same names (``SCHEMA`` below
is the table, parsed).  Per op the table also says which ``p`` slots the op WRITES (every other one is read - the lane scheduler's
hazards), which ``i`` slots select an optional form of the kernel (``opts``: all zero = the base form), and for the ops with a
bf16-storage form which tensor operand each bit of the ``b16`` slot describes.

Ops stay what they always were - dicts with the keys code / i / p / f / n / gid (/ lane) and plain positional lists, which
is what bench.py, the tools and the tests read.  ``Op`` adds access by name on top:

    op.i("x_packed")            op.i("N", "H", "W") -> [N, H, W]            op.p("y")
    op.set(i={"x_packed": 1, "x_seg2_c0": seg}, p={"x_amax2": s2})

``make()`` pads i / f with zeros and p with None to the schema's length - what the wire carries for an unset slot anyway - so
no reader ever has to ask how long an operand list is.
"""
from collections import namedtuple

from . import _ffi

Schema = namedtuple("Schema", "i p f writes opts b16 ix px fx")
B16_SLOT, _TABLE = _ffi.op_table()          # B16_SLOT: i[] slot of the storage-format bits, the same in every op that has a bf16-storage form


def _schema(t):
    i = t["I"] + ([f"rsv{k}" for k in range(len(t["I"]), B16_SLOT)] + ["b16"] if t["B16"] else [])
    assert len(i) <= B16_SLOT + 1, i
    ix, px, fx = ({nm: k for k, nm in enumerate(lst)} for lst in (i, t["P"], t["F"]))
    return Schema(tuple(i), tuple(t["P"]), tuple(t["F"]), tuple(px[w] for w in t["WRITES"]), tuple(t["OPTS"]), tuple(t["B16"]), ix, px, fx)


SCHEMA = {code: _schema(t) for code, t in _TABLE}
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
