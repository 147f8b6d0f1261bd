"""Static execution plan ("tape") builder.

A model instance flattens itself, for a given (batch, H, W, mode), into three lists of C-ABI
calls - forward, loss, backward - over pre-allocated device buffers.  Shapes are static, so the
lists are built once, turned into ``uz_op`` arrays and replayed with one FFI call per pass
(``uz_run_tape``) or as a captured hipGraph.  Nothing here computes on the host: the plan only
decides *which* kernel runs on *which* buffer.

Design points:
  * concat-free: a producer writes straight into a channel slice of the consumer's buffer
    (``View`` = buffer + channel offset), replacing torch.cat (phiseg.py:71,183,315; unet.py:72);
  * gradient fan-in is resolved at plan time: the first backward writer of a gradient region
    overwrites, later writers accumulate (no zero-fill passes);
  * branches whose output never reaches the loss are skipped in backward, which reproduces the
    reference's ``grad is None`` parameters.

This module holds the builder proper: the storage classes, the emitters the models call, ``finalize`` with the arena layout,
the resolution of symbolic operand refs into addresses and the access sets of the ops.  What ``finalize`` runs over the emitted
tapes lives beside it: ``_passes.py`` (split storage, BatchNorm off-chain, bf16 storage), ``_chain_plan.py`` (the deep-level
chain, off by default) and ``_sched.py`` (hazard analysis, cost models, the lane scheduler).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _ffi, _knobs, _ops, _sched
from ._ops import conv_dims

BN_EPS = 1e-3        # reference torchlayers.py:20
BN_MOMENTUM = 0.01   # reference torchlayers.py:20
_ALIGN = 64          # floats
_AMAX_FLOATS = 256   # floats per magnitude-bound slot: 16 sub-slots 64 bytes apart (csrc/split_f16.h)


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


# ----------------------------------------------------------------------------------------------
class ParamTable:
    """Flat fp32 storage for all parameters / BN buffers of a model, addressed by the
    reference's state_dict keys.  spec: ordered [(key, shape, kind)], kind in
    conv_w conv_b bn_w bn_b bn_rm bn_rv bn_nbt (same vocabulary as the golden fixtures)."""

    def __init__(self, spec, device):
        self.spec = [(k, tuple(s), kd) for k, s, kd in spec]
        self.device = device
        self.poff, self.boff, self.shape, self.kind = OrderedDict(), OrderedDict(), {}, {}
        po = bo = 0
        self.nbt_keys = []
        for k, s, kd in self.spec:
            self.shape[k], self.kind[k] = s, kd
            if kd in ("conv_w", "conv_b", "bn_w", "bn_b"):
                self.poff[k] = po
                po += _numel(s)
            elif kd in ("bn_rm", "bn_rv"):
                self.boff[k] = bo
                bo += _numel(s)
            elif kd == "bn_nbt":
                self.nbt_keys.append(k)
            else:
                raise ValueError(kd)
        self.n_params, self.n_buffers = po, bo
        self.pflat = torch.zeros(max(po, 1), dtype=torch.float32, device=device)
        self.gflat = torch.zeros(max(po, 1), dtype=torch.float32, device=device)
        self.bflat = torch.zeros(max(bo, 1), dtype=torch.float32, device=device)
        self.nbt = torch.zeros(max(len(self.nbt_keys), 1), dtype=torch.int64, device=device)
        self._gviews = {}                   # key -> cached gradient view, filled by gview()

    def pview(self, k):
        o = self.poff[k]
        return self.pflat[o:o + _numel(self.shape[k])].view(self.shape[k])

    def gview(self, k):
        """View of parameter k's gradient in the flat buffer.  The view OBJECTS are cached (the buffer never moves): a backward pass
        re-attaches ~400 of them and the optimiser compares them by identity - slicing them anew cost 2 ms of host time per step."""
        cache = self._gviews
        v = cache.get(k)
        if v is None:
            o = self.poff[k]
            v = cache[k] = self.gflat[o:o + _numel(self.shape[k])].view(self.shape[k])
        return v

    def bview(self, k):
        o = self.boff[k]
        return self.bflat[o:o + _numel(self.shape[k])].view(self.shape[k])

    def nbtview(self, k):
        return self.nbt[self.nbt_keys.index(k)]


class Buf:
    __slots__ = ("name", "N", "C", "H", "W", "off", "gbuf", "requires_grad", "amax", "amax_cov", "alias", "relu", "packed", "b16", "vol")

    def __init__(self, name, N, C, H, W, requires_grad=True):
        self.name, self.N, self.C, self.H, self.W = name, int(N), int(C), int(H), int(W)
        self.off, self.gbuf, self.requires_grad = None, None, requires_grad
        self.amax, self.amax_cov = None, []      # magnitude-bound slot and the channel ranges whose producers maintain it
        self.alias = None                        # pooled scratch: several differently shaped Bufs share one arena region
        self.relu = None                         # set by Plan.conv_relu: {(c0, C): state} of Conv -> ReLU units writing into this buffer
        self.packed = False                      # kept in split storage (_passes._split_storage_passes): Plan.tensor() of it is NOT fp32 values
        self.b16 = False                         # kept in bf16 storage (_passes._b16_pass): 2-byte elements, Plan.tensor() of it is a bfloat16 tensor
        self.vol = False                         # a volume (Plan.vol): [D + 2][C][H][W]

    @property
    def numel(self):
        return self.N * self.C * self.H * self.W

    @property
    def words(self):
        """32-bit words of arena the buffer occupies."""
        return (self.numel + 1) // 2 if self.b16 else self.numel

    @property
    def esz(self):
        return 2 if self.b16 else 4


class View:
    """Channel slice [c0, c0+C) of a buffer, optionally restricted to the batch entries [b0, b0+nb) (volumes: the D real
    slices between the two zero slices, see Plan.vol)."""
    __slots__ = ("buf", "c0", "C", "b0", "nb")

    def __init__(self, buf, c0=0, C=None, b0=0, nb=None):
        self.buf, self.c0, self.C = buf, c0, buf.C - c0 if C is None else C
        self.b0, self.nb = b0, nb
        assert 0 <= self.c0 and self.c0 + self.C <= buf.C

    N = property(lambda s: s.buf.N if s.nb is None else s.nb)
    H = property(lambda s: s.buf.H)
    W = property(lambda s: s.buf.W)
    Ctot = property(lambda s: s.buf.C)

    def slice(self, c0, C):
        return View(self.buf, self.c0 + c0, C, self.b0, self.nb)

    @property
    def contiguous(self):
        return self.c0 == 0 and self.C == self.buf.C

    @property
    def numel(self):
        return self.N * self.C * self.H * self.W


def _buf_of(r):
    """The Buf behind one operand ref - a view, a dy that has a buffer of its own, a volume's depth window - or None."""
    if isinstance(r, tuple) and r and r[0] == "win":
        r = r[1]
    if isinstance(r, _ScratchView):
        r = r.view
    return r.buf if isinstance(r, View) else None


class Latent:
    """One (mu, sigma, z) head: SampleZBlock tail (phiseg.py:99-106) or AxisAlignedConvGaussian
    (probabilistic_unet.py:124-129)."""
    def __init__(self, mu, pre, sigma, z, eps, act):
        self.mu, self.pre, self.sigma, self.z, self.eps, self.act = mu, pre, sigma, z, eps, act
        self.kl_dmu = self.kl_dsigma = None


# ----------------------------------------------------------------------------------------------
class Plan:
    def __init__(self, N, ptab, bn_training, device, knobs=None):
        self.N, self.ptab, self.bn_training, self.device = int(N), ptab, bool(bn_training), device
        # the UZ_* switches this plan is built AND rescheduled under: NativeModel._new_plan reads them over the model's defaults, a bare Plan over the table's
        self.knobs = knobs if knobs is not None else _knobs.read()
        self.codes = _ffi.op_codes()
        self.L = _ffi.lib()
        self.bufs = []
        self.fwd_ops, self.loss_ops, self.bwd_ops = [], [], []
        self.extra_ops = {}                 # additional forward-only tapes (e.g. "decode")
        self.target = self.fwd_ops
        self._bwd = []                      # closures, run in reverse
        self._bwd_tail = []                 # closures run after all others (regulariser gradients)
        self._bwd_head = []                 # closures run before all others (re-materialised backward inputs)
        self._record_bwd = True
        self._ginit = {}                    # Buf -> list of (c0, c1) gradient regions already written
        self.scratch = dict(bn=0, wgrad=0, gy=0, ce=0)   # bytes (bn, wgrad, ce) / floats (gy)
        self.ptr_tables = []                # list of lists of pointer refs -> device int64 table
        self.param_grads = []               # parameter keys that receive a gradient, in write order
        self.named = {}                     # user-visible tensors: name -> View
        self.finalized = False
        # Magnitude bounds for the split-fp16 convolutions: slot 0 bounds |parameters| (measured at the head of the forward
        # tape), one slot per activation buffer (atomic-max maintained by the kernels that write it) and one per Conv unit for
        # the gradient w.r.t. its output.  Forward-side slots are zeroed at the head of the forward tape, backward-side slots
        # at the head of the backward tape.
        self.n_amax, self.n_amax_fwd = 1, None
        self._amax_bwd = []                 # slot indices used by backward producers
        self._packs = {"fwd": {}, "bwd": {}}   # pre-packed split-fp16 weight images: wkey -> geometry (see _packed)
        self._packbuf = {}
        self.grad_buckets = []              # [(lo, hi)] float ranges of the flat gradient buffer that get a "final" event (data parallel)
        self.events = []                    # hipEvent_t handles (uz_event_create), one per gradient bucket
        self._gid = 0                       # scheduling group of the ops being emitted (see _sched.schedule)
        self._gyz = {}                       # zero-bordered dy scratch classes of volume units: (slices, floats per slice) -> floats
        self.n_lanes = max(1, min(self.knobs.lanes, 8))      # (NativeModel._new_plan lowers it to the stream budget)
        self._nclaims = {}                   # backward writers seen per buffer (conv_relu's folded ReLU backward checks it was the last one)
        self._dbias_jobs = []                # folded ReLU backward: bias gradients still to be summed from their partials (one launch at the tape's end)
        self._chains = []                    # per chain op: dict(sub=[...], phases=[...]) -> device tables built on first resolve
        self._chain_imgs = {}                # tape -> {wkey: dict(off, bytes, mc, kc, cin, dgrad)} packed weight images of the chain convolutions
        self._chain_imgbuf = {}
        self._detached = 0                   # groups of their own handed out so far (_emit(detached=True), _passes._bn_offchain_pass)
        self._wgrad_jobs = []                # weight-gradient slabs still to be summed (_conv_bwd); finalize() turns them into table launches
        self._units = []                     # Conv2D units of the forward tape (conv_bn_relu), for _passes._split_storage_passes / _bn_offchain_pass
        self._vol_units = []                 # backward ops of the volume units sharing a zero-bordered dy scratch (conv_bn_relu), for _passes._b16_pass
        self._win_of = {}                    # wkey -> the copy a 3x3x3 convolution reads through its depth window (_window_input)
        self._rev_ctx = None                 # branch of the reversible block being emitted (_rev_block), else None
        self._vol_depth = None               # depth of the volume a reversible sequence works on (rev_sequence, _rev_block): shapes _pool's scratch
        self._rev_pool, self._rev_slots = {}, {}   # pooled scratch of the reversible blocks and the arena regions it shares (_pool; laid out by finalize)
        self.sched_cost = self.knobs.sched_cost   # cost model of the lane scheduler, "alone" | "beside" (its device-filling rule: knobs.sched_heavy)
        self.dag = {}                        # id(tape) -> the scheduled DAG, for diagnostics (_schedule)
        self.round4, self.bn_offchain, self.b16_info = {}, {}, {}   # summaries of _passes._split_storage_passes / _bn_offchain_pass / _b16_pass
        self.chain_info = {}                 # tape -> summaries of its chains (_chain_plan._chain_pass)
        # the models' own handles: io (dict of views), total (the loss), bn_prefixes_nbt* (BatchNorm counters a tape bumps: _engine.conv_unit)
        self.io, self.total = None, None
        self.bn_prefixes_nbt, self.bn_prefixes_nbt_loss, self.bn_prefixes_nbt_bwd, self.bn_prefixes_nbt_extra = [], [], [], []
        self._nbt_idx = {}                   # which of those lists -> its counters' indices on the device (NativeModel._bump_nbt)
        self._warm = set()                   # tapes that had their eager warm-up run before graph capture (NativeModel._run)
        self.host = {}                       # what a model keeps with this plan between calls (device pointer tables, the noise span, predict() outputs)
        # filled by finalize(): the loss-scale cell, the bound-slot numbering, the arena and its layout, the pointer tables, the tapes
        self.loss_scale = self.loss_scale_t = None
        self._amax_remap = {}
        self.gy_off, self.scratch_off, self.gyz_off = [], [], []      # per lane
        self.amax_off = self.arena_floats = self.arena = self.base = None
        self.ptrtab, self._tab_off = None, []
        self.tapes, self.scheds, self._program_order = {}, {}, {}     # per tape: (uz_op array, n), uz_sched array, ops in program order

    def _newgroup(self):
        self._gid += 1

    # ------------------------------------------------------------------ buffers
    def buf(self, name, C, H, W, N=None, requires_grad=True):
        b = Buf(name, self.N if N is None else N, C, H, W, requires_grad)
        self.bufs.append(b)
        return View(b)

    def vec(self, name, n, requires_grad=False):
        """Small 1-D float region (loss terms, saved BN statistics, ...)."""
        return self.buf(name, n, 1, 1, N=1, requires_grad=requires_grad)

    def gview(self, v):
        if v.buf.gbuf is None:
            g = Buf("grad:" + v.buf.name, v.buf.N, v.buf.C, v.buf.H, v.buf.W, False)
            g.vol = v.buf.vol
            self.bufs.append(g)
            v.buf.gbuf = g
        return View(v.buf.gbuf, v.c0, v.C, v.b0, v.nb)

    def vol(self, name, C, D, H, W, requires_grad=True):
        """One volume (models/phiseg3D.py): [D + 2][C][H][W] with a zero slice on either side of the D real ones (csrc/vol.hip);
        the returned view addresses the real slices as a batch of D images.  The arena is zero-initialised and nothing ever
        writes the two border slices, so they ARE the depth padding of the 3x3x3 convolutions."""
        b = Buf(name, D + 2, C, H, W, requires_grad)
        b.vol = True
        self.bufs.append(b)
        return View(b, 0, C, 1, D)

    # ------------------------------------------------------------------ magnitude bounds
    def _new_amax(self, bwd=False):
        k = self.n_amax
        self.n_amax += 1
        if bwd:
            self._amax_bwd.append(k)
        return k

    def amax_out(self, v):
        """Slot reference a producer of view `v` accumulates max|v| into (creates the buffer's slot on first use)."""
        if isinstance(v, _ScratchView):
            return ("amax", v.amax, "acc") if v.amax is not None else None
        b = v.buf
        if b.amax is None:
            b.amax = self._new_amax()
        b.amax_cov.append((v.c0, v.c0 + v.C))
        return ("amax", b.amax, "acc")       # third element: this op ACCUMULATES into the slot (see _access)

    def amax_in(self, v):
        """Slot reference bounding |v| for a consumer, or None when some producer of its channels keeps no bound
        (the kernel then measures the tensor itself)."""
        if isinstance(v, _ScratchView):
            return ("amax", v.amax) if v.amax is not None else None
        b = v.buf
        if b.amax is None:
            return None
        ok = all(any(a <= c < e for a, e in b.amax_cov) for c in range(v.c0, v.c0 + v.C))
        return ("amax", b.amax) if ok else None

    def _claim(self, v):
        """Returns the accumulate flag for a backward write to grad(v) and records the region."""
        regs = self._ginit.setdefault(v.buf, [])
        self._nclaims[v.buf] = self._nclaims.get(v.buf, 0) + 1
        lo, hi = v.c0, v.c0 + v.C
        covered = [c for c in range(lo, hi) if any(a <= c < b for a, b in regs)]
        if len(covered) == hi - lo:
            return 1
        if covered:
            raise RuntimeError(f"partial gradient overlap on {v.buf.name}[{lo}:{hi}] vs {regs}")
        regs.append((lo, hi))
        return 0

    def _has_grad(self, v):
        regs = self._ginit.get(v.buf, [])
        return all(any(a <= c < b for a, b in regs) for c in range(v.c0, v.c0 + v.C))

    # ------------------------------------------------------------------ op emission
    def _emit(self, lst, code, p=(), i=(), f=(), n=0, detached=False):
        """p / i / f: operands in wire order or by name (_ops.make pads them to the op's schema).
        detached: a scheduling group of its own, whatever is emitted around it (parameter-only preparation ops: they are ready at
        the head of the tape and must not sit in a layer's chain)."""
        gid = self._gid
        if detached:
            self._detached += 1
            gid = ("detached", self._detached)
        op = _ops.make(code, p, i, f, n, gid)
        lst.append(op)
        return op

    def P(self, key, extra=0):
        return ("param", key, extra)

    def G(self, key, extra=0):
        if key not in self.param_grads:
            self.param_grads.append(key)
        return ("pgrad", key, extra)

    def B(self, key):
        return ("buffer", key, 0)

    def loss_phase(self):
        self.target = self.loss_ops

    def extra_phase(self, name):
        """Switch to an extra forward-only tape (no backward is recorded for its ops)."""
        self.target = self.extra_ops.setdefault(name, [])
        self._record_bwd = False

    def _push_bwd(self, fn):
        if self._record_bwd:
            self._bwd.append(fn)

    def in_loss_phase(self):
        return self.target is self.loss_ops

    def _tables_ok(self):
        """Deferred table-driven reductions (weight-gradient slabs, bias-gradient rows).  Data parallel: a bucket's gradients must be
        final when its all-reduce starts, so there the tables are cut per BUCKET (finalize(): one launch per bucket, and the bucket's
        "final" marker depends on it through the gradient ranges it writes); UZ_DP_TABLES=0 restores one reduction launch per layer."""
        return not self.grad_buckets or self.knobs.dp_tables

    def _by_bucket(self, jobs, key_of):
        """jobs split by the gradient bucket their parameter lies in (one group when there are no buckets), emission order kept."""
        if not self.grad_buckets:
            return [jobs]
        groups = [[j for j in jobs if lo <= self.ptab.poff[key_of(j)] < hi] for lo, hi in self.grad_buckets]
        assert sum(len(g) for g in groups) == len(jobs), "a deferred reduction's parameter lies outside every gradient bucket"
        return [g for g in groups if g]

    def l2_reg(self, keys, term, coeff):
        """coeff * sum_k ||p_k||_2 over the listed parameter tensors (utils.l2_regularisation, utils.py:93-101)."""
        n = len(keys)
        tab = self.ptr_table([("raw", v) for k in keys for v in (self.ptab.poff[k], _numel(self.ptab.shape[k]))])
        norms = self.vec("l2_norms", n)
        self._newgroup()
        self._emit(self.target, "UZ_OP_L2_NORMS", p=[("pflat",), tab, norms], i=[n])
        self._emit(self.target, "UZ_OP_SUM_TERMS", p=[norms, term], i=[n])
        self._emit(self.target, "UZ_OP_SCALE", p=[term], f=[coeff], n=1)

        def tail():
            sc = self.vec("l2_scale", 1)
            self._emit(self.bwd_ops, "UZ_OP_COPY", p=[sc, self.loss_scale], n=4)
            self._emit(self.bwd_ops, "UZ_OP_SCALE", p=[sc], f=[coeff], n=1)
            # the write set is the listed tensors' gradient ranges only: with the whole flat buffer declared, every
            # gradient bucket's "final" marker waited for this op and the data-parallel overlap collapsed to one exchange
            self._emit(self.bwd_ops, "UZ_OP_L2_NORMS_BWD", p=[("pflat",), tab, norms, sc, ("gflat_keys", tuple(keys))], i=[n])
        self._bwd_tail.append(tail)

    # ------------------------------------------------------------------ convolution family
    def _conv_fwd(self, x, wkey, bkey, y, ks, relu, wrow0=0, bn_partials=None, slabs_only=False):
        cout = y.C
        cin = x.C
        if len(self.ptab.shape[wkey]) == 5 and x.nb is None:
            raise RuntimeError(f"{wkey} is a Conv3d weight but its input {x.buf.name} is not a volume")
        if x.nb is not None and ks == 3:
            # Conv3d(3x3x3, pad 1) on a volume = the 2-D kernel over the D slices with the depth window as 3 Cin input channels
            # (csrc/vol.hip); the weights are permuted to [co][kd][ci][3][3] first
            assert wrow0 == 0
            x = self._window_input(x, wkey)
            ws = self.L.uz_conv_workspace(3 * cin, cout, x.N, x.H, x.W, 3)
            self.scratch["wgrad"] = max(self.scratch["wgrad"], ws)
            self._newgroup()
            packed = self._packed(wkey, cin, cout, x, False, vol=True)
            wp = self.P(wkey)                                  # (unused by the kernel when the image is pre-packed)
            if packed is None:
                wp = self.vec(wkey + ":w3d_fwd", cout * cin * 27)
                self._emit(self.target, "UZ_OP_W3D_PERMUTE", p=[self.P(wkey), wp], i=[cout, cin, 0], detached=True)
            self._emit(self.target, "UZ_OP_CONV_FWD",
                       p=[("win", x), wp, self.P(bkey) if bkey else None, y, ("scratch", "wgrad"), self.amax_in(x), ("amax", 0),
                          self.amax_out(y) if relu else None, packed, bn_partials],
                       i=[3 * cin, x.Ctot, cout, y.Ctot, x.N, x.H, x.W, 3, relu], n=ws)
            return
        wextra = wrow0 * cin * ks * ks
        ws = self.L.uz_conv_workspace(cin, cout, x.N, x.H, x.W, ks)
        self.scratch["wgrad"] = max(self.scratch["wgrad"], ws)
        self._newgroup()
        packed = self._packed(wkey, cin, cout, x, False) if (ks == 3 and wrow0 == 0) else None
        self._emit(self.target, "UZ_OP_CONV_FWD",
                   p=[x, self.P(wkey, wextra), self.P(bkey, wrow0) if bkey else None, y, ("scratch", "wgrad"),
                      self.amax_in(x), ("amax", 0), self.amax_out(y) if (relu and ks == 3) else None, packed, bn_partials],
                   i=[cin, x.Ctot, cout, y.Ctot, x.N, x.H, x.W, ks, relu, int(slabs_only)], n=ws)

    def _conv_bwd(self, x, wkey, gy, ks, db_key=None, wrow0=0, rec=None):
        """Weight gradient (+ optional bias gradient) and, when the input carries a gradient,
        the data gradient.  gy: gradient w.r.t. the conv output (a View).  rec (dict): receives the emitted 2-D ops
        ("wgrad", "dgrad") for the split-storage passes of finalize()."""
        rec = rec if rec is not None else {}
        cin, cout = x.C, gy.C
        if x.nb is not None and ks == 3:                      # volume: see _conv_fwd
            assert isinstance(gy, _ScratchView) and gy.off and db_key is None and wrow0 == 0
            x, x_orig = self._win_of.get(wkey, x), x          # the weight gradient reads the depth window
            ws = self.L.uz_conv_bwd_weight_workspace(3 * cin, cout, x.N, x.H, x.W, 3)
            self.scratch["wgrad"] = max(self.scratch["wgrad"], ws)
            # (a depth-window call - 3 C view channels over a C-channel buffer - writes the Conv3d gradient layout itself:
            # uz_conv_bwd_weight's slab reduction does the [co][kd][ci] -> [co][ci][kd] permutation on the way out)
            # (slab reductions deferred to the table launch like the 2-D layers': the table row carries the window's C)
            nslab = 0
            if self._tables_ok() and self.knobs.wgrad_table and self.knobs.wgrad_table_vol \
                    and self._rev_ctx is None:
                nslab = self.L.uz_conv_bwd_weight_slabs(3 * cin, cout, x.N, x.H, x.W, 3)
            slabbuf = self.vec(wkey + ":wslabs", nslab * 9 * cout * 3 * cin) if nslab else None
            rec["wgrad"] = self._emit(self.bwd_ops, "UZ_OP_CONV_BWD_WEIGHT",
                       p=[("win", x), gy, self.G(wkey), None, ("scratch", "wgrad"), self.amax_in(x), self.amax_in(gy), None, slabbuf],
                       i=[3 * cin, x.Ctot, cout, gy.Ctot, x.N, x.H, x.W, 3, 0, 0, 0, 1 if nslab else 0, nslab], n=ws)      # nslab: slabs the buffer was sized for
            if nslab:
                self._wgrad_jobs.append((slabbuf, wkey, nslab, cout, 3 * cin, 9, cin))
            x = x_orig
            if x.buf.requires_grad:
                acc = self._claim(x)
                ws2 = self.L.uz_conv_workspace(cin, 3 * cout, x.N, x.H, x.W, 3)
                self.scratch["wgrad"] = max(self.scratch["wgrad"], ws2)
                packed = self._packed(wkey, cin, cout, x, True, vol=True)
                wp2 = self.P(wkey)
                if packed is None:
                    wp2 = self.vec(wkey + ":w3d_bwd", cout * cin * 27)
                    # the data gradient's weight layout is prepared in the FORWARD tape (same parameters: the optimiser only steps
                    # behind the backward tape), as a group of its own - not in the layer's backward chain
                    self._emit(self.fwd_ops, "UZ_OP_W3D_PERMUTE", p=[self.P(wkey), wp2], i=[cout, cin, 1], detached=True)
                rec["dgrad"] = self._emit(self.bwd_ops, "UZ_OP_CONV_BWD_DATA",
                           p=[("gywin", gy.zkey), wp2, self.gview(x), ("scratch", "wgrad"), self.amax_in(gy), ("amax", 0), packed],
                           i=[3 * cout, gy.Ctot, cin, x.Ctot, x.N, x.H, x.W, 3, acc], n=ws2)
            return
        wextra = wrow0 * cin * ks * ks
        ws = self.L.uz_conv_bwd_weight_workspace(cin, cout, x.N, x.H, x.W, ks)
        self.scratch["wgrad"] = max(self.scratch["wgrad"], ws)

        def emit_wgrad():
            # Slab reductions: outside data-parallel runs (where a bucket's gradients must be final when its all-reduce starts) a
            # 3 x 3 layer leaves its partial-sum slabs in a buffer of its own and ONE table-driven launch at the end of the tape adds
            # the slabs of every layer (UZ_OP_WGRAD_REDUCE_TABLE) - PHiSeg: 106 + 27 small reduction launches less per step
            nslab = 0
            if ks == 3 and db_key is None and wrow0 == 0 and self._tables_ok() and self.knobs.wgrad_table \
                    and self._rev_ctx is None:
                nslab = self.L.uz_conv_bwd_weight_slabs(cin, cout, x.N, x.H, x.W, ks)
            slabbuf = self.vec(wkey + ":wslabs", nslab * ks * ks * cout * cin) if nslab else None
            rec["wgrad"] = self._emit(self.bwd_ops, "UZ_OP_CONV_BWD_WEIGHT",
                                      p=[x, gy, self.G(wkey, wextra), self.G(db_key, wrow0) if db_key else None, ("scratch", "wgrad"),
                                         self.amax_in(x), self.amax_in(gy), None, slabbuf],
                                      i=[cin, x.Ctot, cout, gy.Ctot, x.N, x.H, x.W, ks, 0, 0, 0, 1 if nslab else 0, nslab], n=ws)      # nslab: slabs the buffer was sized for (checked at launch: ADVICE r5)
            if nslab:
                self._wgrad_jobs.append((slabbuf, wkey, nslab, cout, cin, ks * ks))
        # dy in a buffer of its own (small planes): the data gradient - the only thing the next layer's backward waits for -
        # goes first and the weight gradient becomes a scheduling group of its own, so that the latency-bound chains of the deep
        # levels (BatchNorm backward -> data gradient -> next BatchNorm backward) no longer carry the weight gradients and their
        # slab reductions; those fill the other dependency lane instead.
        decoupled = isinstance(gy, _ScratchView) and gy.view is not None
        if not decoupled:
            emit_wgrad()
        if x.buf.requires_grad:
            acc = self._claim(x)
            ws2 = self.L.uz_conv_workspace(cin, cout, x.N, x.H, x.W, ks)
            self.scratch["wgrad"] = max(self.scratch["wgrad"], ws2)
            packed = self._packed(wkey, cin, cout, x, True) if (ks == 3 and wrow0 == 0) else None
            # x is the output of a Conv -> ReLU unit (vanilla U-Net blocks) and this data gradient is the last writer of its
            # gradient: fold that unit's ReLU backward into the epilogue (mask, bias-gradient partials, bound) - the unit then
            # uses grad(x) in place as its dy instead of running uz_relu_bwd over it (conv_relu.bwd checks "last writer")
            fold = None
            st = (x.buf.relu or {}).get((x.c0, x.C)) if x.nb is None else None
            if st is not None and ks == 3 and wrow0 == 0 and self.knobs.fold_relu_bwd:
                npart = self.L.uz_conv_bwd_relu_partials(cin, cout, x.N, x.H, x.W, ks)
                if npart > 0:
                    fold = st["fold"] = dict(part=self.vec(x.buf.name + f":dbpart{x.c0}", 4 * cin * npart), npart=npart,
                                             amax=self.amax_out(self.gview(x)), claims=self._nclaims[x.buf])
            rec["dgrad"] = self._emit(self.bwd_ops, "UZ_OP_CONV_BWD_DATA",
                       p=[gy, self.P(wkey, wextra), self.gview(x), ("scratch", "wgrad"), self.amax_in(gy), ("amax", 0), packed]
                         + ([x, fold["part"], fold["amax"]] if fold else []),
                       i=[cout, gy.Ctot, cin, x.Ctot, x.N, x.H, x.W, ks, acc] + ([x.Ctot, 1] if fold else []), n=ws2)
        if decoupled:
            self._newgroup()
            emit_wgrad()

    def _packed(self, wkey, cin, cout, x, dgrad, vol=False):
        """Reference to the pre-packed split-fp16 weight image of this layer and direction, or None when the call packs its
        own (layers off the split path, extra tapes).  All images of a tape are packed by ONE launch at its head
        (uz_conv_pack_weights) instead of one small launch in front of every convolution."""
        # a Conv3d runs as a 2-D convolution whose contraction side has 3 C channels (the depth window): the image is packed
        # straight from the [Cout][Cin][3][3][3] parameter (no permutation pass)
        gcin, gcout = (cin, 3 * cout) if (vol and dgrad) else ((3 * cin, cout) if vol else (cin, cout))
        if not self.knobs.prepack or self.L.uz_conv_route(1 if dgrad else 0, gcin, gcout, x.N, x.H, x.W, 3) != 1:
            return None
        if not dgrad and self.target is not self.fwd_ops and self.target is not self.bwd_ops:
            return None                                        # extra (decode) tapes: the call packs its own image
        which = "bwd" if dgrad else "fwd"
        if which == "fwd" and self.target is self.bwd_ops and wkey not in self._packs["fwd"]:
            return None                                        # (a forward convolution that only exists in the backward tape)
        lst = self._packs[which]
        if wkey not in lst:
            lst[wkey] = dict(idx=len(lst), cin=cin, cout=cout, W=x.W, dgrad=int(dgrad), vol=int(vol),
                             mc=gcin if dgrad else gcout, kc=gcout if dgrad else gcin,
                             bytes=self.L.uz_conv_packed_bytes(gcin, gcout, x.W, int(dgrad)),
                             rows=self.L.uz_conv_pack_rows(gcin, gcout, x.W, int(dgrad)), cot=self.L.uz_conv_pack_cot(gcin, gcout, x.W, int(dgrad)))
        e = lst[wkey]
        assert (e["cin"], e["cout"], e["W"]) == (cin, cout, x.W), f"{wkey}: one weight, two convolution shapes"
        return ("packw", which, wkey)

    def _window_input(self, x, wkey):
        """The depth window of a 3x3x3 convolution addresses slices d-1, d, d+1 of its input as 3 C consecutive channels, which
        needs the view to span its buffer (C == Ctot).  A channel slice (one half of a reversible block's tensor, the image
        channels of the posterior's input) is first copied into a buffer of its own - pooled scratch inside reversible
        blocks, where the backward tape recomputes it together with everything else."""
        if x.C == x.Ctot:
            return x
        ctx = self._rev_ctx
        if ctx is not None:
            xc = self._pool((ctx, "win" + ("F" if ".f_block." in wkey else "G")), x.C, x.H, x.W)
            for b0 in (0, x.N + 1):                          # pooled scratch is shared between shapes: re-zero the depth padding
                self._emit(self.target, "UZ_OP_MEMSET", p=[View(xc.buf, 0, x.C, b0, 1)], n=4 * x.C * x.H * x.W)
        else:
            xc = self.vol(wkey + ":win", x.C, x.N, x.H, x.W, requires_grad=False)
        self.add_views(x, None, xc)
        self._win_of[wkey] = xc
        return xc

    def _decouple_wgrad(self, x, ks, name=""):
        """Weight gradient as a scheduling group of its own (needs dy in a real buffer instead of the lane scratch): on the
        latency-bound planes (decouple_wgrad_px) and in the sub-networks named by decouple_wgrad_prefixes - chains whose backward
        has no independent partner chain for the second lane, so the weight gradient of layer L runs beside BatchNorm backward +
        data gradient of layer L - 1 (PHiSeg's likelihood: +1 %; its posterior / prior nets: -0.5 ... -1 %, they already pair up)."""
        if x.nb is not None or ks != 3 or self.n_lanes <= 1:
            return False
        return x.N * x.H * x.W <= self.knobs.decouple_wgrad_px or any(name.startswith(q) for q in self.knobs.decouple_wgrad_prefixes)

    def _gy_scratch(self, like):
        self.scratch["gy"] = max(self.scratch["gy"], like.N * like.C * like.H * like.W)
        return ("gyview", like.C)

    def conv_bn_relu(self, x, cprefix, bprefix, out=None, name=None, relu=True, ybuf=None, save=None, a_grad=None):
        """Conv2D unit: Conv2d -> BatchNorm2d(eps=1e-3, momentum=0.01) -> ReLU (torchlayers.py:7-29).
        ybuf / save: caller-owned buffers for the pre-normalisation output and the saved statistics (reversible blocks share
        them); a_grad: view holding the gradient w.r.t. the unit's output instead of grad(a) (no copy)."""
        wkey, bkey = cprefix + ".weight", cprefix + ".bias"
        cout, ks = self.ptab.shape[wkey][0], self.ptab.shape[wkey][2]
        name = name or cprefix
        new = (lambda nm: self.vol(nm, cout, x.N, x.H, x.W)) if x.nb is not None else (lambda nm: self.buf(nm, cout, x.H, x.W))
        y = ybuf if ybuf is not None else new(name + ":y")
        a = out if out is not None else new(name + ":a")
        assert a.C == cout and a.H == x.H and a.W == x.W
        # (4 C floats: mean, rstd and - where the statistics come from the convolution's partials - alpha, beta' for a data gradient
        # that folds this unit's backward reduction, see _passes._split_storage_passes)
        save = save if save is not None else self.vec(name + ":bnsave", 4 * cout)
        # BatchNorm statistics in the convolution's epilogue (torchlayers.py:18-21: every Conv2d of a unit feeds a BatchNorm2d):
        # where the forward kernel supports it, it leaves per-tile {sum, sum of squares, max, max(-y)} partials and the
        # BatchNorm finalises them instead of streaming y a second time
        npart = 0
        # (not where the BatchNorm forward is ONE launch that forms the statistics from the channel's batch in registers anyway:
        #  the small path, and the mid path up to uz_bn_fwd_fused_limit)
        if self.bn_training and self.knobs.bn_fuse_stats and x.N * x.H * x.W > self.L.uz_bn_fwd_fused_limit(x.H, x.W) and \
                (x.nb is None or (ks == 3 and self.knobs.bn_fuse_stats_vol)):
            # (a volume's Conv3d is the 2-D kernel over its slices with the depth window as 3 Cin input channels: same epilogue)
            npart = self.L.uz_conv_bn_partials(x.C if x.nb is None else 3 * x.C, cout, x.N, x.H, x.W, ks)
        bnpart = self.vec(name + ":bnpart", 4 * cout * npart) if npart else None
        # Small planes (the 8x8 ... 2x2 levels: a unit is conv -> split-K reduce -> BatchNorm, 5 - 30 us each, on the step's critical
        # chains): the convolution stops after its main kernel and the one-workgroup-per-channel BatchNorm adds the slabs itself -
        # one launch and one pass over y less per unit, bit-identical values (include/uz_api.h: uz_conv_fwd_slabs)
        nslab = 0
        if x.nb is None and x.N * x.H * x.W <= 4096 and self.knobs.bn_fold_reduce:
            nslab = self.L.uz_conv_splitk_parts(x.C, cout, x.N, x.H, x.W, ks)
            nslab = nslab if nslab > 1 else 0
        self._conv_fwd(x, wkey, bkey, y, ks, 0, bn_partials=bnpart, slabs_only=nslab > 0)
        bnws = self.L.uz_bn_workspace(cout, x.N, x.H, x.W)
        self.scratch["bn"] = max(self.scratch["bn"], bnws)
        gam, bet = bprefix + ".weight", bprefix + ".bias"
        # unit record for the split-storage passes (finalize -> _passes._split_storage_passes); units inside reversible sequences (shared scratch,
        # recomputation inside the backward tape) and volume units stay as they are
        plain = ybuf is None and a_grad is None and x.nb is None and self._rev_ctx is None and self.target is self.fwd_ops
        unit = dict(name=name, y=y, a=a, save=save, relu=int(relu), npart=npart, C=cout, N=x.N, H=x.H, W=x.W) if plain else None
        if unit is not None:
            self._units.append(unit)
        op_fwd = self._emit(self.target, "UZ_OP_BN_RELU_FWD",
                   p=[y, self.P(gam), self.P(bet), self.B(bprefix + ".running_mean"), self.B(bprefix + ".running_var"),
                      save, a, ("scratch", "bn"), self.amax_out(a), bnpart,
                      ("scratch", "wgrad") if nslab else None, (self.P(bkey) if bkey else None) if nslab else None],
                   i=[cout, y.Ctot, a.Ctot, x.N, x.H, x.W, int(self.bn_training), int(relu), npart, nslab], f=[BN_EPS, BN_MOMENTUM])
        if unit is not None:
            unit["bn_fwd"] = op_fwd

        def bwd():
            if a_grad is None and not self._has_grad(a):
                return
            if not self.bn_training:
                raise RuntimeError("backward through eval-mode BatchNorm is not supported")
            gy = self._gy_scratch(y)
            gyv = _ScratchView(y.N, cout, y.H, y.W, amax=self._new_amax(bwd=True))
            if self._decouple_wgrad(x, ks, cprefix) and ybuf is None and a_grad is None:
                gyv.view = self.buf(name + ":dy", cout, y.H, y.W, N=y.N, requires_grad=False)
                gy = gyv
            if x.nb is not None and ks == 3:
                # volume: dy sits one slice into the scratch, between two zeroed border slices (the data gradient reads it
                # through a depth window)
                # ... in a scratch region of its own per (slices, slice size): the arena is zero-initialised and only the interior
                # slices are ever written, so the two border slices stay zero without a memset per layer and step
                sl = cout * y.H * y.W
                gyv.zkey = (y.N, sl)
                self._gyz[gyv.zkey] = (y.N + 2) * sl
                gy, gyv.off = ("gyvol", gyv.zkey), sl
            ga = a_grad if a_grad is not None else self.gview(a)
            # conv-bias gradient (the sum of dy: analytically zero behind a training-mode BatchNorm, the reference returns its
            # rounding noise and so do we): outside data-parallel runs the large-plane units leave their per-workgroup sums in rows of
            # their own and ONE table-driven launch at the end of the tape adds them - a summation launch less in every unit's chain
            dbrows = self.L.uz_bn_bwd_dbias_rows(x.N, x.H, x.W) if (plain and self._tables_ok() and self.knobs.dbias_table) else 0
            dbpart = self.vec(name + ":dbrows", 2 * dbrows * cout) if dbrows else None
            op_bwd = self._emit(self.bwd_ops, "UZ_OP_BN_RELU_BWD",
                                p=[ga, y, self.P(gam), self.P(bet), save, gy, self.G(gam), self.G(bet), dbpart if dbrows else self.G(bkey), ("scratch", "bn"),
                                   ("amax", gyv.amax, "acc")],
                                i=[ga.Ctot, cout, y.Ctot, cout, x.N, x.H, x.W, int(relu), 0, 0, 1 if dbrows else 0])
            if dbrows:
                self._dbias_jobs.append((dbpart, bkey, dbrows, cout, 1))
            rec = {}
            self._conv_bwd(x, wkey, gyv, ks, rec=rec)
            if x.nb is not None and ks == 3 and ybuf is None and a_grad is None and self._rev_ctx is None:
                # volume unit: its three backward ops share the zero-bordered dy scratch (see _passes._b16_pass)
                self._vol_units.append(dict(bn_bwd=op_bwd, gyv=gyv, wgrad=rec.get("wgrad"), dgrad=rec.get("dgrad")))
            if unit is not None:
                unit.update(bn_bwd=op_bwd, ga=ga, ks=ks, cin=x.C, wgrad=rec.get("wgrad"), dgrad=rec.get("dgrad"))
        self._push_bwd(bwd)
        return a

    # ------------------------------------------------------------------ reversible blocks
    def _pool(self, key, C, H, W, vec=False):
        """Scratch activations of the reversible blocks: one buffer per (branch, role, shape), re-used by every block that
        needs that role - nothing inside a reversible sequence is kept for the backward pass, it is recomputed."""
        pool, slots = self._rev_pool, self._rev_slots
        k = (key, C, H, W)
        if k not in pool:
            nm = "revpool:" + "/".join(map(str, k))
            D = self._vol_depth
            v = self.vec(nm, C) if vec else (self.vol(nm, C, D, H, W) if D else self.buf(nm, C, H, W))
            # all shapes of one (branch, role) share ONE region sized for the largest of them: a reversible sequence's scratch is
            # dead as soon as the next sequence of the branch starts (forward) or has been back-propagated (backward)
            # (pooled volumes therefore have no guaranteed zero border slices: _window_input clears those of the one kind of
            # pooled volume that is read through a depth window)
            slot = slots.setdefault(key[:2], {"floats": 0, "off": None})
            slot["floats"] = max(slot["floats"], v.buf.numel)
            v.buf.alias = slot
            pool[k] = v
        return pool[k]

    def add_views(self, a, b, y, alpha=1.0, accumulate=0, target=None):
        self._emit(target if target is not None else self.target, "UZ_OP_ADD_VIEWS",
                   p=[a, b, y, self.amax_in(a), self.amax_in(b) if b is not None else None,
                      self.amax_out(y) if (self.amax_in(a) is not None and (b is None or self.amax_in(b) is not None)) else None],
                   i=[a.Ctot, b.Ctot if b is not None else 0, y.Ctot, y.C, y.N, y.H, y.W, accumulate], f=[alpha])

    def rev_sequence(self, x, prefix, cout, depth, unit, out=None):
        """ReversibleSequence (torchlayers.py:55-82): an optional 1x1 Conv2D unit to `cout` channels (`inital_conv`), then
        `depth` additive-coupling blocks of revtorch (revtorch==0.2.0, requirements.txt:38, not vendored - restated from
        its published algorithm): split the channels into halves (x1, x2);
            y1 = x1 + F(x2),  y2 = x2 + G(y1),      F, G = Conv2D(c/2 -> c/2, 3x3) units (conv + BN + ReLU)
        and in the backward pass recompute the inputs from the outputs instead of storing them:
            x2 = y2 - G(y1),  x1 = y1 - F(x2),      then back-propagate through G and F on the recomputed tensors.
        The blocks' activations live in pooled scratch buffers (forward and backward share them); only the sequence's
        output is kept - that is the memory saving the reference advertises (README.md:4-5).  Like revtorch, the
        recomputation re-runs F and G in training mode, so their BatchNorm running statistics receive a second momentum
        update per step.  `unit(plan, x, prefix, **kw)` emits one Conv2D unit."""
        branch = prefix.split(".", 1)[0]
        N, H, W, h = x.N, x.H, x.W, cout // 2
        assert cout % 2 == 0
        self._vol_depth = x.N if x.nb is not None else None      # volumes: pooled scratch is volume-shaped (and keyed by depth below)
        if x.nb is not None:
            branch = (branch, x.N)
        seq_out = self.vol(prefix + ":revout", cout, x.N, H, W) if x.nb is not None else self.buf(prefix + ":revout", cout, H, W)
        widened = x.C != cout
        if widened:
            # the 1x1 unit's output is only the first block's input: it is recomputed in backward like every other block
            # input, so it lives in pooled scratch, and its gradient IS the dX the blocks form in the sequence's gradient buffer
            x = unit(self, x, prefix + ".inital_conv", out=self._pool((branch, "xin"), cout, H, W), a_grad=self.gview(seq_out))
        record = self._record_bwd
        blocks = []
        cur = x
        for i in range(depth):
            y = seq_out if i == depth - 1 else self._pool((branch, "x%d" % (i & 1)), cout, H, W)
            bp = f"{prefix}.sequence.reversible_blocks.{i}"
            self._rev_block(cur, y, bp, unit, h, branch, forward=True)
            blocks.append((cur, y, bp))
            cur = y
        if out is not None:                                  # consumer-owned slice of a concat buffer: strided copy
            self._newgroup()
            self.add_views(seq_out, None, out)

        def bwd():
            gsrc = seq_out
            if out is not None:
                if not self._has_grad(out):
                    return
                acc = self._claim(seq_out)
                self.add_views(self.gview(out), None, self.gview(seq_out), accumulate=acc, target=self.bwd_ops)
            if not self._has_grad(seq_out):
                return
            ycur = seq_out
            self._vol_depth = seq_out.N if seq_out.nb is not None else None
            for i in reversed(range(depth)):
                xin, _, bp = blocks[i]
                xrec = self._pool((branch, "x%d" % (i & 1)), cout, H, W)       # same ping-pong pair as the forward pass
                self._ginit.pop(xrec.buf, None)
                xrec.buf.gbuf = self.gview(seq_out).buf           # dX is formed in place in the sequence's gradient buffer
                self._ginit[xrec.buf] = [(0, cout)]
                self._rev_block(xrec, ycur, bp, unit, h, branch, forward=False)
                ycur = xrec
            if x.buf.requires_grad and not widened:
                acc = self._claim(x)
                self._newgroup()
                self.add_views(self.gview(seq_out), None, self.gview(x), accumulate=acc, target=self.bwd_ops)
        if record:
            self._push_bwd(bwd)
        return out if out is not None else seq_out

    def _rev_block(self, xv, yv, bp, unit, h, branch, forward):
        """One additive-coupling block.  forward=True: y from x (forward tape).  forward=False (inside the backward tape):
        x recomputed from y into `xv`, then the gradients of F, G and dX (in place in the shared gradient buffer)."""
        N, H, W = xv.N, xv.H, xv.W
        self._vol_depth = xv.N if xv.nb is not None else None
        self._rev_ctx = branch
        x1, x2, y1, y2 = xv.slice(0, h), xv.slice(h, h), yv.slice(0, h), yv.slice(h, h)
        bufs = {}
        for tag in ("F", "G"):
            ybuf, abuf = self._pool((branch, tag + "y"), h, H, W), self._pool((branch, tag + "a"), h, H, W)
            save = self._pool((branch, tag + "s"), 4 * h, 1, 1, vec=True)
            for b in (ybuf, abuf):
                self._ginit.pop(b.buf, None)
            bufs[tag] = (ybuf, abuf, save)
        if forward:
            rec, self._record_bwd = self._record_bwd, False      # nothing of the block is recorded: backward recomputes it
            tF = unit(self, x2, bp + ".f_block.0", out=bufs["F"][1], ybuf=bufs["F"][0], save=bufs["F"][2])
            self._newgroup()
            self.add_views(x1, tF, y1)
            tG = unit(self, y1, bp + ".g_block.0", out=bufs["G"][1], ybuf=bufs["G"][0], save=bufs["G"][2])
            self._newgroup()
            self.add_views(x2, tG, y2)
            self._record_bwd = rec
            self._rev_ctx = None
            return
        gy = self.gview(yv)
        gy1, gy2 = gy.slice(0, h), gy.slice(h, h)
        tgt, rec, saved_bwd = self.target, self._record_bwd, self._bwd
        self.target, self._record_bwd, self._bwd = self.bwd_ops, True, []
        try:
            # x2 = y2 - G(y1); gradients through G: dy1 += G'(dy2) (in place in the gradient buffer)
            self._newgroup()
            tG = unit(self, y1, bp + ".g_block.0", out=bufs["G"][1], ybuf=bufs["G"][0], save=bufs["G"][2], a_grad=gy2, recompute=True)
            self._newgroup()
            self.add_views(y2, tG, x2, alpha=-1.0)
            g_closures, self._bwd = self._bwd, []
            # x1 = y1 - F(x2); gradients through F: dx2 = dy2 + F'(dy1_total) (in place), dx1 = dy1_total (already there)
            self._newgroup()
            tF = unit(self, x2, bp + ".f_block.0", out=bufs["F"][1], ybuf=bufs["F"][0], save=bufs["F"][2], a_grad=gy1, recompute=True)
            self._newgroup()
            self.add_views(y1, tF, x1, alpha=-1.0)
            f_closures = self._bwd
            for fn in reversed(g_closures):
                self._newgroup()
                fn()
            for fn in reversed(f_closures):
                self._newgroup()
                fn()
        finally:
            self.target, self._record_bwd, self._bwd = tgt, rec, saved_bwd
            self._rev_ctx = None

    def conv_relu(self, x, prefix, out=None, name=None):
        """nn.Conv2d(3, pad 1) + nn.ReLU(inplace=True) of the vanilla U-Net blocks (unet.py:25-30)."""
        wkey, bkey = prefix + ".weight", prefix + ".bias"
        cout, _, ks, _ = self.ptab.shape[wkey]
        a = out if out is not None else self.buf((name or prefix) + ":a", cout, x.H, x.W)
        self._conv_fwd(x, wkey, bkey, a, ks, 1)
        self.scratch["bn"] = max(self.scratch["bn"], self.L.uz_bn_workspace(cout, x.N, x.H, x.W))
        if a.buf.relu is None:
            a.buf.relu = {}
        state = a.buf.relu[(a.c0, a.C)] = {}

        def bwd():
            if not self._has_grad(a):
                return
            fold = state.get("fold")
            if fold is not None:
                # the data gradient that wrote grad(a) last already applied this unit's ReLU mask (see _conv_bwd)
                if self._nclaims.get(a.buf, 0) != fold["claims"]:
                    raise RuntimeError(f"{prefix}: a later writer of grad({a.buf.name}) follows the data gradient that folded the ReLU "
                                       "backward - set UZ_FOLD_RELU_BWD=0 for this model")
                if not self._tables_ok() or not self.knobs.dbias_table:
                    self._emit(self.bwd_ops, "UZ_OP_CHAN_SUM_PARTIALS", p=[fold["part"], self.G(bkey)], i=[fold["npart"], cout, fold.get("dbl", 0)])
                else:
                    self._dbias_jobs.append((fold["part"], bkey, fold["npart"], cout, fold.get("dbl", 0)))
                self._conv_bwd(x, wkey, self.gview(a), ks)
                return
            gy = self._gy_scratch(a)
            gyv = _ScratchView(a.N, cout, a.H, a.W, amax=self._new_amax(bwd=True))
            self._emit(self.bwd_ops, "UZ_OP_RELU_BWD",
                       p=[self.gview(a), a, gy, self.G(bkey), ("scratch", "bn"), ("amax", gyv.amax, "acc")],
                       i=[a.Ctot, cout, a.Ctot, cout, x.N, x.H, x.W])
            self._conv_bwd(x, wkey, gyv, ks)
        self._push_bwd(bwd)
        return a

    def conv_bare(self, x, prefix, out=None, name=None, rows=None):
        """Plain nn.Conv2d (1x1 heads: phiseg.py:95-96,281-284; unet.py:122; probabilistic_unet.py:95).
        rows=(r0, n): use only output rows [r0, r0+n) of the parameter (mu / log-sigma halves)."""
        wkey, bkey = prefix + ".weight", prefix + ".bias"
        cout, ks = self.ptab.shape[wkey][0], self.ptab.shape[wkey][2]
        r0 = 0
        if rows is not None:
            r0, cout = rows
        y = out if out is not None else (self.vol((name or prefix) + ":y", cout, x.N, x.H, x.W) if x.nb is not None
                                         else self.buf((name or prefix) + ":y", cout, x.H, x.W))
        self._conv_fwd(x, wkey, bkey, y, ks, 0, wrow0=r0)

        def bwd():
            if not self._has_grad(y):
                return
            self._conv_bwd(x, wkey, self.gview(y), ks, db_key=bkey, wrow0=r0)
        self._push_bwd(bwd)
        return y

    # ------------------------------------------------------------------ resampling
    def _resample(self, fcode, bcode, x, y, extra_i=()):
        self._newgroup()
        pp = [x, y]
        if fcode in ("UZ_OP_AVGPOOL_FWD", "UZ_OP_BILINEAR_FWD"):
            # pooling and interpolation are convex combinations: the output inherits the input's magnitude bound
            xin = self.amax_in(x)
            pp += [xin, self.amax_out(y) if xin is not None else None]
        self._emit(self.target, fcode, p=pp, i=[x.C, x.Ctot, y.Ctot, x.N, x.H, x.W, *extra_i])

        def bwd():
            if not self._has_grad(y) or not x.buf.requires_grad:
                return
            acc = self._claim(x)
            # x is the output of a Conv -> ReLU unit and this pooling / interpolation backward is the last writer of its gradient
            # (the third unit of every vanilla U-Net block): fold that unit's ReLU backward in, like _conv_bwd does
            fold = None
            st = (x.buf.relu or {}).get((x.c0, x.C)) if x.nb is None else None
            if st is not None and bcode in ("UZ_OP_AVGPOOL_BWD", "UZ_OP_BILINEAR_BWD") and self.knobs.fold_relu_bwd:
                rows = self.L.uz_resample_bwd_relu_rows(0 if bcode == "UZ_OP_AVGPOOL_BWD" else 1, x.C, x.N, x.H, x.W)
                fold = st["fold"] = dict(part=self.vec(x.buf.name + f":dbpart{x.c0}", 2 * rows * x.C), npart=rows, dbl=1,
                                         amax=self.amax_out(self.gview(x)), claims=self._nclaims[x.buf])
            self._emit(self.bwd_ops, bcode, p=[self.gview(y), self.gview(x)] + ([x, fold["part"], fold["amax"]] if fold else []),
                       i=[x.C, y.Ctot, x.Ctot, x.N, x.H, x.W, *extra_i, acc] + ([x.Ctot] if fold else []))
        self._push_bwd(bwd)
        return y

    def avgpool(self, x, name):
        """nn.AvgPool2d(2, 2, ceil_mode=True) (phiseg.py:23, unet.py:22)."""
        y = self.buf(name, x.C, (x.H + 1) // 2, (x.W + 1) // 2, requires_grad=x.buf.requires_grad)
        return self._resample("UZ_OP_AVGPOOL_FWD", "UZ_OP_AVGPOOL_BWD", x, y)

    def bilinear(self, x, align_corners, name=None, out=None):
        y = out if out is not None else self.buf(name, x.C, 2 * x.H, 2 * x.W, requires_grad=x.buf.requires_grad)
        return self._resample("UZ_OP_BILINEAR_FWD", "UZ_OP_BILINEAR_BWD", x, y, (int(align_corners),))

    def nearest(self, x, factor, name):
        y = self.buf(name, x.C, x.H * factor, x.W * factor, requires_grad=x.buf.requires_grad)
        if factor == 1:
            pass
        return self._resample("UZ_OP_NEAREST_FWD", "UZ_OP_NEAREST_BWD", x, y, (factor,))

    def avgpool3d(self, x, name):
        """nn.AvgPool3d(2, 2, ceil_mode=True) (phiseg3D.py:101) on a volume."""
        D, H, W = x.N, x.H, x.W
        y = self.vol(name, x.C, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2, requires_grad=x.buf.requires_grad)
        self._newgroup()
        self._emit(self.target, "UZ_OP_AVGPOOL3D_FWD", p=[x, y], i=[x.C, x.Ctot, y.Ctot, D, H, W])
        if self.amax_in(x) is not None:                       # a mean of inputs: the input's bound holds (forwarded by a 1-op copy)
            self.add_views_bound(x, y)

        def bwd():
            if not self._has_grad(y) or not x.buf.requires_grad:
                return
            acc = self._claim(x)
            self._emit(self.bwd_ops, "UZ_OP_AVGPOOL3D_BWD", p=[self.gview(y), self.gview(x)], i=[x.C, y.Ctot, x.Ctot, D, H, W, acc])
        self._push_bwd(bwd)
        return y

    def add_views_bound(self, x, y):
        """Make y's magnitude-bound slot inherit x's (one lane of a tiny launch)."""
        self._emit(self.target, "UZ_OP_ABSMAX_COPY", p=[self.amax_in(x), self.amax_out(y)])

    def trilinear(self, x, name=None, out=None):
        """F.interpolate(mode='trilinear', scale_factor=2, align_corners=True) (phiseg3D.py:146,306,376): the 2-D bilinear kernel
        per slice, then linear interpolation along the depth (csrc/vol.hip) - the interpolation is separable."""
        D, H, W = x.N, x.H, x.W
        mid = self.vol((name or "tri") + ":inplane", x.C, D, 2 * H, 2 * W, requires_grad=x.buf.requires_grad)
        self.bilinear(x, True, out=mid)
        y = out if out is not None else self.vol(name, x.C, 2 * D, 2 * H, 2 * W, requires_grad=x.buf.requires_grad)
        self._newgroup()
        self._emit(self.target, "UZ_OP_DEPTH_LERP_FWD", p=[mid, y], i=[x.C, mid.Ctot, y.Ctot, D, 2 * H, 2 * W])
        if self.amax_in(mid) is not None:
            self.add_views_bound(mid, y)

        def bwd():
            if not self._has_grad(y) or not x.buf.requires_grad:
                return
            acc = self._claim(mid)
            self._emit(self.bwd_ops, "UZ_OP_DEPTH_LERP_BWD", p=[self.gview(y), self.gview(mid)], i=[x.C, y.Ctot, mid.Ctot, D, 2 * H, 2 * W, acc])
        self._push_bwd(bwd)
        return y

    def nearest3d(self, x, f, fz, name):
        y = self.vol(name, x.C, x.N * fz, x.H * f, x.W * f, requires_grad=x.buf.requires_grad)
        self._newgroup()
        self._emit(self.target, "UZ_OP_NEAREST3D_FWD", p=[x, y], i=[x.C, x.Ctot, y.Ctot, x.N, x.H, x.W, f, fz])

        def bwd():
            if not self._has_grad(y) or not x.buf.requires_grad:
                return
            acc = self._claim(x)
            self._emit(self.bwd_ops, "UZ_OP_NEAREST3D_BWD", p=[self.gview(y), self.gview(x)], i=[x.C, y.Ctot, x.Ctot, x.N, x.H, x.W, f, fz, acc])
        self._push_bwd(bwd)
        return y

    def spatial_mean(self, x, name):
        y = self.buf(name, x.C, 1, 1)
        self._newgroup()
        self._emit(self.target, "UZ_OP_SPATIAL_MEAN_FWD", p=[x, y], i=[x.C, x.Ctot, x.N, x.H, x.W])

        def bwd():
            if not self._has_grad(y):
                return
            acc = self._claim(x)
            self._emit(self.bwd_ops, "UZ_OP_SPATIAL_MEAN_BWD", p=[self.gview(y), self.gview(x)],
                       i=[x.C, x.Ctot, x.N, x.H, x.W, acc])
        self._push_bwd(bwd)
        return y

    def bcast_channels(self, z, out):
        """Fcomb tiling of z (N, L) over the spatial axes into channels of `out` (probabilistic_unet.py:190-197)."""
        L = z.C
        self._newgroup()
        self._emit(self.target, "UZ_OP_BCAST_CHANNELS", p=[z, out], i=[L, out.Ctot, out.N, out.H, out.W])
        if self._record_bwd:
            # another tape (decode: sample() / reconstruct()) may overwrite these channels between loss() and
            # backward(), which the reference allows; the backward tape therefore re-tiles z before it reads them
            self._bwd_head.append(lambda: self._emit(self.bwd_ops, "UZ_OP_BCAST_CHANNELS", p=[z, out],
                                                     i=[L, out.Ctot, out.N, out.H, out.W]))

        def bwd():
            if not self._has_grad(out) or not z.buf.requires_grad:
                return
            assert self._claim(z) == 0
            self._emit(self.bwd_ops, "UZ_OP_BCAST_CHANNELS_BWD", p=[self.gview(out), self.gview(z)],
                       i=[out.Ctot, L, out.N, out.H, out.W])
        self._push_bwd(bwd)

    # ------------------------------------------------------------------ inputs / latents / losses
    def posterior_input(self, patch, mask, nlabels, name):
        out = self.buf(name, patch.C + nlabels, patch.H, patch.W, requires_grad=False)
        self._newgroup()
        self._emit(self.target, "UZ_OP_POSTERIOR_INPUT", p=[patch, mask, out], i=[patch.C, nlabels, patch.N, patch.H, patch.W])
        return out

    def latent(self, mu, pre, eps, name, want_z=True, act=0):
        assert mu.contiguous and pre.contiguous
        new = (lambda nm: self.vol(nm, mu.C, mu.N, mu.H, mu.W)) if mu.nb is not None else (lambda nm: self.buf(nm, mu.C, mu.H, mu.W, N=mu.N))
        sigma = new(name + ":sigma")
        z = new(name + ":z") if want_z else None
        lat = Latent(mu, pre, sigma, z, eps, act)
        self._newgroup()
        self._emit(self.target, "UZ_OP_LATENT_FWD", p=[mu, pre, eps, sigma, z], i=[act], n=mu.numel)

        def bwd():
            dz = self.gview(z) if (z is not None and self._has_grad(z)) else None
            if dz is None and lat.kl_dmu is None:
                return
            assert self._claim(mu) == 0 and self._claim(pre) == 0
            self._emit(self.bwd_ops, "UZ_OP_LATENT_BWD",
                       p=[lat.kl_dmu, lat.kl_dsigma, dz, eps, sigma, self.gview(mu), self.gview(pre)], i=[act], n=mu.numel)
        self._push_bwd(bwd)
        return lat

    def latent_heads(self, h, mu_prefix, sigma_prefix, eps, name, want_z=True, act=0):
        """The tail of a SampleZBlock (phiseg.py:95-105): mu = mu_conv(h), pre = sigma_conv(h), sigma = softplus(pre), z = mu + sigma eps.
        On 2-D fp32 planes the three forward launches become ONE (h read once) and the six launches of the two heads' backward THREE
        (one data gradient that writes dh once, one weight-gradient pair that reads h once) - csrc/conv1x1_small.hip, bit-identical to the
        separate ops (UZ_FUSE_HEADS=0 keeps those).  Returns the Latent like latent()."""
        wm, bm, wsg, bsg = mu_prefix + ".weight", mu_prefix + ".bias", sigma_prefix + ".weight", sigma_prefix + ".bias"
        L, cin = self.ptab.shape[wm][0], h.C
        fuse = (self.knobs.fuse_heads and h.nb is None and self.ptab.shape[wm][2:] == (1, 1) and self.ptab.shape[wsg] == self.ptab.shape[wm]
                and len(self.ptab.shape[wm]) == 4 and bool(self.L.uz_latent_heads_ok(cin, L)))
        if not fuse:
            mu = self.conv_bare(h, mu_prefix)
            ps = self.conv_bare(h, sigma_prefix)
            return self.latent(mu, ps, eps, name, want_z=want_z, act=act)
        mu = self.buf(mu_prefix + ":y", L, h.H, h.W)
        pre = self.buf(sigma_prefix + ":y", L, h.H, h.W)
        sigma = self.buf(name + ":sigma", L, h.H, h.W)
        z = self.buf(name + ":z", L, h.H, h.W) if want_z else None
        lat = Latent(mu, pre, sigma, z, eps, act)
        self._newgroup()
        self._emit(self.target, "UZ_OP_LATENT_HEADS_FWD", p=[h, self.P(wm), self.P(bm), self.P(wsg), self.P(bsg), eps, mu, pre, sigma, z],
                   i=[cin, h.Ctot, L, h.N, h.H, h.W, act])

        def bwd():
            dz = self.gview(z) if (z is not None and self._has_grad(z)) else None
            if dz is None and lat.kl_dmu is None:
                return
            assert self._claim(mu) == 0 and self._claim(pre) == 0
            self._emit(self.bwd_ops, "UZ_OP_LATENT_BWD",
                       p=[lat.kl_dmu, lat.kl_dsigma, dz, eps, sigma, self.gview(mu), self.gview(pre)], i=[act], n=mu.numel)
            # head a = the sigma head: its separate backward ran first (reverse order of the forward), so its rows are added first.
            # The data gradient - what the unit below waits for - goes first; the weight gradients are a scheduling group of their own.
            if h.buf.requires_grad:
                acc = self._claim(h)
                self._emit(self.bwd_ops, "UZ_OP_LATENT_HEADS_BWD_DATA", p=[self.gview(pre), self.gview(mu), self.P(wsg), self.P(wm), self.gview(h)],
                           i=[L, cin, h.Ctot, h.N, h.H, h.W, acc])
            ws = self.L.uz_latent_heads_bwd_weight_workspace(cin, L, h.N, h.H, h.W)
            self.scratch["wgrad"] = max(self.scratch["wgrad"], ws)
            self._newgroup()
            self._emit(self.bwd_ops, "UZ_OP_LATENT_HEADS_BWD_WEIGHT",
                       p=[h, self.gview(pre), self.gview(mu), self.G(wsg), self.G(bsg), self.G(wm), self.G(bm), ("scratch", "wgrad")],
                       i=[cin, h.Ctot, L, h.N, h.H, h.W], n=ws)
        self._push_bwd(bwd)
        return lat

    def kl(self, q, p, weight, term):
        """weight * KL_two_gauss_with_diag_cov(q || p) (phiseg.py:436-479)."""
        n, per = q.mu.N, q.mu.C * q.mu.H * q.mu.W
        if q.mu.nb is not None:                                 # volume: ONE sample whose depth slices are stored as the batch
            n, per = 1, q.mu.N * per
        self._newgroup()
        self.scratch["bn"] = max(self.scratch["bn"], 512)
        self._emit(self.target, "UZ_OP_KL_FWD", p=[q.mu, q.sigma, p.mu, p.sigma, term, ("scratch", "bn")], i=[n, per], f=[weight])

        def bwd():
            for lat, tag in ((q, "q"), (p, "p")):
                lat.kl_dmu = self.buf(f"kl:{tag}:{lat.mu.buf.name}:dmu", lat.mu.C, lat.mu.H, lat.mu.W, requires_grad=False)
                lat.kl_dsigma = self.buf(f"kl:{tag}:{lat.mu.buf.name}:dsigma", lat.mu.C, lat.mu.H, lat.mu.W, requires_grad=False)
            self._emit(self.bwd_ops, "UZ_OP_KL_BWD",
                       p=[q.mu, q.sigma, p.mu, p.sigma, self.loss_scale, q.kl_dmu, q.kl_dsigma, p.kl_dmu, p.kl_dsigma],
                       i=[n, per], f=[weight])
        self._push_bwd(bwd)

    def residual_ce(self, s_list, mask, terms, post_scale=None):
        """residual_multinoulli_loss over the level logits (phiseg.py:481-513); terms: vec View of L floats.
        post_scale: extra factor on the terms (1/(H*W) turns the L=1 case into nn.CrossEntropyLoss() mean,
        unet.py:159-165)."""
        L, K = len(s_list), s_list[0].C
        assert all(s.contiguous for s in s_list)
        tab = self.ptr_table(list(s_list))
        ws = self.L.uz_ce_workspace(mask.N, mask.H, mask.W, L)
        self.scratch["ce"] = max(self.scratch["ce"], ws)
        self._newgroup()
        self._emit(self.target, "UZ_OP_CE_FWD", p=[tab, mask, terms, ("scratch", "ce")], i=[L, K, mask.N, mask.H, mask.W])
        if post_scale is not None:
            self._emit(self.target, "UZ_OP_SCALE", p=[terms], f=[post_scale], n=L)

        def bwd():
            for s in s_list:
                assert self._claim(s) == 0
            gtab = self.ptr_table([self.gview(s) for s in s_list])
            scale_ref = self.loss_scale
            if post_scale is not None:
                scale_ref = self.vec("ce_scale", 1)
                self._emit(self.bwd_ops, "UZ_OP_COPY", p=[scale_ref, self.loss_scale], n=4)
                self._emit(self.bwd_ops, "UZ_OP_SCALE", p=[scale_ref], f=[post_scale], n=1)
            self._emit(self.bwd_ops, "UZ_OP_CE_BWD", p=[tab, gtab, mask, scale_ref], i=[L, K, mask.N, mask.H, mask.W])
        self._push_bwd(bwd)

    def sum_terms(self, terms, n, total):
        self._newgroup()
        self._emit(self.target, "UZ_OP_SUM_TERMS", p=[terms, total], i=[n])

    def scale_(self, v, alpha, n):
        self._newgroup()
        self._emit(self.target, "UZ_OP_SCALE", p=[v], f=[alpha], n=n)

    def ptr_table(self, refs):
        self.ptr_tables.append(refs)
        return ("ptrtab", len(self.ptr_tables) - 1)

    # ------------------------------------------------------------------ the tape rewrites (_passes.py, _chain_plan.py) as seen from the plan
    def _all_tapes(self):
        return [("fwd", self.fwd_ops), ("loss", self.loss_ops), ("bwd", self.bwd_ops)] + list(self.extra_ops.items())

    def _users_of(self, v):
        return _passes._users_of(self, v)

    def _b16_slots(self, o):
        return _passes._b16_slots(self, o)

    def _b16_ok(self, o):
        return _passes._b16_ok(self, o)

    def _chain_tables(self, idx):
        return _chain_plan._chain_tables(self, idx)

    def chain_status(self, stream_ptr):
        return _chain_plan.chain_status(self, stream_ptr)

    # ------------------------------------------------------------------ finalisation
    def finalize(self, want_backward=True):
        assert not self.finalized
        self.loss_scale = self.vec("loss_scale", 1)
        if want_backward:
            for fn in self._bwd_head:
                self._newgroup()
                fn()
            for fn in reversed(self._bwd):
                self._newgroup()
                fn()
            if self._dbias_jobs:
                # all bias gradients of the folded ReLU backward in one launch (21 launches of ~7 us in U-Net's single chain)
                for part_jobs in self._by_bucket(self._dbias_jobs, lambda j: j[1]):
                    refs = [q for part, bkey, rows, c, dbl in part_jobs for q in (part, self.G(bkey), ("raw", rows), ("raw", c), ("raw", dbl))]
                    self._newgroup()
                    self._emit(self.bwd_ops, "UZ_OP_CHAN_SUM_TABLE",
                               p=[self.ptr_table(refs), ("gflat_keys", tuple(j[1] for j in part_jobs))],
                               i=[len(part_jobs), max(j[3] for j in part_jobs)])
                self._dbias_jobs = []
            jobs = self._wgrad_jobs
            if jobs:
                # One launch for ALL layers.  (UZ_WGRAD_TABLE_CHUNK = n: one launch per n layers in backward order, each a scheduling group
                # that is ready as soon as ITS layers' slabs are written - measured: 1 789 / 1 790 / 1 793 / 1 791 images/s for one table /
                # chunks of 16 / 8 / 32 layers, three alternations; with the chunks PRIORITISED in the lane scheduler - started the moment their layers are done - 1 820 -> 1 795 / 1 782 for chunks
                # of 16 / 8: they delay the critical chains.  The single launch behind the tape stays.)
                chunk = self.knobs.wgrad_table_chunk if self.knobs.wgrad_table_chunk > 0 else len(jobs)
                parts = self._by_bucket(jobs, lambda j: j[1]) if self.grad_buckets else [jobs[j0:j0 + chunk] for j0 in range(0, len(jobs), chunk)]
                for part in parts:
                    refs, blk = [], 0
                    for slabbuf, wkey, nslab, co, ci, kk, *vol in part:          # (vol: the C of a depth window's row, else absent)
                        refs += [slabbuf, self.G(wkey), ("raw", nslab), ("raw", co), ("raw", ci), ("raw", kk), ("raw", blk), ("raw", vol[0] if vol else 0)]
                        blk += self.L.uz_wgrad_reduce_blocks(ci, co, 3 if kk == 9 else 1)
                    self._newgroup()
                    self._emit(self.bwd_ops, "UZ_OP_WGRAD_REDUCE_TABLE",
                               p=[self.ptr_table(refs), ("gflat_keys", tuple(j[1] for j in part))], i=[len(part), blk])
                self._wgrad_jobs = []
            # the regulariser's gradients ADD to what the layers wrote (g += coeff w / |w|): behind the deferred table reductions, which
            # ASSIGN the bias / weight gradients they sum (round 4 until its last hours ran them in front - the table overwrote the
            # regulariser's share of every 3 x 3 weight gradient; tests/test_unet_probunet_gpu.py now compares the plans with and
            # without tables bit for bit)
            for fn in self._bwd_tail:
                self._newgroup()
                fn()
            # data parallel: one event per gradient bucket, recorded as soon as every writer of that slice of the flat
            # gradient buffer is done (the scheduler hoists the marker to that point of the DAG); the communication
            # stream waits for it and all-reduces the bucket beside the rest of the backward tape
            for b, (lo, hi) in enumerate(self.grad_buckets):
                self._newgroup()
                self._emit(self.bwd_ops, "UZ_OP_EVENT_RECORD", p=[("event", b), ("gflat_range", lo, hi)])
        self._bwd = []
        _passes._split_storage_passes(self)
        _passes._bn_offchain_pass(self)
        _passes._b16_pass(self)
        _chain_plan._chain_pass(self)
        # magnitude-bound slots: zero the forward-side slots and measure the parameter bound at the head of the forward tape,
        # zero the backward-side slots at the head of the backward tape (group 0 of each tape: everything else depends on it)
        self.n_amax_fwd = self.n_amax
        bwd_slots = sorted(self._amax_bwd)
        fwd_slots = [k for k in range(self.n_amax) if k not in set(bwd_slots)]
        # renumber so that forward slots are [0, nf) and backward slots [nf, n): one memset each
        remap = {k: i for i, k in enumerate(fwd_slots + bwd_slots)}
        self._amax_remap, self.n_amax_fwd = remap, len(fwd_slots)
        head = self._gid = -1
        pack_ops = {}
        for which, lst in self._packs.items():
            if not lst:
                continue
            off = rows = 0
            refs = []
            for wkey, e in lst.items():
                e["off"], e["row0"] = off, rows
                off += e["bytes"]
                rows += e["rows"]
                refs += [self.P(wkey), ("packw", which, wkey), ("raw", e["mc"]), ("raw", e["kc"]), ("raw", e["cin"]), ("raw", e["cot"]),
                         ("raw", e["dgrad"] | (e["vol"] << 1)), ("raw", e["row0"])]
            self._packbuf[which] = self.vec("packed_weights:" + which, off // 4)
            # a scheduling group of its own (gid head - 1) behind the bound measurement: only the layers that READ the packed images wait for
            # it - the first layers of both encoders (1 / 3 input channels: fp32 matrix path) start beside it (40 us off the forward's chain)
            pack_ops[which] = _ops.make("UZ_OP_PACK_WEIGHTS", p=[self.ptr_table(refs), ("amaxw", 0), self._packbuf[which]], i=[len(lst), rows],
                                        gid=head - 1 if self.knobs.pack_own_group else head)
        if "bwd" in pack_ops and self.bwd_ops:
            self.bwd_ops[:0] = [pack_ops["bwd"]]
        if self.fwd_ops:
            ops0 = []
            ops0.append(_ops.make("UZ_OP_MEMSET", p=[("amaxrange", 0, self.n_amax_fwd)], n=4 * _AMAX_FLOATS * self.n_amax_fwd, gid=head))
            ops0.append(_ops.make("UZ_OP_ABSMAX", p=[("pflat",), ("amaxw", 0)], n=self.ptab.n_params, gid=head))
            if "fwd" in pack_ops:
                ops0.append(pack_ops["fwd"])
            self.fwd_ops[:0] = ops0
        # Extra forward-only tapes (decode) run long after the forward tape that measured the parameter bound in slot 0 -
        # behind an optimiser step or a load_state_dict the bound may be stale, and a bound more than 4x too small overflows the
        # fp16 pieces.  A tape with a convolution on the split path therefore re-measures the bound at its own head.
        for name, ops in self.extra_ops.items():
            if any(o["code"] == "UZ_OP_CONV_FWD" and o.i("ks") == 3 and self.L.uz_conv_route(*conv_dims(o)) == 1 for o in ops):
                ops[:0] = [_ops.make("UZ_OP_MEMSET", p=[("amaxrange", 0, 1)], n=4 * _AMAX_FLOATS, gid=head),
                           _ops.make("UZ_OP_ABSMAX", p=[("pflat",), ("amaxw", 0)], n=self.ptab.n_params, gid=head)]
        if self.bwd_ops and bwd_slots:
            self.bwd_ops[:0] = [_ops.make("UZ_OP_MEMSET", p=[("amaxrange", self.n_amax_fwd, self.n_amax)],
                                          n=4 * _AMAX_FLOATS * (self.n_amax - self.n_amax_fwd), gid=head)]
        # arena layout
        off = 0
        for slot in self._rev_slots.values():
            slot["off"] = off
            off += -(-slot["floats"] // _ALIGN) * _ALIGN
        for b in self.bufs:
            if b.alias is not None:
                b.off = b.alias["off"]
                continue
            b.off = off
            off += -(-b.words // _ALIGN) * _ALIGN
        # scratch regions are private to a scheduling group, so every capture lane gets its own copy
        self.gy_off, self.scratch_off, self.gyz_off = [], [], []
        for _ in range(self.n_lanes):
            self.gy_off.append(off)
            off += -(-self.scratch["gy"] // _ALIGN) * _ALIGN
            zo = {}
            for key, fl in self._gyz.items():
                zo[key] = off
                off += -(-fl // _ALIGN) * _ALIGN
            self.gyz_off.append(zo)
            so = {}
            for k in ("bn", "wgrad", "ce"):
                so[k] = off
                off += -(-(self.scratch[k] // 4 + 1) // _ALIGN) * _ALIGN
            self.scratch_off.append(so)
        if self.grad_buckets and self.device.type == "cuda":
            for _ in self.grad_buckets:
                h = C.c_void_p()
                _ffi.check(self.L.uz_event_create(C.byref(h), 0), "event_create")
                self.events.append(h.value)
        self.amax_off = off
        off += self.n_amax * _AMAX_FLOATS
        self.arena_floats = off
        self.arena = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.base = self.arena.data_ptr()
        # pointer tables
        ntab = sum(len(t) for t in self.ptr_tables)
        self.ptrtab = torch.zeros(max(ntab, 1), dtype=torch.int64, device=self.device)
        vals, self._tab_off, k = [], [], 0
        for t in self.ptr_tables:
            self._tab_off.append(k)
            for r in t:
                vals.append(self._resolve(r))
                k += 1
        if vals:
            self.ptrtab.copy_(torch.tensor(vals, dtype=torch.int64))
        self.tapes, self.scheds, self._program_order = {}, {}, {}
        for nm, ops in (("fwd", self.fwd_ops), ("loss", self.loss_ops), ("bwd", self.bwd_ops), *self.extra_ops.items()):
            self._program_order[nm] = list(ops)              # the scheduler reorders `ops` in place; reschedule() starts from this order again
            self.scheds[nm] = self._schedule(ops)
            self.tapes[nm] = self._materialize(ops)
        self.loss_scale_t = self.tensor(self.loss_scale).view(1)
        self.loss_scale_t.fill_(1.0)
        self.finalized = True
        return self

    def reschedule(self, which):
        """Schedules tape `which` again from its program order - after the per-op durations (`o["cost_us"]`, Engine.tune_schedule)
        or the scheduler's settings changed - and rebuilds its op array.  Any schedule of the same DAG gives the same bits: ordered
        pairs stay ordered, and the only unordered writers of one location are the commuting magnitude-bound maxima."""
        ops = {"fwd": self.fwd_ops, "bwd": self.bwd_ops, "loss": self.loss_ops}.get(which)
        if ops is None:
            ops = self.extra_ops[which]
        ops[:] = self._program_order[which]
        self.scheds[which] = self._schedule(ops)
        self.tapes[which] = self._materialize(ops)

    def _resolve(self, r, lane=0):
        if r is None:
            return 0
        if isinstance(r, _ScratchView):
            if r.view is not None:
                return self._resolve(r.view, lane)
            if r.zkey is not None:
                return self.base + 4 * self.gyz_off[lane][r.zkey] + (2 if len(r.zkey) > 2 else 4) * r.off
            return self.base + 4 * (self.gy_off[lane] + r.off)
        if isinstance(r, View):
            assert r.buf.off is not None
            return self.base + 4 * r.buf.off + r.buf.esz * ((r.b0 * r.buf.C + r.c0) * r.buf.H * r.buf.W)
        kind = r[0]
        if kind == "param":
            return self.ptab.pflat.data_ptr() + 4 * (self.ptab.poff[r[1]] + r[2])
        if kind == "pgrad":
            return self.ptab.gflat.data_ptr() + 4 * (self.ptab.poff[r[1]] + r[2])
        if kind == "buffer":
            return self.ptab.bflat.data_ptr() + 4 * self.ptab.boff[r[1]]
        if kind == "pflat":
            return self.ptab.pflat.data_ptr()
        if kind in ("gflat", "gflat_keys"):
            return self.ptab.gflat.data_ptr()
        if kind == "scratch":
            return self.base + 4 * self.scratch_off[lane][r[1]]
        if kind == "gyview":
            return self.base + 4 * self.gy_off[lane]
        if kind == "ptrtab":
            return self.ptrtab.data_ptr() + 8 * self._tab_off[r[1]]
        if kind == "packw":
            return self.base + 4 * self._packbuf[r[1]].buf.off + self._packs[r[1]][r[2]]["off"]
        if kind == "raw":
            return int(r[1])
        if kind == "chaintab":
            return self._chain_tables(r[1])[r[2]].data_ptr()
        if kind == "chainimg":
            return self.base + 4 * self._chain_imgbuf[r[1]].buf.off + self._chain_imgs[r[1]][r[2]]["off"]
        if kind == "win":                                    # depth window of a volume: starts one slice before the view
            v = r[1]
            return self.base + 4 * v.buf.off + v.buf.esz * (((v.b0 - 1) * v.buf.C + v.c0) * v.buf.H * v.buf.W)
        if kind == "gywin":                                  # depth window of a volume unit's dy scratch (dy lives one slice into it)
            return self.base + 4 * self.gyz_off[lane][r[1]]
        if kind == "gyvol":                                  # dy of a volume unit: the real slices start one slice in
            return self.base + 4 * self.gyz_off[lane][r[1]] + (2 if len(r[1]) > 2 else 4) * r[1][1]
        if kind == "amax":
            return self.base + 4 * (self.amax_off + _AMAX_FLOATS * self._amax_remap[r[1]])
        if kind == "amaxw":
            return self.base + 4 * (self.amax_off + _AMAX_FLOATS * self._amax_remap[0])
        if kind == "amaxrange":
            return self.base + 4 * (self.amax_off + _AMAX_FLOATS * r[1])
        if kind == "event":
            return self.events[r[1]] if self.events else 0
        if kind == "gflat_range":
            return 0
        raise ValueError(r)

    def _materialize(self, ops):
        arr = (_ffi.uz_op * max(len(ops), 1))()
        for k, o in enumerate(ops):
            e = arr[k]
            e.code = self.codes[o["code"]]
            assert len(o["i"]) <= len(e.i) and len(o["f"]) <= len(e.f) and len(o["p"]) <= len(e.p), o["code"]
            for j, v in enumerate(o["i"]):
                e.i[j] = v
            for j, v in enumerate(o["f"]):
                e.f[j] = v
            e.n = o["n"]
            for j, r in enumerate(o["p"]):
                e.p[j] = self._resolve(r, o.get("lane", 0))
        return arr, len(ops)

    # ------------------------------------------------------------------ lane scheduling
    # Which p[] slots an op writes (every other slot is read) is part of its schema (_ops.writes).  Scratch slots are private to a
    # group and parameters are read-only inside a tape, so neither creates a dependency.
    _WRITES = _ops.WRITES          # the static part, by op code: an alias kept for callers that read Plan._WRITES; nothing is restated here

    def _access(self, o):
        """(reads, writes, accumulates) of op `o` as resource ranges.  Accumulates (bound slots only) commute with each other
        and conflict with reads and writes."""
        if o["code"] == "UZ_OP_CHAIN":
            reads, writes, accs = [], [], []
            for q in o["_acc_ops"]:
                r_, w_, a_ = self._access(q)
                reads.extend(r_); writes.extend(w_); accs.extend(a_)
            reads.extend(self._resources(("chainimg", o["_which"], None)))
            # (inside the launch the accumulators of a bound slot are ordered against its readers by the phases; towards the rest of the
            #  tape the launch both accumulates into and reads those slots: declare them written)
            writes.extend(accs)
            return reads, writes, []
        wr = _ops.writes(o)
        reads, writes, accs = [], [], []
        for j, r in enumerate(o["p"]):
            if j in wr:
                writes.extend(self._resources(r))
            elif isinstance(r, tuple) and len(r) == 3 and r[0] == "amax" and r[2] == "acc":
                accs.extend(self._resources(r))
            else:
                reads.extend(self._resources(r))
        return reads, writes, accs

    def _resources(self, r):
        """Dependency-relevant resources behind one pointer ref: (space, lo, hi) half-open ranges."""
        if isinstance(r, _ScratchView) and r.view is not None:
            return self._resources(r.view)
        if r is None or isinstance(r, _ScratchView):
            return []
        if isinstance(r, View):
            if r.buf.alias is not None:                  # pooled scratch: differently shaped Bufs overlap in memory -> whole-region hazards
                return [(("pool", id(r.buf.alias)), 0, 1 << 30)]
            return [(("buf", id(r.buf)), r.c0, r.c0 + r.C)]
        kind = r[0]
        if kind == "pgrad":
            lo = self.ptab.poff[r[1]]
            return [(("gflat",), lo, lo + _numel(self.ptab.shape[r[1]]))]
        if kind == "gflat":
            return [(("gflat",), 0, 1 << 62)]
        if kind == "gflat_keys":
            return [(("gflat",), self.ptab.poff[k], self.ptab.poff[k] + _numel(self.ptab.shape[k])) for k in r[1]]
        if kind == "buffer":
            return [(("bnbuf", r[1]), 0, 1)]
        if kind == "ptrtab":
            return [x for q in self.ptr_tables[r[1]] for x in self._resources(q)]
        if kind == "packw":
            return self._resources(self._packbuf[r[1]]) if r[1] in self._packbuf else [(("packw", r[1]), 0, 1)]      # (before finalize() lays the images out: _chain_plan._chain_pass)
        if kind == "chainimg":
            return self._resources(self._chain_imgbuf[r[1]]) if r[1] in self._chain_imgbuf else [(("chainimg", r[1]), 0, 1)]
        if kind == "chaintab":
            return []
        if kind == "win":
            return self._resources(r[1])
        if kind in ("gywin", "gyvol"):
            return []
        if kind == "amax":
            # Bound slots are atomic-max accumulated by the kernels that write the data they bound.  A slot has three access
            # classes (_access): the zeroing / parameter-bound measurement at the head of a tape WRITES it; producers ACCUMULATE
            # (refs tagged "acc": unordered among themselves - no false serialisation between the producers of one concat buffer);
            # consumers READ it - and a reader is ordered against EVERY accumulator of its slot, also one that writes channels the
            # reader never touches: a kernel derives its operand scale from the slot more than once (workgroup by workgroup, main
            # loop and epilogue), so the value must not move while it runs.
            return [(("amax",), r[1], r[1] + 1)]
        if kind == "amaxw":
            return [(("amax",), 0, 1)]
        if kind == "amaxrange":
            inv = {v: k for k, v in self._amax_remap.items()}
            return [(("amax",), inv[j], inv[j] + 1) for j in range(r[1], r[2])]
        if kind == "gflat_range":
            return [(("gflat",), r[1], r[2])]
        if kind == "event":
            return [(("event", r[1]), 0, 1)]
        if kind in ("param", "pflat", "scratch", "gyview", "raw"):
            return []
        raise ValueError(r)

    _op_cost = staticmethod(_sched._op_cost)
    _op_cost_beside = staticmethod(_sched._op_cost_beside)

    def _hazard_deps(self, ops):
        """Per op of `ops` (program order) the set of earlier ops it must follow."""
        return _sched.hazard_deps([self._access(o) for o in ops])

    def _schedule(self, ops):
        """Lane schedule of tape `ops` (_sched.schedule: REORDERS `ops` in place), under the switches the plan was built with."""
        sched, self.dag[id(ops)] = _sched.schedule(ops, self._access, self.n_lanes, self.sched_cost, self.knobs.sched_heavy)
        return sched

    # ------------------------------------------------------------------ execution helpers
    def tensor(self, v):
        """torch view (storage only) of a plan buffer slice, NCHW (volumes: the D real slices, i.e. DCHW)."""
        b = v.buf
        if b.b16:
            full = self.arena[b.off:b.off + b.words].view(torch.bfloat16)[:b.numel].view(b.N, b.C, b.H, b.W)
        else:
            full = self.arena[b.off:b.off + b.numel].view(b.N, b.C, b.H, b.W)
        if v.nb is not None:
            full = full[v.b0:v.b0 + v.nb]
        return full[:, v.c0:v.c0 + v.C]

    def span(self, views):
        """One flat tensor covering the given whole, consecutively allocated buffers (alignment gaps included), or None when
        they are not laid out that way: lets the host fill all of them (latent noise) with ONE launch."""
        bufs = [v.buf for v in views]
        if any(v.nb is not None or not v.contiguous or b.alias is not None for v, b in zip(views, bufs)):
            return None
        for a, b in zip(bufs, bufs[1:]):
            if not (a.off + a.numel <= b.off <= a.off + a.numel + _ALIGN):
                return None
        return self.arena[bufs[0].off:bufs[-1].off + bufs[-1].numel]

    def run(self, which, stream_ptr):
        arr, n = self.tapes[which]
        if n:
            _ffi.check(self.L.uz_run_tape(arr, n, C.c_void_p(stream_ptr)), f"tape '{which}'")

    def summary(self):
        cnt = {}
        for nm, ops in (("fwd", self.fwd_ops), ("loss", self.loss_ops), ("bwd", self.bwd_ops)):
            cnt[nm] = len(ops)
        cnt["arena_MB"] = self.arena_floats * 4 / 2 ** 20 if self.finalized else None
        return cnt


class _ScratchView:
    """Shape carrier for the shared dy scratch (gradient w.r.t. a conv output, consumed at once)."""
    def __init__(self, N, C, H, W, amax=None):
        self.N, self.C, self.H, self.W, self.Ctot = N, C, H, W, C
        self.buf = None
        self.amax = amax          # magnitude-bound slot of this unit's dy
        self.off = 0              # float offset inside the scratch (volumes: one slice, behind the zeroed border slice)
        self.nb = None
        self.view = None          # a buffer of its own instead of the lane's scratch (decoupled weight gradients, see _conv_bwd)
        self.zkey = None          # volume units: the zero-bordered scratch class (slices, floats per slice) this dy lives in


from . import _chain_plan, _passes      # noqa: E402  (down here: both import View, _ScratchView and _buf_of from this module)
