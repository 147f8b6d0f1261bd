"""Every UZ_* environment variable the Python package reads: one row each, two readers.  (The C library's getenv tuning switches are
documented where they are read, under csrc/.)  A row's kind says what the variable accepts and what a reader returns: "flag" (0 | 1 ->
bool), "int", "float", a tuple (one of its strings, or what one of its types parses: the string), "list" (comma list -> tuple of the
non-empty items), "str" / "path" (as it is).  Anything else raises ValueError.  Scope "plan": the switch decides what a Plan contains and is
read ONCE per plan, by read(); the other scopes read through get() at the moment they need the value."""
import os
from collections import namedtuple

Knob = namedtuple("Knob", "name attr kind default scope doc")
TABLE = tuple(Knob(*row) for row in (
    ("UZ_LANES", "lanes", "int", 2, "plan", "dependency lanes of a replayed step; unset: the model decides (NativeModel.default_lanes*), a Plan clamps it to 1 ... 8"),
    ("UZ_SCHED_COST", "sched_cost", ("alone", "beside"), "alone", "plan", "the lane scheduler's cost model; unset: beside under the lane replay, alone under the graph replay"),
    ("UZ_SCHED_HEAVY", "sched_heavy", ("r4", "off", float), "r4", "plan", "which groups count as device-filling: r4, off or microseconds; unset: off under the lane replay, r4 under the graph replay"),
    ("UZ_DP_TABLES", "dp_tables", "flag", True, "plan", "data parallel: cut the deferred reduction tables per gradient bucket; 0 = a reduction launch per layer"),
    ("UZ_WGRAD_TABLE", "wgrad_table", "flag", True, "plan", "one table-driven launch adds the weight-gradient slabs of every layer"),
    ("UZ_WGRAD_TABLE_VOL", "wgrad_table_vol", "flag", True, "plan", "... of the volume path's layers too"),
    ("UZ_WGRAD_TABLE_CHUNK", "wgrad_table_chunk", "int", 0, "plan", "layers per weight-gradient table launch; 0 = one launch for all"),
    ("UZ_DBIAS_TABLE", "dbias_table", "flag", True, "plan", "one table-driven launch adds the bias-gradient rows of every unit"),
    ("UZ_FOLD_RELU_BWD", "fold_relu_bwd", "flag", True, "plan", "a Conv -> ReLU unit's ReLU backward in the epilogue of the last writer of its gradient"),
    ("UZ_PREPACK", "prepack", "flag", True, "plan", "one weight-packing launch at the head of a tape instead of one per convolution"),
    ("UZ_PACK_OWN_GROUP", "pack_own_group", "flag", True, "plan", "that launch as a scheduling group of its own: only its readers wait for it"),
    ("UZ_BN_FUSE_STATS", "bn_fuse_stats", "flag", True, "plan", "BatchNorm statistics from partials the convolution's epilogue leaves"),
    ("UZ_BN_FUSE_STATS_VOL", "bn_fuse_stats_vol", "flag", True, "plan", "... in the volume path's 3x3x3 units too"),
    ("UZ_BN_FOLD_REDUCE", "bn_fold_reduce", "flag", True, "plan", "small planes: BatchNorm forward adds the convolution's split-K slabs itself"),
    ("UZ_FUSE_HEADS", "fuse_heads", "flag", True, "plan", "the two 1x1 heads and the sampling tail of a SampleZBlock as one op per direction"),
    ("UZ_DECOUPLE_WGRAD", "decouple_wgrad_px", "int", 0, "plan", "planes (N*H*W) up to which a weight gradient is a scheduling group of its own; unset: NativeModel.decouple_wgrad_px"),
    ("UZ_DECOUPLE_PREFIX", "decouple_wgrad_prefixes", "list", (), "plan", "sub-networks decoupled at every size; set but empty: none; unset: NativeModel.decouple_wgrad_prefixes"),
    ("UZ_FOLD_BN_BWD", "fold_bn_bwd", "flag", False, "plan", "large planes: BatchNorm backward's reduction in the sole data gradient's epilogue (measured no gain)"),
    ("UZ_BN_FOLD_DGRAD", "bn_fold_dgrad", "flag", True, "plan", "small planes: BatchNorm backward adds the data gradient's split-K slabs itself"),
    ("UZ_PACK_DY", "pack_dy", "flag", True, "plan", "dY of large-plane units in split storage"),
    ("UZ_PACK_ACT", "pack_act", "flag", True, "plan", "activations read only by split-path convolutions in split storage"),
    ("UZ_BN_OFFCHAIN", "bn_offchain", "flag", False, "plan", "BatchNorm's apply pass off the forward chain (_passes._bn_offchain_pass; measured 1 % slower)"),
    ("UZ_STORE_B16", "store_b16", "flag", False, "plan", "with UZ_CONV_MATH=bf16: the volume path's large tensors in bf16 storage"),
    ("UZ_CHAIN", "chain_px", "int", 0, "plan", "planes (N*H*W) up to which small-plane ops run as phases of chain launches; 0 = off; unset: NativeModel.chain_px"),
    ("UZ_CHAIN_NETS", "chain_nets", "list", None, "plan", "diagnostics: build only these chains (fwd and sub-network names); unset: all"),
    ("UZ_CHAIN_BWD", "chain_bwd", "flag", True, "plan", "chains in the backward tape too"),
    ("UZ_CHAIN_WGS", "chain_wgs", "int", 256, "plan", "workgroups of the forward chain launch (nothing runs beside it)"),
    ("UZ_CHAIN_WGS_BWD", "chain_wgs_bwd", "int", 80, "plan", "workgroups of a backward chain (it runs beside the other lanes' kernels)"),
    ("UZ_REPLAY", "replay", ("lanes", "graph"), "lanes", "engine", "how enable_graphs() replays a tape: lanes (host-issued lane replay) or graph (hipGraph); read when NativeModel is defined"),
    ("UZ_DP_BUCKET_MB", "dp_bucket_mb", "float", 12.0, "dp", "size of the gradient slices of dp.param_buckets"),
    ("UZ_DP_BACKEND", "dp_backend", "str", None, "dp", "rccl | torch; unset: dp.GradSync follows the process group (nccl -> rccl, else torch), train_model.py takes rccl on a GPU"),
    ("UZ_DP_STREAM_PRIORITY", "dp_stream_priority", "int", 1, "dp", "priority of the communication stream"),
    ("UZ_TRAIN_REPLAY", "train_replay", "str", "1", "train", "anything but 0: train_model.py replays its steps on the engine's lanes"),
    ("UZ_TUNE_SCHEDULE", "tune_schedule", "int", 8, "train", "rounds of NativeModel.tune_schedule after the third step; 0 = keep the static schedule"),
    ("UZ_DATA_ROOT", "data_root", "path", None, "train", "sys_config.data_root where --data-root is not given"),
    ("UZ_PREPROC_FOLDER", "preproc_folder", "path", None, "train", "sys_config.preproc_folder where --preproc-folder is not given"),
    ("UZ_LOG_ROOT", "log_root", "path", None, "train", "sys_config.log_root where --log-root is not given"),
    ("UZ_LIB", "lib", "path", None, "lib", "path of the C-ABI library; unset: libuz_hip.so beside the package"),
))
_BY_NAME = {k.name: k for k in TABLE}
Snapshot = namedtuple("Snapshot", [k.attr for k in TABLE if k.scope == "plan"] + ["from_env"])


def _parse(k, raw):
    kind = k.kind
    try:
        if kind == "flag":
            return {"0": False, "1": True}[raw]
        if kind in ("int", "float"):
            return (int if kind == "int" else float)(raw)
        if isinstance(kind, tuple) and raw not in kind:
            next(t for t in kind if callable(t))(raw)                      # (StopIteration: a choice of strings only)
    except (KeyError, ValueError, StopIteration):
        accepts = " | ".join(getattr(t, "__name__", t) for t in kind) if isinstance(kind, tuple) else {"flag": "0 | 1"}.get(kind, kind)
        raise ValueError(f"{k.name}={raw!r}: expected {accepts}") from None
    return tuple(q for q in raw.split(",") if q) if kind == "list" else raw


def get(name, environ=os.environ):
    """The value of one variable now: parsed where it is set, else the row's default."""
    return _parse(_BY_NAME[name], environ[name]) if name in environ else _BY_NAME[name].default


def read(defaults=None, environ=os.environ):
    """Snapshot of the plan-scope switches, by attribute.  Precedence: the environment where the variable is set, else `defaults`
    (attribute -> value: the model's own), else the row's default.  from_env: the attributes the environment decided."""
    rows = [k for k in TABLE if k.scope == "plan"]
    env = {k.attr: _parse(k, environ[k.name]) for k in rows if k.name in environ}
    return Snapshot(**{**{k.attr: k.default for k in rows}, **(defaults or {}), **env}, from_env=frozenset(env))
