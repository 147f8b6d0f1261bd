"""The tape encoding against its record.  tests/golden/tape_dispatch.json was recorded before include/uz_ops.def existed, from the
hand-indexed run_one() and the hand-written Python schema: per raw uz_op the entry point csrc/tape.hip dispatches to and the slot
every argument comes from, the op codes, and the schema.  The table, run_one() and _ops.SCHEMA must keep saying the same thing -
a slot moved on one side only shows here, without a GPU (tests/_tape_dispatch.py: how the record is made and extended)."""
import functools
import json

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi, _ops
from tests import _tape_dispatch as T


@functools.lru_cache(None)
def _gold():
    with open(T.GOLDEN) as fh:
        return json.load(fh)


def test_run_one_makes_the_recorded_call_for_every_vector():
    records = _gold()["records"]
    got = T.replay([vec for vec, _ in records])
    assert len(records) > 600
    for (vec, want), have in zip(records, got):
        assert have == want, (vec, have, want)


def test_op_codes_equal_the_record():
    assert _ffi.op_codes() == _gold()["codes"]
    assert _ffi.op_codes()["UZ_OP_CONV_FWD"] == 1


def test_schema_parsed_from_the_table_equals_the_record():
    assert T.schema_dump(_ops.SCHEMA) == _gold()["schema"]
    assert _ops.B16_SLOT == 13


def test_every_op_of_the_table_has_a_base_record():
    """No new op without a record: some vector of its code sets exactly the ordinary i slots and every p slot of the op."""
    vectors = [vec for vec, _ in _gold()["records"]]
    for name, s in _ops.SCHEMA.items():
        code = _ffi.op_codes()[name]
        ordinary = [nm not in s.opts and nm != "b16" and not nm.startswith("rsv") for nm in s.i]
        assert any(v[0] == code and [x != 0 for x in v[1][:len(s.i)]] == ordinary and all(v[4][:len(s.p)]) for v in vectors), name
