"""Every case of the BatchNorm dispatch table (tests/_bn_routes.py) takes the route it claims: uz_bn_route - the function the entry
points of csrc/bn.hip dispatch on - answers exactly the claimed path, instance, parts, nb, ngrp and float4 flag.  The cases sit on
both sides of every size limit, so a retune that moves one by a unit fails here and names the case; a GPU parity
test of the case would then no longer test the instance it was written for.  Also held here, without a GPU: the
ReLU-edge cap of every case (the share of gradient elements the reference zeroes stays within RELU_EDGE_SHARE)."""
import os

import pytest

from tests import _bn_routes as R

# UZ_BN_MID, UZ_BN_MID_FWD, UZ_BN_MID_HALF are read once per process and move the routes: the claims are those of the default build
SET = [s for s in R.SWITCHES if os.environ.get(s) is not None]
need_defaults = pytest.mark.skipif(bool(SET), reason=f"{', '.join(SET)} set: the table states the routes of the default dispatch")


@need_defaults
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_takes_the_route_it_claims(case):
    from unet_zoo_amd import _ffi
    got = R.queries(_ffi.lib(), case)
    assert got == case.claims, f"{R.case_id(case)}: claims {case.claims}, the dispatch answers {got}"


@need_defaults
@pytest.mark.parametrize("case", R.PARTIAL_CASES, ids=R.case_id)
def test_folded_inputs_take_the_large_path(case):
    """conv_partials (forward) and conv_partials + dbias_partials (backward) keep a call off the one-launch mid path."""
    from unet_zoo_amd import _ffi
    L = _ffi.lib()
    want = R.PARTIAL_CLAIMS[(case.N, case.H, case.W)]
    assert R.query(L, case, 0, R.F_CONV_PARTIALS) == want
    assert R.query(L, case, 1, R.F_CONV_PARTIALS | R.F_DBIAS_PARTIALS) == want
    assert R.query(L, case, 1, R.F_DBIAS_PARTIALS) == want
    rows = L.uz_bn_bwd_dbias_rows(case.N, case.H, case.W)
    # a mid-size plane reports no rows (its plain backward is one launch); beyond the limit one row per image and chunk
    assert rows == (0 if case.claims[1][1][0] == R.MID else case.N * want[2])


@need_defaults
def test_the_table_covers_every_route():
    ids = [R.case_id(c) for c in R.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    routes = {(k, r[0], r[1], r[5]) for c in R.CASES for k, r in c.claims}
    for d in ("fwd", "bwd"):
        assert {(d, R.SMALL, e, 0) for e in (2, 8, 16)} <= routes
        assert {(d, R.MID, nt, 1) for nt in (512, 1024)} <= routes
        assert {(d, R.LARGE, 0, v) for v in (0, 1)} <= routes and (d, R.LARGE_ST, 0, 1) in routes
    assert {r[2] for c in R.CASES for _, r in c.claims} == {1, 2}
    assert {r[3] for c in R.CASES for _, r in c.claims} >= {1, 2, 8}
    assert len(R.PARTIAL_CASES) == 3 and len(R.SLAB_CASES) == 3 and len(R.PACKED_CASES) == 2 and len(R.UNBIASED_CASES) == 3


def test_the_query_refuses_what_no_entry_point_accepts():
    import ctypes
    from unet_zoo_amd import _ffi
    L = _ffi.lib()
    out = (ctypes.c_int * 6)()
    assert L.uz_bn_route(0, 3, 3, 4, 2731, 1, 1, 0, out) == 0
    assert L.uz_bn_route(2, 3, 3, 4, 2731, 1, 1, 0, out) != 0            # direction
    assert L.uz_bn_route(0, 0, 3, 4, 2731, 1, 1, 0, out) != 0            # empty tensor
    assert L.uz_bn_route(0, 3, 3, 4, 2731, 1, 1, 32, out) != 0           # unknown flag bit
    assert L.uz_bn_route(0, 8, 3, 64, 64, 1, 1, R.F_B16, out) != 0       # bf16 storage at 32768 values per channel
    assert L.uz_bn_route(0, 3, 3, 145, 113, 1, 1, R.F_B16, out) != 0     # bf16 storage with H W % 4 != 0
    assert L.uz_bn_route(0, 3, 3, 4, 2731, 1, 1, 0, None) != 0


@pytest.mark.parametrize("case", [c for c in R.CASES if c.training], ids=R.case_id)
def test_relu_edge_share_stays_under_the_cap(case):
    share = R.reference(case, 1)["edge_share"]
    print(f"{R.case_id(case)}: {share:.2e} of the elements lie within {R.RELU_EDGE:g} of the ReLU edge")
    assert share <= R.RELU_EDGE_SHARE, f"{R.case_id(case)}: {share:.2e} of the gradient would be zeroed; give the case another seed offset"
