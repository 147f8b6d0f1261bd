"""Every case of the convolution dispatch table (tests/_conv_routes.py) takes the route it claims: the host-side queries
(uz_conv_route, uz_conv_split_parts, uz_conv_pack_cot, uz_conv_bn_partials, uz_conv_bwd_relu_partials,
uz_conv_bwd_weight_slabs) answer exactly the claimed values under the case's math mode.  The cases sit in pairs on both sides
of every routing threshold, so a retune that moves a threshold by one unit fails here and names the case it moved - the GPU
parity of tests/test_conv_routes_gpu.py is then no longer testing the instance the case was written for."""
import pytest

from tests import _conv_routes as R


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_takes_the_route_it_claims(case):
    from unet_zoo_amd import _ffi
    L = _ffi.lib()
    with R.dispatch_state(L, case.mode):
        got = R.queries(L, case)
    assert got == case.claims, f"{R.case_id(case)}: claims {case.claims}, the dispatch answers {got}"


def test_the_table_straddles_its_thresholds():
    """Each direction and math mode the GPU tier runs has cases on more than one route, and the table has no duplicates."""
    ids = [R.case_id(c) for c in R.CASES]
    assert len(ids) == len(set(ids))
    for d in R.DIRECTIONS:
        routes = {c.claims["route"] for c in R.CASES if c.direction == d and c.mode == 1}
        assert {0, 1} <= routes, (d, routes)
    assert {c.claims["route"] for c in R.CASES if c.mode == 0} == {0}
    assert all(c.claims["route"] == 1 for c in R.CASES if c.mode == 2 and c.ks == 3)
