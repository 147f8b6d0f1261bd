"""Every case of the volume dispatch table (tests/_vol_routes.py) launches what it claims: uz_vol_route - which decides through the
same route functions as the entry points of csrc/vol.hip - answers exactly the claimed kernel and workgroups per plane.  The cases
sit on both sides of every threshold, so a retune that moves one by a unit fails here and names the case; the GPU parity of
tests/test_vol_routes_gpu.py is then no longer testing the instance the case was written for."""
import ctypes

import pytest

from tests import _vol_routes as R


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_takes_the_route_it_claims(case):
    from unet_zoo_amd import _ffi
    got = R.queries(_ffi.lib(), case)
    assert got == case.claims, f"{R.case_id(case)}: claims {case.claims}, the dispatch answers {got}"


@pytest.mark.parametrize("Cout,Cin,groups", R.PERMUTE_CASES)
def test_permute_case_takes_the_grid_it_claims(Cout, Cin, groups):
    from unet_zoo_amd import _ffi
    assert R.query(_ffi.lib(), 10, Cout, Cin, 1, 1, 1, 1, 16, 16) == (R.SCALAR, groups)


@pytest.mark.parametrize("n,groups", [c for c in R.CVT_CASES if c[0]])
def test_conversion_case_takes_the_grid_it_claims(n, groups):
    from unet_zoo_amd import _ffi
    assert R.query(_ffi.lib(), 11, n, 1, 1, 1, 1, 1, 16, 16) == (R.SCALAR, groups)


def test_the_table_covers_every_kernel_of_every_op():
    ids = [R.case_id(c) for c in R.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for op, (fk, bk) in R.OP_KERNELS.items():
        assert {c.claims["fwd"][0] for c in R.CASES if c.op == op} == fk, op
        assert {c.claims["bwd"][0] for c in R.CASES if c.op == op} == bk, op
    # each kernel with a capped grid has a case at the cap and a case beyond it (the claims say 64 either way: the plane sizes tell)
    for op in ("pool", "lerp"):
        for d in ("fwd", "bwd"):
            for k in (R.SCALAR, R.VEC):
                assert sum(1 for c in R.CASES if c.op == op and c.claims[d] == (k, 64)) >= 2, (op, d, k)
    assert any(c.claims["bwd"] == (R.WAVE, 65535) for c in R.CASES)


def test_the_query_refuses_what_no_entry_point_accepts():
    from unet_zoo_amd import _ffi
    L = _ffi.lib()
    out = (ctypes.c_int * 2)()
    assert L.uz_vol_route(0, 3, 4, 8, 8, 1, 1, 16, 16, out) == 0
    assert L.uz_vol_route(12, 3, 4, 8, 8, 1, 1, 16, 16, out) != 0          # op
    assert L.uz_vol_route(0, 3, 0, 8, 8, 1, 1, 16, 16, out) != 0           # empty tensor
    assert L.uz_vol_route(5, 3, 4, 8, 8, 0, 1, 16, 16, out) != 0           # factor
    assert L.uz_vol_route(0, 3, 4, 8, 8, 1, 1, 16, 16, None) != 0
    # the bf16-storage forms serve their float4 shapes only
    assert L.uz_vol_route(6, 3, 4, 8, 8, 1, 1, 16, 16, out) == 0 and tuple(out) == (R.ST, 1)
    assert L.uz_vol_route(6, 3, 4, 7, 8, 1, 1, 16, 16, out) != 0           # odd H
    assert L.uz_vol_route(7, 3, 4, 8, 6, 1, 1, 16, 16, out) != 0           # W % 4
    assert L.uz_vol_route(8, 3, 4, 5, 7, 1, 1, 16, 16, out) != 0           # H W % 4
    assert L.uz_vol_route(9, 3, 4, 4, 8, 1, 1, 16, 8, out) != 0            # alignment


def test_the_wave_gates_are_torchs_own_fp32_error():
    """NEAREST_WAVE_TORCH32, from which tests/test_vol_routes_gpu.py takes the wave kernel's gate, is what torch's fp32 CPU backward is
    away from fp64 on the GPU tier's operands - recomputed here, so a change of seed, shape or table cannot leave the gate stale."""
    assert {(c.f, c.fz) for c in R.WAVE_CASES} == set(R.NEAREST_WAVE_TORCH32) and len(R.WAVE_CASES) == len(R.NEAREST_WAVE_TORCH32)
    for c in R.WAVE_CASES:
        assert R.nearest_torch32_error(c) == pytest.approx(R.NEAREST_WAVE_TORCH32[(c.f, c.fz)], rel=1e-3), R.case_id(c)
    assert all(0 < v < 2.5e-6 for v in R.NEAREST_WAVE_TORCH32.values())          # each 4 x value stays under the old gate of ONE child
