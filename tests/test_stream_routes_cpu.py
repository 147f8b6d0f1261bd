"""Every case of the streaming dispatch table (tests/_stream_routes.py) takes the kernel it claims: uz_stream_route,
uz_resample_bwd_relu_rows and uz_kl_fwd_parts - which decide through the same predicates as the entry points - answer exactly
the claimed values.  The cases sit on both sides of every threshold, so a retune that moves one by a unit fails here and names
the case; the GPU parity of tests/test_stream_routes_gpu.py is then no longer testing the instance the case was written for."""
import os
import subprocess
import sys

import pytest

from tests import _stream_routes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# UZ_BILINEAR_BWD_PAIR (read once per process) turns every float4-band answer into the pair kernel
PAIR = os.environ.get("UZ_BILINEAR_BWD_PAIR") is not None


def _expected(case):
    claims = dict(case.claims)
    if PAIR and case.op.startswith("bilinear_bwd") and claims["route"] == 2:
        claims["route"] = 1
    return claims


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_takes_the_route_it_claims(case):
    from unet_zoo_amd import _ffi
    got = R.queries(_ffi.lib(), case)
    assert got == _expected(case), f"{R.case_id(case)}: claims {_expected(case)}, the dispatch answers {got}"


@pytest.mark.parametrize("N,per,parts", R.KL_CASES)
def test_kl_case_takes_the_parts_it_claims(N, per, parts):
    from unet_zoo_amd import _ffi
    assert _ffi.lib().uz_kl_fwd_parts(N, per) == parts


def test_the_table_covers_every_route_of_every_op():
    ids = [R.case_id(c) for c in R.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    assert len(R.KL_CASES) == len(set(R.KL_CASES))
    for op, routes in R.OP_ROUTES.items():
        claimed = {c.claims["route"] for c in R.CASES if c.op.replace("_relu", "") == op}
        assert claimed == routes, (op, claimed)
    assert {p for _, _, p in R.KL_CASES} >= {1, 3, 64}


def test_the_query_honours_the_pair_switch():
    """With UZ_BILINEAR_BWD_PAIR set, a fresh process answers the pair kernel where this one answers the float4 band."""
    code = ("from unet_zoo_amd import _ffi; L = _ffi.lib(); "
            "print(L.uz_stream_route(3, 3, 2, 4, 32, 0, 16, 16, 16), L.uz_stream_route(3, 3, 2, 4, 16, 0, 16, 16, 16), L.uz_stream_route(3, 3, 2, 4, 32, 0, 4, 16, 16))")
    outs = []
    for pair in (None, "1"):
        env = dict(os.environ)
        env.pop("UZ_BILINEAR_BWD_PAIR", None)
        if pair:
            env["UZ_BILINEAR_BWD_PAIR"] = pair
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.split()[-3:])
    assert outs == [["2", "1", "0"], ["1", "1", "0"]], outs
