"""Every case of the heads dispatch table (tests/_head_routes.py) launches what it claims: uz_heads_route - which decides through the
same predicates as the entry points of csrc/conv1x1_small.hip - answers exactly the claimed form, pixel workgroups, channel groups
and chunk count.  The cases sit on both sides of every threshold, so a retune that moves one by a unit fails here and names the
case; the GPU parity of tests/test_head_routes_gpu.py is then no longer testing the instance the case was written for.  Also: the
four convolution queries agree with the dispatch at ks = 1 for the output counts the streaming kernels do not instantiate."""
import ctypes
import os
import subprocess
import sys

import pytest

from tests import _conv_routes as CR
from tests import _head_routes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# UZ_HEADS_PAR=0 (read at every call) keeps the sequential forward everywhere
NO_PAR = os.environ.get("UZ_HEADS_PAR") is not None and int(os.environ["UZ_HEADS_PAR"]) == 0


def _expected(case):
    claims = dict(case.claims)
    if NO_PAR and claims.get("fwd", (0,))[0] == R.PAR:
        claims["fwd"] = (R.VEC, (case.H * case.W + 1023) // 1024)
    return claims


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_takes_the_route_it_claims(case):
    from unet_zoo_amd import _ffi
    got = R.queries(_ffi.lib(), case)
    assert got == _expected(case), f"{R.case_id(case)}: claims {_expected(case)}, the dispatch answers {got}"


def test_the_table_covers_every_form_of_every_op():
    ids = [R.case_id(c) for c in R.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for (kind, d), forms in R.FORMS.items():
        claimed = {c.claims[d][0] for c in R.CASES if c.kind == kind and d in c.claims}
        assert claimed == forms, (kind, d, claimed)
    assert {c.claims["wgrad"][0] for c in R.CASES if c.kind == "c1_b16" and "wgrad" in c.claims} == {R.VEC}
    # pixel workgroups 1 and 2, QPB 1, 4 and 64, one and several channel groups (ragged and not), chunk counts 1, 2, 16 and the cap
    assert {c.claims["fwd"][1] for c in R.CASES if "fwd" in c.claims and c.claims["fwd"][0] == R.PAR} == {1, 4, 64}
    assert {c.claims["fwd"][1] for c in R.CASES if "fwd" in c.claims and c.claims["fwd"][0] in (R.SCALAR, R.VEC)} == {1, 2}
    groups = {(c.claims["dgrad"][2], c.Cin % c.claims["dgrad"][3] != 0) for c in R.CASES if "dgrad" in c.claims and c.claims["dgrad"][0] != R.MFMA}
    assert {(1, False), (2, True), (4, True), (64, False)} <= groups, groups
    assert {c.claims["wgrad"][1] for c in R.CASES if "wgrad" in c.claims} >= {1, 2, 16, 64}


def test_the_query_refuses_what_no_entry_point_accepts():
    from unet_zoo_amd import _ffi
    L = _ffi.lib()
    out = (ctypes.c_int * 5)()
    assert L.uz_heads_route(3, 512, 4, 2, 4, 4, 1, out) == 0
    assert L.uz_heads_route(3, 513, 4, 2, 4, 4, 1, out) != 0           # latent heads: Cin
    assert L.uz_heads_route(4, 8, 0, 2, 4, 4, 1, out) != 0 and L.uz_heads_route(5, 8, 5, 2, 4, 4, 1, out) != 0      # L
    assert L.uz_heads_route(0, 8, 2, 0, 4, 4, 1, out) != 0             # empty tensor
    assert L.uz_heads_route(6, 8, 2, 2, 4, 4, 1, out) != 0             # op
    assert L.uz_heads_route(0, 8, 2, 2, 4, 4, 1, None) != 0
    for kind, N, Cin, L_, H, W in R.REFUSED:
        if kind == "lat":
            assert L.uz_latent_heads_ok(Cin, L_) == 0 and L.uz_heads_route(3, Cin, L_, N, H, W, 1, out) != 0


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_the_convolution_queries_agree_with_the_heads_dispatch_at_ks_1(mode):
    """uz_conv_route, uz_conv_bwd_weight_slabs, uz_conv_splitk_parts and uz_conv_bwd_splitk_parts answer 'streaming' exactly where
    uz_heads_route says the streaming kernels run: 5 and 7 outputs take the MFMA kernels, as 9 outputs and 513 channels do."""
    from unet_zoo_amd import _ffi
    L = _ffi.lib()
    out = (ctypes.c_int * 5)()
    with CR.dispatch_state(L, mode):
        for Cin, Cout, N, H, W in R.CONV_QUERY_STREAMING:
            for op in range(3):
                assert L.uz_heads_route(op, Cin, Cout, N, H, W, 1, out) == 0 and out[0] == R.VEC
            assert [L.uz_conv_route(k, Cin, Cout, N, H, W, 1) for k in range(3)] == [2, 2, 2]
            assert L.uz_conv_bwd_weight_slabs(Cin, Cout, N, H, W, 1) == 0
            assert L.uz_conv_splitk_parts(Cin, Cout, N, H, W, 1) == 1 and L.uz_conv_bwd_splitk_parts(Cin, Cout, N, H, W, 1) == 1
        for (Cin, Cout, N, H, W), want in R.CONV_QUERY_MFMA:
            for op in range(3):
                assert L.uz_heads_route(op, Cin, Cout, N, H, W, 1, out) == 0 and out[0] == R.MFMA
            got = dict(routes=tuple(L.uz_conv_route(k, Cin, Cout, N, H, W, 1) for k in range(3)), slabs=L.uz_conv_bwd_weight_slabs(Cin, Cout, N, H, W, 1),
                       parts=L.uz_conv_splitk_parts(Cin, Cout, N, H, W, 1), bwd_parts=L.uz_conv_bwd_splitk_parts(Cin, Cout, N, H, W, 1))
            assert got == want, (Cin, Cout, got, want)


def test_the_query_honours_the_heads_par_switch():
    """With UZ_HEADS_PAR=0 a fresh process answers the sequential float4 forward where this table claims the channel-parallel one."""
    code = ("import ctypes; from unet_zoo_amd import _ffi; L = _ffi.lib(); o = (ctypes.c_int * 5)(); "
            "assert L.uz_heads_route(3, 24, 2, 2, 16, 16, 1, o) == 0; print(o[0], o[1])")
    outs = []
    for par in (None, "1", "0"):
        env = dict(os.environ)
        env.pop("UZ_HEADS_PAR", None)
        if par:
            env["UZ_HEADS_PAR"] = par
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.split()[-2:])
    assert outs == [["2", "64"], ["2", "64"], ["1", "1"]], outs
