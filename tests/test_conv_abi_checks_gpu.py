"""Two child-process checks of the convolution C ABI against fp64 references, on shapes no other test drives through it:
tools/wgrad_forms_check.py - the split-path weight gradient (conv_wgrad_split.hip) with fp32 and split-storage operands on ragged channel
counts, a partial last tile row and a 16-wide plane, against autograd's weight gradient (reference: torchlayers.py:18, nn.Conv2d);
tools/conv_free_check.py - forward and data gradient of the split-K 2 x 2 ... 8 x 8 planes (conv_mfma.hip)."""
import os, subprocess, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_weight_gradient_abi_vs_fp64():
    e = dict(os.environ)
    if e.get("UZ_CONV_MATH", "") in ("f32", "0", "bf16", "3"):
        pytest.skip("the split-fp16 weight gradient is not in play in this arithmetic mode")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "wgrad_forms_check.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ALL OK" in r.stdout, r.stdout[-2000:]


def test_small_plane_convolution_abi_vs_fp64():
    """Forward and data gradient of the 2 x 2 ... 8 x 8 planes, ragged channels, channel-slice views, accumulate."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "conv_free_check.py")], env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
