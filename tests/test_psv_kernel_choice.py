"""Which warp kernel the plane-sweep variance runs (v3d_psv_kernel_choice: 0 window, 1 reuse, 2 gather) -- the one statement the
library dispatches on and `MVSNet.cost_volume_depth` asks before it requests the channel-last fp32 volume, which only the window
kernel writes.  The window kernel's tap words keep their sign bit as a flag, so the size that counts is that of the BORDERED
channel-last copy, (n_img (Hf + 2) (Wf + 2) + 2 (Wf + 2) + 16) C floats, not of the feature stack."""
import os
import subprocess
import sys

from conftest import v3d

WINDOW, REUSE, GATHER = 0, 1, 2


def test_choice_follows_channels_and_the_bordered_size():
    choice = v3d('_lib').load().v3d_psv_kernel_choice
    assert choice(3299, 32, 60, 80) == WINDOW      # bordered copy 2 146 853 888 B, just under 2^31
    assert choice(3300, 32, 60, 80) == REUSE       # 2 147 504 640 B
    assert choice(3400, 32, 60, 80) == REUSE       # the raw stack, 2 088 960 000 B, is still below 2^31
    assert choice(8, 16, 60, 80) == GATHER
    assert choice(8, 24, 60, 80) < 0 and choice(0, 32, 60, 80) < 0


def test_developer_option_forces_the_fallback_kernels():
    code = ("import importlib; L = importlib.import_module('3dvnet_amd._lib'); lib = L.load(); out = [];\n"
            "for k in (1, 2, 0):\n"
            "    L.set_option('psv_kernel', k); out.append(lib.v3d_psv_kernel_choice(8, 32, 60, 80))\n"
            "print(*out)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ['1', '2', '0']
