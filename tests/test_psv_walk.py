"""Host-side policy of the window warp kernel's depth walk (v3d_psv_walk_chunks): how many 8-plane chunks a wave walks is a
function of the shape alone -- the longest walk that leaves 16 rounds of the 4 096 resident waves, evened out over the
segments.  The GPU tests of the walk (tests/test_psv_walk_gpu.py) run at shapes where this rule gives 1."""
import subprocess
import sys

from conftest import v3d


def test_walk_follows_the_shape():
    lib = v3d('_lib').load()
    walk = lib.v3d_psv_walk_chunks
    assert walk(64, 96, 56, 56) == 4          # cfg2 step: 64 x 12 x 392 waves = 4.6 x 16 rounds -> 3 segments of 4 chunks
    assert walk(8, 192, 120, 160) == 6        # cfg5 step: 8 x 24 x 2 400 waves = 7.0 x 16 rounds -> 7, evened out: 4 x 6
    assert walk(1, 192, 120, 160) == 1        # one cfg5 view: 14 rounds
    assert walk(2, 96, 56, 56) == 1           # a few views: one chunk per wave (the kernel without the walk)
    assert walk(64, 40, 56, 56) == 1          # 5 chunks: 1.9 x 16 rounds
    assert walk(1000, 40, 56, 56) == 5        # never more than the chunks there are
    assert walk(160, 40, 56, 56) == 3         # 5 chunks at a walk of 4 are 3 + 2, not 4 + 1
    assert walk(64, 96, 56, 56) == walk(64, 96, 56, 56)
    assert walk(0, 96, 56, 56) < 0 and walk(64, 0, 56, 56) < 0


def test_forced_walk_is_clamped_to_the_chunks():
    code = ("import importlib; L = importlib.import_module('3dvnet_amd._lib'); lib = L.load();"
            "L.set_option('psv_walk', 5); a = lib.v3d_psv_walk_chunks(2, 96, 56, 56);"
            "L.set_option('psv_walk', 50); b = lib.v3d_psv_walk_chunks(2, 96, 56, 56);"
            "L.set_option('psv_walk', 0); c = lib.v3d_psv_walk_chunks(2, 96, 56, 56); print(a, b, c)")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ['5', '12', '1']
