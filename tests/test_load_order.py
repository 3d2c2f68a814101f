"""One HIP runtime per process, whichever is loaded first (CPU). build() loads libcnf_hip.so before
anything imported torch; torch's wheel may carry its own libamdhip64 / libhsa-runtime64, and with
the system copies mapped next to them the library's calls find no device. Needs a fresh process:
here torch is already loaded."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
from arl_conditional_normalizing_flows_amd import _lib
assert 'torch' not in sys.modules
_lib.load()
import torch
for stem in ('libamdhip64', 'libhsa-runtime64'):
    paths = sorted({l.split()[-1] for l in open('/proc/self/maps') if '/' + stem + '.so' in l})
    print(stem, paths)
    assert len(paths) == 1, paths
'''


def test_library_loaded_before_torch_shares_its_hip_runtime(lib):
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
