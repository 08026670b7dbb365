"""The engine's layered headers (csrc/spl_engine_*.h, the map at the top of spl_engine.hip) are real layers:
each one compiles as a main file of its own, so none relies on what its includer happened to include first.
No GPU: the compiler's front end only."""
import glob
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "splendor-gym_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"  # csrc/Makefile's default

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

HEADERS = sorted(os.path.basename(h) for h in glob.glob(os.path.join(CSRC, "spl_engine_*.h")))


@pytest.mark.parametrize("header", HEADERS)
def test_header_stands_alone(header):
    r = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-Wno-pragma-once-outside-header",
                        "-x", "hip", os.path.join(CSRC, header)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
