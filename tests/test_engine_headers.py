"""The engine's layered headers (csrc/spl_engine_*.h, the map at the top of spl_engine.hip) are real layers:
each one compiles as a main file of its own, so none relies on what its includer happened to include first,
and each includes only layers below it.  tools/microbench_deal.hip, which takes the deal layer alone, compiles too.
No GPU: the compiler's front end only."""
import glob
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "splendor-gym_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"  # csrc/Makefile's default

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

HEADERS = sorted(os.path.basename(h) for h in glob.glob(os.path.join(CSRC, "spl_engine_*.h")))
LAYER_INCLUDE = re.compile(r'^#include "(spl_engine_\w+\.h)"', re.M)


def syntax_only(path):
    return subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-Wno-pragma-once-outside-header",
                           "-x", "hip", path], capture_output=True, text=True, timeout=300)


@needs_hipcc
@pytest.mark.parametrize("header", HEADERS)
def test_header_stands_alone(header):
    r = syntax_only(os.path.join(CSRC, header))
    assert r.returncode == 0, r.stderr[-4000:]


@needs_hipcc
def test_microbench_deal_takes_the_deal_layer_alone():
    path = os.path.join(REPO, "tools", "microbench_deal.hip")
    engine = re.findall(r'^#include ".*(spl_engine[\w.]*)"', open(path).read(), re.M)
    assert engine == ["spl_engine_deal.h"], engine
    r = syntax_only(path)
    assert r.returncode == 0, r.stderr[-4000:]


def test_a_layer_includes_only_layers_below_it():
    order = LAYER_INCLUDE.findall(open(os.path.join(CSRC, "spl_engine.hip")).read())
    assert len(order) == len(set(order)), order
    assert sorted(order) == HEADERS, (order, HEADERS)  # every header in csrc/ is a layer of the engine
    for i, header in enumerate(order):
        for inc in LAYER_INCLUDE.findall(open(os.path.join(CSRC, header)).read()):
            assert inc in order[:i], f"{header} includes {inc}, which is not below it"
