"""csrc/Makefile's `variant` rule, which every tool that builds an experiment library goes through
(tools/variants.py): the sources it knows are the sources there are, a variant compiles only the
subset it names, with the product's flags plus its own, and links the product's objects for the rest;
and what it builds loads.  No GPU: compiling and dlopen only."""
import os
import shlex
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "splendor-gym_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"  # csrc/Makefile's default

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

FLAG = "-DSPL_VARIANT_SELFTEST"


def make(*args):
    r = subprocess.run(["make", "-C", CSRC, *args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def names():
    return make("-s", "names").split()


def test_makefile_names_every_source():
    stems = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert sorted(names()) == stems


def test_variant_dry_run_compiles_the_subset_and_links_the_product(tmp_path):
    lib = str(tmp_path / "libselftest.so")
    out = make("-n", "variant", "NAME=selftest", "ONLY=spl_eval", f"DEFS={FLAG}", f"LIB={lib}")
    cmds = [shlex.split(line) for line in out.splitlines() if "hipcc" in line]
    obj_of = lambda c: os.path.realpath(c[c.index("-o") + 1])
    product_obj, variant_obj = os.path.join(CSRC, "obj"), os.path.join(REPO, "splendor-gym_amd", "ablate", "obj", "selftest")
    compiles = [c for c in cmds if "-c" in c]
    flagged = [c for c in compiles if FLAG in c]
    assert len(flagged) == 1, flagged
    (c,) = flagged
    assert os.path.realpath(c[-1]) == os.path.join(CSRC, "spl_eval.hip"), c
    assert obj_of(c) == os.path.join(variant_obj, "spl_eval.o"), c
    product_flags = make("-s", "flags-spl_eval").split()
    assert [a for a in c[1:] if a in product_flags] == product_flags, (c, product_flags)
    # whatever else is compiled (nothing, once the product is built) is a product object, without the flag
    for other in compiles:
        assert other is c or os.path.dirname(obj_of(other)) == product_obj, other
    links = [c for c in cmds if "-shared" in c]
    assert len(links) == 1 and obj_of(links[0]) == os.path.realpath(lib), links
    objs = [os.path.realpath(a) for a in links[0] if a.endswith(".o")]
    assert sorted(os.path.basename(o)[:-2] for o in objs) == sorted(names()), objs
    assert sorted(o for o in objs if os.path.dirname(o) != product_obj) == [os.path.join(variant_obj, "spl_eval.o")], objs
    assert [a for a in links[0][1:] if a in make("-s", "flags-spl_engine").split()] == make("-s", "flags-spl_engine").split()


def test_variant_library_loads(tmp_path):
    """The same variant built for real (spl_eval.hip compiles in seconds; the rest is the product's
    objects) exports every symbol the package binds."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "variants.py"), "build", f"selftest={FLAG}",
                        "only=spl_eval", f"lib={tmp_path}/lib{{name}}.so"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lib = tmp_path / "libselftest.so"
    assert lib.exists(), r.stdout
    code = ("import sys; sys.path.insert(0, %r); from splendor_gym import _native; lib = _native.load_library(); "
            "print(lib.spl_eval_abi_version(), lib.spl_abi_version())") % os.path.join(REPO, "splendor-gym_amd")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPLENDOR_AMD_LIB=str(lib)), capture_output=True,
                       text=True, timeout=300)  # dlopen only: no GPU needed
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.split() == ["1", "9"]
