"""Experiment builds of the engine library (not the product), selected at run time with
SPLENDOR_AMD_LIB.  build_variant() is the one Python entry point of csrc/Makefile's `variant` rule,
which every tool that builds a library goes through (ablate.py, stamps.py, wsstamps.py,
ablate_policy*.sh, ab_policy32.sh): the named subset of the sources is compiled with the product's
flags plus the extra -D flags, every other source is the product's own object from csrc/obj, and the
link line is the product's.  Ablated variants compute wrong outputs by design; only their timings mean
anything.

    python tools/variants.py build name[@REV]=-DFLAG[,-DFLAG2] ... [only=spl_engine[,spl_dual]] [lib=PATTERN]
    python tools/variants.py bench name ... [-- bench.py args]     (on the GPU box)
build: splendor-gym_amd/ablate/lib_<name>.so, or PATTERN with {name} filled in.  only= names the sources the
flags apply to (default: all).  @REV takes those sources from git revision REV (with REV's headers), the
others from the working tree; with no only=, all of today's sources must exist in REV.
"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "splendor-gym_amd", "csrc")
OUTD = os.path.join(REPO, "splendor-gym_amd", "ablate")


def sources_at(rev):
    """csrc/ as of git revision `rev`, exported beside its include/ to a temporary tree."""
    import tempfile
    d = tempfile.mkdtemp(prefix="spl_rev_")
    arc = subprocess.run(["git", "-C", REPO, "archive", rev, "splendor-gym_amd/csrc", "include"], check=True,
                         capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", d], input=arc, check=True)
    return os.path.join(d, "splendor-gym_amd", "csrc")


def _make(*args):
    return ["make", "-s", "-j4", "-C", CSRC, *args]


def build_variant(name, defs=(), only=(), rev=None, lib=None):
    """One `make variant`: returns the library's path (default ablate/lib_<name>.so)."""
    lib = os.path.abspath(lib) if lib else os.path.join(OUTD, f"lib_{name}.so")
    cmd = _make("variant", f"NAME={name}", "DEFS=" + " ".join(defs), f"LIB={lib}")
    if only:
        cmd.append("ONLY=" + " ".join(only))
    if rev:
        cmd.append("SRC=" + sources_at(rev))
    subprocess.run(cmd, check=True)
    return lib


def build_variants(jobs, workers=4):
    """jobs: keyword dicts for build_variant, built `workers` at a time.  The product's objects are made
    first, once: concurrent makes would race on csrc/obj."""
    from concurrent.futures import ThreadPoolExecutor
    subprocess.run(_make(*[os.path.join(CSRC, "obj", n + ".o") for n in source_names()]), check=True)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        for job, lib in zip(jobs, ex.map(lambda j: build_variant(**j), jobs)):
            print("built", job["name"], lib, flush=True)


def source_names():
    return subprocess.run(_make("names"), check=True, capture_output=True, text=True).stdout.split()


def build(specs):
    only = [s[5:].split(",") for s in specs if s.startswith("only=")]
    lib = [s[4:] for s in specs if s.startswith("lib=")]
    jobs = []
    for spec in specs:
        if spec.startswith(("only=", "lib=")):
            continue
        name, _, flags = spec.partition("=")
        name, _, rev = name.partition("@")
        jobs.append(dict(name=name, defs=[f for f in flags.split(",") if f], only=only[-1] if only else (),
                         rev=rev or None, lib=lib[-1].format(name=name) if lib else None))
    build_variants(jobs)


def bench(names, extra):
    for name in names:
        env = dict(os.environ, SPLENDOR_AMD_LIB=os.path.join(OUTD, f"lib_{name}.so"))
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--full", "--no-cpu-baseline", *extra], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(name, "FAILED", r.stderr[-2000:])
            raise SystemExit(1)
        import json
        d = json.loads(r.stdout.strip().splitlines()[-1])
        line = {"variant": name, "value": d["value"], "kernel_us": d["roofline"]["kernel_avg_us"],
                "frac": d["roofline"]["frac"]}
        for k in ("in_place_l3", "other_mode", "rollout_store"):
            if k in d:
                line[k + "_us"] = d[k]["roofline"]["kernel_avg_us"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "build":
        build(sys.argv[2:])
    else:
        args = sys.argv[2:]
        extra = args[args.index("--") + 1:] if "--" in args else []
        names = args[:args.index("--")] if "--" in args else args
        bench(names, extra)
