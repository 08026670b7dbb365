"""Child process of tests/test_gpu_successors.py::test_checked_build: one successor parity case on the
BOUNDS-CHECK build of the engine (SPLENDOR_AMD_LIB -> libsplendor_amd_checked.so); prints the recorded
invariant violations as JSON.  Test infrastructure only."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "splendor-gym_amd"), HERE, os.path.join(HERE, "golden")]

import torch  # noqa: E402

import successors_ref as sr  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from splendor_gym import _native  # noqa: E402
from splendor_gym.device import Engine  # noqa: E402


def main():
    lib = _native.load_library()
    flags = ctypes.c_uint32()
    _native.check(lib, lib.spl_debug_bounds_flags(ctypes.byref(flags), 1))
    n = 65
    e = Engine(n, 2)
    e.reset(seeds=list(range(3100, 3100 + n)))
    sr.random_plies(e, 40, seed=13)
    R = sr.oracle_pairs(Oracle(), e.download())
    got = sr.planes(e.successors(obs=True, obs_u8=True, mask_bits=True, winner=True, out=sr.prefilled(e)))
    sr.compare(got, R, "checked build")
    torch.cuda.synchronize()
    _native.check(lib, lib.spl_debug_bounds_flags(ctypes.byref(flags), 0))
    print(json.dumps({"pairs": int(R["flags"].size), "legal": int((R["flags"] & sr.LEGAL != 0).sum()),
                      "flags": int(flags.value)}))


if __name__ == "__main__":
    main()
