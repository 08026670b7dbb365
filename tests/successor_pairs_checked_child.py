"""Child process of tests/test_gpu_search_pairs.py::test_checked_build: the pairs call on the BOUNDS-CHECK build of
the engine (SPLENDOR_AMD_LIB -> libsplendor_amd_checked.so) against the dense call on the same arena, once with
room for every pair and once overflowing; prints the recorded invariant violations as JSON.  Test infrastructure
only."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "splendor-gym_amd"), HERE, os.path.join(HERE, "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import successors_ref as sr  # noqa: E402
from splendor_gym import _native  # noqa: E402
from splendor_gym.device import Engine  # noqa: E402
from splendor_gym.search import pairs_reference, pick_pairs, pick_pairs_reference  # noqa: E402


def main():
    lib = _native.load_library()
    flags = ctypes.c_uint32()
    _native.check(lib, lib.spl_debug_bounds_flags(ctypes.byref(flags), 1))
    n = 65
    e = Engine(n, 2)
    e.reset(seeds=list(range(3100, 3100 + n)))
    sr.random_plies(e, 40, seed=13)
    s = e.successors(obs=False, obs_u8=True, mask_bits=True, winner=True)
    R = pairs_reference(s)
    m = int(R["base"][-1])
    pairs = e.successor_pairs(capacity=m, mask_bits=True, winner=True)
    assert pairs.total() == m
    for k in ("obs_u8", "flags", "reward", "pair", "mask_bits", "winner", "base"):
        assert getattr(pairs, k).cpu().numpy()[:len(R[k])].tobytes() == R[k].tobytes(), k
    value = torch.zeros(m, dtype=torch.float32, device=e.device)
    act = pick_pairs(pairs.legal, pairs.base, pairs.flags, pairs.reward, value, -1.0).cpu().numpy()
    want, _ = pick_pairs_reference(R["legal"], R["base"], R["flags"], R["reward"], np.zeros(m, np.float32), -1.0)
    assert act.tobytes() == want.tobytes()
    small = e.successor_pairs(capacity=m // 2)
    total = small.total()
    torch.cuda.synchronize()
    _native.check(lib, lib.spl_debug_bounds_flags(ctypes.byref(flags), 0))
    print(json.dumps({"pairs": m, "overflow_total": total, "flags": int(flags.value)}))


if __name__ == "__main__":
    main()
