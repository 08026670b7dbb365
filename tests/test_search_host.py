"""The one-ply search without a GPU (include/splendor_search.h): the ABI constant and the ctypes mirrors against
the header, spl_successors and spl_search_pick refusing bad arguments on the host before any device work, and
pick_reference, the numpy oracle of the pick kernel, on written-out cases."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000  # a plausible, aligned, never-dereferenced device address: every case below is refused first
L, T = 0x01, 0x02  # SPL_SUCC_LEGAL, SPL_SUCC_TERMINATED
NAN, INF = np.float32("nan"), np.float32("inf")


def _lib():
    from splendor_gym import _native
    return _native, _native.load_library()  # dlopen only: no GPU needed


def _refused(lib, code, word):
    assert code == -1, code  # SPL_E_ARG
    msg = lib.spl_last_error()
    assert msg and word.encode() in msg, msg


def test_abi_constant_and_struct_sizes():
    native, lib = _lib()
    src = open(os.path.join(REPO, "include", "splendor_search.h")).read()
    assert re.search(r"#define SPL_SEARCH_ABI 1\b", src)
    assert lib.spl_search_abi_version() == native.SEARCH_ABI == 1
    for name, val in (("LEGAL", 0x01), ("TERMINATED", 0x02), ("TURN_LIMIT", 0x04), ("DREW", 0x08)):
        assert re.search(r"#define SPL_SUCC_%s 0x%02x\b" % (name, val), src), name
        assert getattr(native, "SUCC_" + name) == val
    assert lib.spl_abi_version() == 9  # the engine's own ABI did not move
    assert ctypes.sizeof(native.SuccArgs) == 6 * 8
    assert ctypes.sizeof(native.PickArgs) == 5 * 8 + 2 * 4
    assert native.PickArgs.sign.offset == 40
    for cls, tname in ((native.SuccArgs, "spl_succ_args_t"), (native.PickArgs, "spl_pick_args_t")):
        body = re.search(r"typedef struct \{([^{]*?)\} " + tname + ";", src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            names += [re.sub(r"[\s*]", "", part).split(" ")[-1] for part in
                      re.sub(r"^\s*(?:const\s+)?[a-z0-9_]+\s", "", decl.strip()).split(",") if part.strip()]
        assert names == [f[0] for f in cls._fields_], (tname, names)


def test_successors_refusals():
    native, lib = _lib()
    full = dict(obs_u8=P, obs=P, flags=P, reward=P, mask_bits=P, winner=P)
    args = lambda **kw: ctypes.byref(native.SuccArgs(**kw))
    ctx = ctypes.c_void_p(P)  # never dereferenced before the refusals below
    arena = native.ArenaDesc(P, lib.spl_arena_bytes(10, 2), 10, 2, 0, 0)
    _refused(lib, lib.spl_successors(None, ctypes.byref(arena), args(**full), None), "null context")
    _refused(lib, lib.spl_successors(ctx, None, args(**full), None), "null arena")
    _refused(lib, lib.spl_successors(ctx, ctypes.byref(native.ArenaDesc(None, 0, 10, 2, 0, 0)), args(**full), None),
             "null arena")
    _refused(lib, lib.spl_successors(ctx, ctypes.byref(native.ArenaDesc(P, 16, 10, 2, 0, 0)), args(**full), None),
             "too small")
    _refused(lib, lib.spl_successors(ctx, ctypes.byref(arena), None, None), "null")
    _refused(lib, lib.spl_successors(ctx, ctypes.byref(arena), args(**{**full, "obs": None, "obs_u8": None}), None),
             "at least one")
    for name in ("flags", "reward"):
        _refused(lib, lib.spl_successors(ctx, ctypes.byref(arena), args(**{**full, name: None}), None), "null")
    for name in ("obs", "obs_u8"):
        _refused(lib, lib.spl_successors(ctx, ctypes.byref(arena), args(**{**full, name: P + 8}), None), "aligned")
    _refused(lib, lib.spl_successors(ctx, ctypes.byref(arena), args(**{**full, "reward": P + 2}), None), "aligned")
    _refused(lib, lib.spl_successors(ctx, ctypes.byref(arena), args(**{**full, "mask_bits": P + 4}), None), "aligned")


def test_pick_refusals():
    native, lib = _lib()
    full = dict(flags=P, reward=P, value=P, action=P, best_q=P, sign=-1.0)
    args = lambda **kw: ctypes.byref(native.PickArgs(**kw))
    _refused(lib, lib.spl_search_pick(4, None, None), "null")
    for n in (0, -1):
        _refused(lib, lib.spl_search_pick(n, args(**full), None), "positive")
    for name in ("flags", "reward", "value", "action"):
        _refused(lib, lib.spl_search_pick(4, args(**{**full, name: None}), None), "null")
    for name in ("reward", "value", "action", "best_q"):
        _refused(lib, lib.spl_search_pick(4, args(**{**full, name: P + 2}), None), "aligned")


def _planes(cols):
    """[45, n] planes from per-table dicts {a: (flags, reward, value)}; every other pair is illegal."""
    n = len(cols)
    flags, reward, value = np.zeros((45, n), np.uint8), np.zeros((45, n), np.float32), np.zeros((45, n), np.float32)
    for t, col in enumerate(cols):
        for a, (f, r, v) in col.items():
            flags[a, t], reward[a, t], value[a, t] = f, r, v
    return flags, reward, value


def test_pick_reference_written_out_cases():
    from splendor_gym.search import pick_reference
    cols = [
        {3: (L, 0, -0.5), 7: (L, 0, -0.5), 9: (L, 0, 0.25)},           # a tie at q = 0.5: the lower a
        {2: (L, 0, NAN), 5: (L, 0, 0.5), 6: (L, 0, NAN)},              # NaN in the lead: it never wins, q = -0.5 does
        {4: (L, 0, -0.9), 20: (L | T, 0.5, -123.0)},                   # not terminal: q = 0.9 beats the reward 0.5
        {4: (L, 0, -0.9), 20: (L | T, 1.0, 123.0)},                    # a terminal reward beats the larger value
        {11: (L, 0, NAN), 12: (L, 0, NAN)},                            # all-NaN legal: the first legal a
        {},                                                            # no legal action
        {8: (L, 0, INF), 30: (L, 0, INF)},                             # q = -inf everywhere: no comparison succeeds
        {0: (0, 9.0, -9.0), 44: (L, 0, 0.75)},                         # an illegal pair's planes are not read as q
        {10: (L | T, -0.1, 5.0), 13: (L | T, -1.0, -5.0)},             # terminal pairs: rewards alone
    ]
    act, best = pick_reference(*_planes(cols), -1.0)
    assert act.dtype == np.int32 and best.dtype == np.float32
    assert act.tolist() == [3, 5, 4, 20, 11, -1, 8, 44, 10]
    want = np.array([0.5, -0.5, 0.9, 1.0, -np.inf, -np.inf, -np.inf, -0.75, -0.1], np.float32)
    assert best.tobytes() == want.tobytes()
    # sign = +1: the value as it stands
    act, best = pick_reference(*_planes(cols[:3]), 1.0)
    assert act.tolist() == [9, 5, 20] and best.tolist() == [0.25, 0.5, 0.5]
    with pytest.raises(ValueError):
        pick_reference(np.zeros((44, 2), np.uint8), np.zeros((44, 2), np.float32), np.zeros((44, 2), np.float32), -1.0)


def test_search_source_takes_no_engine_layer():
    """spl_search.hip reads planes, not tables: spl_common.h only, and it is one of the Makefile's NAMES."""
    csrc = os.path.join(REPO, "splendor-gym_amd", "csrc")
    inc = re.findall(r'^#include "([^"]+)"', open(os.path.join(csrc, "spl_search.hip")).read(), re.M)
    assert inc == ["../../include/splendor_search.h", "spl_common.h"], inc
    names = re.search(r"^NAMES := (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert "spl_search" in names and "spl_engine" in names
    # the successor layer sits on the step layer and below, never on the multi-wave layers
    layers = re.findall(r'^#include "(spl_engine_\w+\.h)"', open(os.path.join(csrc, "spl_engine_succ.h")).read(), re.M)
    assert set(layers) <= {"spl_engine_%s.h" % k for k in ("args", "stamps", "base", "rules", "obs", "deal", "step")}, layers
