"""The ragged one-ply search without a GPU (include/splendor_search.h, SPL_SEARCH_PAIRS): the ctypes mirrors of
spl_succ_pairs_args_t / spl_pick_pairs_args_t against the header, every refusal of spl_successors_pairs and
spl_search_pick_pairs on the host before any device work, pairs_reference and pick_pairs_reference (the numpy
oracles of the kernels' tests) on written-out cases and against pick_reference, and the new engine layer's place."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "splendor-gym_amd", "csrc")
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


def _members(src, tname):
    body = re.search(r"typedef struct \{([^{]*?)\} " + tname + ";", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [re.sub(r"[\s*]", "", part).split(" ")[-1] for part in
                  re.sub(r"^\s*(?:const\s+)?[a-z0-9_]+\s", "", decl.strip()).split(",") if part.strip()]
    return names


def test_abi_constants_and_struct_sizes():
    native, lib = _lib()
    src = open(os.path.join(REPO, "include", "splendor_search.h")).read()
    assert re.search(r"#define SPL_SEARCH_PAIRS 1\b", src) and native.SEARCH_PAIRS == 1
    assert re.search(r"#define SPL_SEARCH_ABI 1\b", src)  # the additions did not move it
    assert lib.spl_search_abi_version() == native.SEARCH_ABI == 1
    assert lib.spl_abi_version() == 9
    assert ctypes.sizeof(native.SuccPairsArgs) == 8 * 8 + 8  # eight pointers, capacity, padding
    assert native.SuccPairsArgs.capacity.offset == 64
    assert ctypes.sizeof(native.PickPairsArgs) == 7 * 8 + 4 * 4  # seven pointers, three scalars, padding
    assert (native.PickPairsArgs.sign.offset, native.PickPairsArgs.capacity.offset,
            native.PickPairsArgs.reserved.offset) == (56, 60, 64)
    for cls, tname in ((native.SuccPairsArgs, "spl_succ_pairs_args_t"), (native.PickPairsArgs, "spl_pick_pairs_args_t")):
        assert _members(src, tname) == [f[0] for f in cls._fields_], tname
    for name in ("spl_successors_pairs", "spl_search_pick_pairs"):
        assert re.search(r"\bint %s\(" % name, src) and hasattr(lib, name) and name in native.SIGNATURES


def test_successors_pairs_refusals():
    native, lib = _lib()
    full = dict(obs_u8=P, flags=P, reward=P, pair=P, mask_bits=P, winner=P, legal=P, base=P, capacity=100)
    args = lambda **kw: ctypes.byref(native.SuccPairsArgs(**kw))
    ctx = ctypes.c_void_p(P)  # never dereferenced before the refusals below
    arena = native.ArenaDesc(P, lib.spl_arena_bytes(10, 2), 10, 2, 0, 0)
    call = lambda **kw: lib.spl_successors_pairs(ctx, ctypes.byref(arena), args(**{**full, **kw}), None)
    _refused(lib, lib.spl_successors_pairs(None, ctypes.byref(arena), args(**full), None), "null context")
    _refused(lib, lib.spl_successors_pairs(ctx, None, args(**full), None), "null arena")
    _refused(lib, lib.spl_successors_pairs(ctx, ctypes.byref(native.ArenaDesc(None, 0, 10, 2, 0, 0)), args(**full), None),
             "null arena")
    _refused(lib, lib.spl_successors_pairs(ctx, ctypes.byref(native.ArenaDesc(P, 16, 10, 2, 0, 0)), args(**full), None),
             "too small")
    _refused(lib, lib.spl_successors_pairs(ctx, ctypes.byref(arena), None, None), "null")
    for name in ("obs_u8", "flags", "reward", "pair", "legal", "base"):
        _refused(lib, call(**{name: None}), "null")
    _refused(lib, call(obs_u8=P + 8), "aligned")
    for name, off in (("reward", 2), ("pair", 2), ("base", 2), ("mask_bits", 4), ("legal", 4)):
        _refused(lib, call(**{name: P + off}), "aligned")
    for cap in (0, -1):
        _refused(lib, call(capacity=cap), "capacity")
    many = 2 ** 31 // 45 + 1  # the first table count whose 45 n does not fit int32
    big = native.ArenaDesc(P, lib.spl_arena_bytes(many, 2), many, 2, 0, 0)
    _refused(lib, lib.spl_successors_pairs(ctx, ctypes.byref(big), args(**full), None), "int32")


def test_pick_pairs_refusals():
    native, lib = _lib()
    full = dict(legal=P, base=P, flags=P, reward=P, value=P, action=P, best_q=P, sign=-1.0, capacity=8)
    args = lambda **kw: ctypes.byref(native.PickPairsArgs(**kw))
    _refused(lib, lib.spl_search_pick_pairs(4, None, None), "null")
    for n in (0, -1):
        _refused(lib, lib.spl_search_pick_pairs(n, args(**full), None), "positive")
    for name in ("legal", "base", "flags", "reward", "value", "action"):
        _refused(lib, lib.spl_search_pick_pairs(4, args(**{**full, name: None}), None), "null")
    _refused(lib, lib.spl_search_pick_pairs(4, args(**{**full, "legal": P + 4}), None), "aligned")
    for name in ("base", "reward", "value", "action", "best_q"):
        _refused(lib, lib.spl_search_pick_pairs(4, args(**{**full, name: P + 2}), None), "aligned")
    for cap in (0, -1):
        _refused(lib, lib.spl_search_pick_pairs(4, args(**{**full, "capacity": cap}), None), "capacity")


def _planes(n, cols):
    """[45, n] planes from {table: {a: (flags, reward, value)}}; every other pair is illegal."""
    flags, reward, value = np.zeros((45, n), np.uint8), np.zeros((45, n), np.float32), np.zeros((45, n), np.float32)
    for t, col in cols.items():
        for a, (f, r, v) in col.items():
            flags[a, t], reward[a, t], value[a, t] = f, r, v
    return dict(flags=flags, reward=reward, value=value)


# 130 tables: block 0 has pairs, block 1 (tables 64..127) has none, block 2 is partial (tables 128, 129)
CASE = {
    0: {3: (L, 0, -0.5), 7: (L, 0, -0.5), 9: (L, 0, 0.25)},   # a tie at q = 0.5: the lower a
    5: {2: (L, 0, NAN), 7: (L, 0, 0.5), 6: (L, 0, NAN)},       # NaN in the lead: it never wins
    63: {3: (L | T, 1.0, 123.0), 44: (L, 0, -0.9)},            # a terminal reward beats the value
    2: {11: (L, 0, NAN), 12: (L, 0, NAN)},                     # all-NaN legal: the first legal a
    128: {0: (L, 0, INF), 30: (L, 0, INF)},                    # q = -inf everywhere: no comparison succeeds
    129: {0: (L | T, -0.1, 5.0), 1: (0, 9.0, -9.0)},           # (129, 1) is not legal: no pair
}


def test_pairs_reference_written_out():
    from splendor_gym.search import pairs_reference
    n = 130
    R = pairs_reference(_planes(n, CASE))
    # by block, then action, then table: block 0's pairs, then block 2's; block 1 has none
    want = [(2, 5), (3, 0), (3, 63), (6, 5), (7, 0), (7, 5), (9, 0), (11, 2), (12, 2), (44, 63), (0, 128), (0, 129), (30, 128)]
    assert R["pair"].dtype == np.int32 and R["pair"].tolist() == [a * n + t for a, t in want]
    assert R["base"].dtype == np.int32 and R["base"].tolist() == [0, 10, 10, 13]
    assert R["legal"].dtype == np.uint64 and R["legal"].shape == (n,)
    legal = {0: 1 << 3 | 1 << 7 | 1 << 9, 5: 1 << 2 | 1 << 6 | 1 << 7, 63: 1 << 3 | 1 << 44, 2: 1 << 11 | 1 << 12,
             128: 1 | 1 << 30, 129: 1}
    assert [int(x) for x in R["legal"]] == [legal.get(t, 0) for t in range(n)]
    assert R["flags"].tolist() == [L, L, L | T, L, L, L, L, L, L, L, L, L | T, L]
    assert R["reward"].dtype == np.float32 and R["reward"][2] == 1.0 and R["reward"][11] == np.float32(-0.1)
    assert R["value"][[1, 4, 6, 9]].tolist() == [-0.5, -0.5, 0.25, np.float32(-0.9)]
    # rows ride along: a [45, n, 300] plane compacts to [m, 300] in the same order
    rows = np.zeros((45, n, 300), np.uint8)
    for i, (a, t) in enumerate(want):
        rows[a, t] = i + 1
    R = pairs_reference(dict(flags=_planes(n, CASE)["flags"], obs_u8=rows))
    assert R["obs_u8"].shape == (13, 300) and (R["obs_u8"] == np.arange(1, 14, dtype=np.uint8)[:, None]).all()
    # no legal pair at all; a single table
    R = pairs_reference(_planes(65, {}))
    assert R["base"].tolist() == [0, 0, 0] and R["pair"].shape == (0,) and not R["legal"].any()
    R = pairs_reference(_planes(1, {0: {44: (L, 0, 0)}}))
    assert R["base"].tolist() == [0, 1] and R["pair"].tolist() == [44] and int(R["legal"][0]) == 1 << 44
    with pytest.raises(ValueError):
        pairs_reference(dict(flags=np.zeros((44, 2), np.uint8)))


def test_pick_pairs_reference_written_out():
    from splendor_gym.search import pairs_reference, pick_pairs_reference
    n = 130
    R = pairs_reference(_planes(n, CASE))
    act, best = pick_pairs_reference(R["legal"], R["base"], R["flags"], R["reward"], R["value"], -1.0)
    assert act.dtype == np.int32 and best.dtype == np.float32 and act.shape == best.shape == (n,)
    want_a = np.full(n, -1, np.int32)  # a table with no legal action: -1
    want_q = np.full(n, -np.inf, np.float32)
    for t, (a, q) in {0: (3, 0.5), 5: (7, -0.5), 63: (3, 1.0), 2: (11, -np.inf), 128: (0, -np.inf), 129: (0, -0.1)}.items():
        want_a[t], want_q[t] = a, q
    assert act.tolist() == want_a.tolist() and best.tobytes() == want_q.tobytes()
    act, best = pick_pairs_reference(R["legal"], R["base"], R["flags"], R["reward"], R["value"], 1.0)
    assert (act[0], act[5], act[63]) == (9, 7, 3) and (best[0], best[5], best[63]) == (0.25, 0.5, 1.0)
    # capacity 11: the pairs at 11 and 12, (0, 129) and (30, 128), take no part
    act, best = pick_pairs_reference(R["legal"], R["base"], R["flags"], R["reward"], R["value"], -1.0, capacity=11)
    assert act[129] == -1 and best[129] == -np.inf and act[128] == 0 and act[:128].tolist() == want_a[:128].tolist()
    # the legal words decide what is a pair, not the LEGAL bit of the compacted flags
    act2, _ = pick_pairs_reference(R["legal"], R["base"], R["flags"] & ~np.uint8(L), R["reward"], R["value"], -1.0)
    assert act2.tolist() == want_a.tolist()
    with pytest.raises(ValueError):
        pick_pairs_reference(R["legal"], R["base"][:-1], R["flags"], R["reward"], R["value"], -1.0)


def random_planes(n, seed):
    rs = np.random.default_rng(seed)
    kinds = np.array([0, 0, 0, L, L, L | 0x08, L | T, L | T | 0x04], np.uint8)
    flags = kinds[rs.integers(0, len(kinds), (45, n))]
    flags[:, rs.random(n) < 0.1] = 0  # tables without a legal action
    if n > 128:
        flags[:, 64:128] = 0          # a whole block without a pair
    value = np.round(rs.normal(size=(45, n)), 1).astype(np.float32)  # one decimal: ties are common
    reward = rs.choice(np.array([1.0, -1.0, 0.0, -0.1], np.float32), (45, n))
    for x, p in ((NAN, 0.05), (INF, 0.03), (-INF, 0.03)):
        value[rs.random((45, n)) < p] = x
    col = rs.random(n)
    value[:, col < 0.1] = NAN
    value[:, col > 0.9] = INF
    return dict(flags=flags, reward=reward, value=value)


@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 300])
def test_pick_over_pairs_is_the_dense_pick(n, sign):
    from splendor_gym.search import pairs_reference, pick_pairs_reference, pick_reference
    d = random_planes(n, 7 * n + int(sign))
    R = pairs_reference(d)
    m = int(R["base"][-1])
    assert m == int(((d["flags"] & L) != 0).sum()) == len(R["pair"])
    a, t = R["pair"] // n, R["pair"] % n
    keys = list(zip((t // 64).tolist(), a.tolist(), t.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == m
    got = pick_pairs_reference(R["legal"], R["base"], R["flags"], R["reward"], R["value"], sign)
    want = pick_reference(d["flags"], d["reward"], d["value"], sign)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_the_pairs_layer_sits_on_the_successor_layer():
    """spl_engine_pairs.h is a layer of the engine: included once by spl_engine.hip, after spl_engine_succ.h, and it
    includes only layers below it; spl_engine_succ.h and spl_search.hip keep their include sets."""
    layer = re.compile(r'^#include "(spl_engine_\w+\.h)"', re.M)
    order = layer.findall(open(os.path.join(CSRC, "spl_engine.hip")).read())
    assert order.count("spl_engine_pairs.h") == 1
    at = order.index("spl_engine_pairs.h")
    assert "spl_engine_succ.h" in order[:at]
    mine = layer.findall(open(os.path.join(CSRC, "spl_engine_pairs.h")).read())
    assert "spl_engine_succ.h" in mine and all(h in order[:at] for h in mine), mine
    below = layer.findall(open(os.path.join(CSRC, "spl_engine_succ.h")).read())
    assert "spl_engine_pairs.h" not in below
    inc = re.findall(r'^#include "([^"]+)"', open(os.path.join(CSRC, "spl_search.hip")).read(), re.M)
    assert inc == ["../../include/splendor_search.h", "spl_common.h"], inc
