"""The evaluation league without a GPU (include/splendor_eval.h): the ABI constant and the ctypes mirrors,
every spl_eval_* entry point refusing bad arguments on the host before any device work, and the
greedy_v2 fixture (tests/golden/eval_v2.json, the reference's bank-aware opponent) reproduced by the
host callable over the oracle-backed env."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
P = 0x10000  # a plausible, aligned, never-dereferenced device address: every case below is refused first


def _lib():
    from splendor_gym import _native
    return _native, _native.load_library()  # dlopen only: no GPU needed


def _refused(lib, code, word):
    assert code < 0, code
    msg = lib.spl_last_error()
    assert msg and word.encode() in msg, msg


def test_abi_constant_and_struct_sizes():
    native, lib = _lib()
    src = open(os.path.join(REPO, "include", "splendor_eval.h")).read()
    assert re.search(r"#define SPL_EVAL_ABI 1\b", src)
    assert re.search(r"#define SPL_POLICY_GREEDY_V2 3\b", src) and re.search(r"#define SPL_EVAL_KEEP \(-1\)", src)
    assert lib.spl_eval_abi_version() == native.EVAL_ABI == 1
    assert (native.POLICY_GREEDY_V2, native.EVAL_KEEP, native.EVAL_COLS) == (3, -1, 8)
    # spl_eval_act_t: 8 pointers, seed, ply, table0, policy + reserved
    assert ctypes.sizeof(native.EvalAct) == 8 * 8 + 3 * 8 + 2 * 4
    assert native.EvalAct.seed.offset == 64 and native.EvalAct.policy.offset == 88
    assert ctypes.sizeof(native.EvalCheck) == 5 * 8
    assert ctypes.sizeof(native.EvalTally) == 9 * 8
    assert ctypes.sizeof(native.EvalReduce) == 8 * 8
    # the mirrors name the header's members in the header's order
    for cls, tname in ((native.EvalAct, "spl_eval_act_t"), (native.EvalCheck, "spl_eval_check_t"),
                       (native.EvalTally, "spl_eval_tally_t"), (native.EvalReduce, "spl_eval_reduce_t")):
        body = re.search(r"typedef struct \{([^{]*?)\} " + tname + ";", src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            names += [re.sub(r"[\s*]", "", part).split(" ")[-1] for part in
                      re.sub(r"^\s*(?:const\s+)?[a-z0-9_]+\s", "", decl.strip()).split(",") if part.strip()]
        assert names == [f[0] for f in cls._fields_], (tname, names)


ACT = dict(mask=P, obs=P, action=P, policy=0)


def test_scripted_act_refusals():
    native, lib = _lib()
    act = lambda **kw: ctypes.byref(native.EvalAct(**kw))
    _refused(lib, lib.spl_eval_scripted_act(4, None, None), "null")
    for n in (0, -1):
        _refused(lib, lib.spl_eval_scripted_act(n, act(**ACT), None), "positive")
    _refused(lib, lib.spl_eval_scripted_act(4, act(**{**ACT, "obs_u8": P}), None), "exactly one")  # both
    _refused(lib, lib.spl_eval_scripted_act(4, act(**{**ACT, "obs": None}), None), "exactly one")  # neither
    for name in ("mask", "action"):
        _refused(lib, lib.spl_eval_scripted_act(4, act(**{**ACT, name: None}), None), "null")
    for name in ("table_key", "ply_base", "errors"):  # the 8-byte planes
        _refused(lib, lib.spl_eval_scripted_act(4, act(**{**ACT, name: P + 4}), None), "aligned")
    for name in ("obs", "action", "policy_of"):
        _refused(lib, lib.spl_eval_scripted_act(4, act(**{**ACT, name: P + 2}), None), "aligned")
    _refused(lib, lib.spl_eval_scripted_act(4, act(**{**ACT, "obs": None, "obs_u8": P + 1}), None), "aligned")
    for bad in (4, -2):  # a scalar policy outside -1..3 (a per-table one is counted on the device)
        _refused(lib, lib.spl_eval_scripted_act(4, act(**{**ACT, "policy": bad}), None), "unknown policy")


def test_check_and_tally_refusals():
    native, lib = _lib()
    full = dict(action=P, mask=P, playing=P, checks=P, illegal=P)
    chk = lambda **kw: ctypes.byref(native.EvalCheck(**kw))
    _refused(lib, lib.spl_eval_check(4, None, None), "null")
    _refused(lib, lib.spl_eval_check(0, chk(**full), None), "positive")
    for name in full:
        _refused(lib, lib.spl_eval_check(4, chk(**{**full, name: None}), None), "null")
    for name in ("action", "checks", "illegal"):
        _refused(lib, lib.spl_eval_check(4, chk(**{**full, name: P + 2}), None), "aligned")
    full = {k: P for k in ("done", "game_ended_on", "agent_step_reward", "opp_reward", "final_obs", "playing", "result",
                           "turns", "prestige")}
    tal = lambda **kw: ctypes.byref(native.EvalTally(**kw))
    _refused(lib, lib.spl_eval_tally(4, None, None), "null")
    _refused(lib, lib.spl_eval_tally(0, tal(**full), None), "positive")
    for name in full:
        _refused(lib, lib.spl_eval_tally(4, tal(**{**full, name: None}), None), "null")
    for name in ("agent_step_reward", "opp_reward", "final_obs", "turns", "prestige"):
        _refused(lib, lib.spl_eval_tally(4, tal(**{**full, name: P + 2}), None), "aligned")


def test_reduce_refusals():
    native, lib = _lib()
    full = {k: P for k in ("group_of", "playing", "result", "turns", "prestige", "checks", "illegal", "out")}
    red = lambda **kw: ctypes.byref(native.EvalReduce(**kw))
    _refused(lib, lib.spl_eval_reduce(4, 1, None, None), "null")
    _refused(lib, lib.spl_eval_reduce(0, 1, red(**full), None), "n must be positive")
    for G in (0, -1):
        _refused(lib, lib.spl_eval_reduce(4, G, red(**full), None), "G must be positive")
    for name in full:
        if name != "group_of":  # NULL group_of: one group
            _refused(lib, lib.spl_eval_reduce(4, 1, red(**{**full, name: None}), None), "null")
    _refused(lib, lib.spl_eval_reduce(4, 1, red(**{**full, "out": P + 4}), None), "aligned")
    _refused(lib, lib.spl_eval_reduce(4, 1, red(**{**full, "turns": P + 2}), None), "aligned")


def test_step_still_rejects_the_new_policy_id():
    """spl_step's fused policies stay 0..2: greedy_v2 lives in spl_eval_scripted_act only."""
    native, lib = _lib()
    arena = native.ArenaDesc(None, 0, 10, 2, 0, 0)
    args = native.StepArgs(actions=P, obs=P, mask=P, reward=P, terminated=P, flags=P, policy=native.POLICY_GREEDY_V2)
    assert lib.spl_step(None, ctypes.byref(arena), ctypes.byref(args), None) < 0


def test_batched_seeding_equals_numpy_seed_by_seed():
    """An evaluation deals tens of thousands of seeded games at once: pcg64_states hashes 32-bit seeds
    together in numpy, and must give PCG64(SeedSequence(seed))'s state for each, edge seeds included;
    other seeds (None, wider than 32 bits) still go one by one."""
    from splendor_gym import seeding
    rng = np.random.RandomState(3)
    seeds = [0, 1, 2**31 - 1, 2**31, 2**32 - 1] + rng.randint(0, 2**32, size=3000, dtype=np.uint64).tolist() + \
        rng.randint(1e9, size=1000).tolist()
    got = seeding.pcg64_states(seeds)
    assert got.dtype == np.uint64 and got.shape == (len(seeds), 4) and got.flags["C_CONTIGUOUS"]
    assert got.tolist() == [seeding.pcg64_state(s) for s in seeds]
    assert np.array_equal(got, seeding._pcg64_states_u32(seeds))  # the batched path is the one taken
    assert np.array_equal(seeding.pcg64_states(np.arange(5, dtype=np.int64)), seeding.pcg64_states(range(5)))
    wide = seeding.pcg64_states([2**32, 7, 2**63 + 5])
    assert wide.tolist() == [seeding.pcg64_state(s) for s in (2**32, 7, 2**63 + 5)]
    assert seeding.pcg64_states([None, 7]).shape == (2, 4) and seeding.pcg64_states([]).shape == (0, 4)


@pytest.mark.parametrize("case", range(4))
def test_greedy_v2_fixture_on_oracle_env(case):
    """scripts.eval_suite.eval_vs_opponent over the oracle-backed env against the host
    greedy_opponent_v2_factory(env) — the opponent reads the bank from env.state, as in the reference
    run that wrote tests/golden/eval_v2.json — reproduces the fixture."""
    from oracle_env import OracleSplendorEnv
    from splendor_gym.scripts.eval_suite import eval_vs_opponent, greedy_opponent_v2_factory
    from splendor_gym.wrappers.selfplay import SelfPlayWrapper
    with open(os.path.join(GOLD, "eval_v2.json")) as f:
        c = json.load(f)[case]
    assert c["opponent"] == "greedy_v2"

    def agent(obs, info):
        legal = np.flatnonzero(info["action_mask"])
        return int((legal[0] if c["agent"] == "first_legal" else legal[-1]) if len(legal) else 0)

    def make_env():
        inner = OracleSplendorEnv()
        assert hasattr(inner, "state")
        env = SelfPlayWrapper(inner, opponent_policy=greedy_opponent_v2_factory(inner))
        env.reset(seed=0)
        return env

    got = eval_vs_opponent(make_env, agent, n_games=c["n_games"], seed=c["seed"])
    want = c["result"]
    for k in ("n", "wins", "losses", "draws"):
        assert got[k] == want[k], (k, got, want)
    for k in ("win_rate", "win_rate_ci95", "avg_turns", "avg_prestige", "illegal_action_rate"):
        assert got[k] == pytest.approx(want[k], abs=1e-12), (k, got, want)
