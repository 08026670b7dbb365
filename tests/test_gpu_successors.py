"""One-ply successors on the device (include/splendor_search.h): spl_successors against the CPU oracle for every
(table, action) pair — random positions, the reference's crafted states, the MT continuation, an edited card
table, the bounds-check build — its read-only and full-write contracts, spl_search_pick against its numpy
restatement bit for bit, and OnePlyValuePolicy."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edited_tables as et
import successors_ref as sr
from oracle.oracle import Oracle, view_to_table

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CHECKED = os.path.join(os.path.dirname(HERE), "splendor-gym_amd", "splendor_gym", "libsplendor_amd_checked.so")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def edge_cases():
    with open(os.path.join(GOLD, "edge_cases.json")) as f:
        return json.load(f)


def engine(n, P, **kw):
    from splendor_gym.device import Engine
    return Engine(n, P, **kw)


def all_planes(eng):
    """One call with both row forms and every optional plane, into buffers pre-filled with 0xAB."""
    return sr.planes(eng.successors(obs=True, obs_u8=True, mask_bits=True, winner=True, out=sr.prefilled(eng)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("P", [2, 3, 4])
def test_parity_with_the_oracle(orc, P, n):
    """40 uniform-random plies from seeded deals, then every pair against Oracle.env_step: single, partial, full,
    full + 1 and three blocks with a partial last."""
    e = engine(n, P)
    e.reset(seeds=list(range(300 * P + n, 300 * P + 2 * n)))
    sr.random_plies(e, 40, seed=7 * P + n)
    R = sr.oracle_pairs(orc, e.download())
    got = all_planes(e)
    sr.compare(got, R, f"P={P} n={n}")
    if n >= 63:  # the comparison saw both kinds of pair, and moves that drew
        assert (R["flags"] & sr.LEGAL).any() and not (R["flags"] & sr.LEGAL).all()
        assert (R["flags"] & sr.DREW).any()


def crafted_engine(edge_cases, P, extra=()):
    cs = [c for c in edge_cases if c["P"] == P]
    recs = np.stack([view_to_table(c["before"]) for c in cs] + list(extra))
    e = engine(len(recs), P)
    e.reset(seeds=list(range(len(recs))))
    e.upload(recs)
    return e, cs


def late_table(orc):
    """A two-player table at move 301, seat 1 to move (past the byte of the staged row): every legal move ends
    it by the turn limit with move_count 302 in its row."""
    v = orc.initial_state(2, 77)
    v.update(move_count=301, turn_count=151, to_play=1)
    return view_to_table(v)


@pytest.mark.parametrize("P", [2, 3, 4])
def test_crafted_states(orc, edge_cases, P):
    """tests/golden/edge_cases.json: all 45 actions of every state against the oracle, and the reference's own
    recorded step against its pair (token returns, nobles, the turn limit, reserved buys, empty decks, terminal
    tables, which have no legal pair); at two players also a table with move_count > 255."""
    e, cs = crafted_engine(edge_cases, P, [late_table(orc)] if P == 2 else [])
    R = sr.oracle_pairs(orc, e.download())
    got = all_planes(e)
    sr.compare(got, R, f"crafted P={P}")
    seen = dict(terminal=0, turn_limit=0, legal=0)
    for i, c in enumerate(cs):
        a = c["action"]
        if c["exception"] == "RuntimeError":  # a table that is over: no legal pair
            assert not got["flags"][:, i].any(), c["name"]
            seen["terminal"] += 1
            continue
        if c["exception"] or c["flags"] & 3:  # out of range, illegal, or no legal move at all
            if 0 <= a < 45:
                assert got["flags"][a, i] == 0, c["name"]
            continue
        f = int(got["flags"][a, i])
        assert f & sr.LEGAL, c["name"]
        np.testing.assert_array_equal(got["obs"][a, i], np.array(c["obs"], np.int32), err_msg=c["name"])
        assert int(got["mask"][a, i]) == c["mask"], c["name"]
        assert got["reward"][a, i] == np.float32(c["reward"]), c["name"]
        assert bool(f & sr.TERMINATED) == bool(c["terminated"]), c["name"]
        assert bool(f & sr.TURN_LIMIT) == bool(c["flags"] & 4), c["name"]
        seen["legal"] += 1
        seen["turn_limit"] += bool(c["flags"] & 4)
    assert seen["legal"] > 50 and seen["turn_limit"] > 0, seen
    if P == 2:
        late = len(cs)
        legal = (got["flags"][:, late] & sr.LEGAL) != 0
        assert legal.any() and (got["obs"][legal, late, 295] == 302).all() and (got["u8"][legal, late, 297] == 1).all()
        assert (got["flags"][legal, late] & (sr.TERMINATED | sr.TURN_LIMIT) == sr.TERMINATED | sr.TURN_LIMIT).all()


def heavy_tables(orc, n, seed):
    """Deals whose player to move holds 50..200 tokens of several colours: a take or a reserve returns hundreds
    of tokens, far past the streamed MT outputs (tests/test_gpu_rng_continuation.py)."""
    rs = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        v = orc.initial_state(2, 500 + i)
        p = v["players"][v["to_play"]]
        p["tokens"] = [0] * 6
        for c in rs.choice(5, int(rs.integers(1, 6)), replace=False):
            p["tokens"][int(c)] = int(rs.integers(50, 201))
        p["tokens"][5] = int(rs.integers(0, 3))
        recs.append(view_to_table(v))
    return recs


def test_the_continuation_path(orc, edge_cases):
    """Stream limit 1: every token return of the crafted token cases and of tables holding hundreds of tokens
    runs the full-state MT continuation (LaneMT in the wave's LDS)."""
    from splendor_gym import _native
    lib = _native.load_library()
    recs = [view_to_table(c["before"]) for c in edge_cases if c["P"] == 2 and c["name"].startswith("token_")]
    assert len(recs) >= 3
    recs = np.stack(recs + heavy_tables(orc, 24, 5))
    e = engine(len(recs), 2)
    e.reset(seeds=list(range(len(recs))))
    e.upload(recs)
    R = sr.oracle_pairs(orc, e.download())
    try:
        _native.check(lib, lib.spl_debug_set_stream_limit(1))
        got = all_planes(e)
        e.torch.cuda.synchronize()
    finally:
        _native.check(lib, lib.spl_debug_set_stream_limit(454))
    sr.compare(got, R, "stream limit 1")
    sr.compare(all_planes(e), R, "stream limit 454")


def test_read_only_and_deterministic():
    """The arena's bytes are the same after a call, a trajectory does not see the call, and two calls write the
    same bytes in every plane."""
    import torch
    n = 130
    a, b = engine(n, 2), engine(n, 2)
    for e in (a, b):
        e.reset(seeds=list(range(40, 40 + n)))
        sr.random_plies(e, 25, seed=3)
    before = a.arena.clone()
    s1 = a.successors(obs=True, obs_u8=True, mask_bits=True, winner=True, out=sr.prefilled(a))
    assert torch.equal(a.arena, before)
    s2 = a.successors(obs=True, obs_u8=True, mask_bits=True, winner=True, out=sr.prefilled(a))
    for k in ("obs", "obs_u8", "flags", "mask_bits", "winner"):
        assert torch.equal(getattr(s1, k), getattr(s2, k)), k
    assert torch.equal(s1.reward.view(torch.int32), s2.reward.view(torch.int32))
    na, nb = (torch.zeros(n, dtype=torch.int32, device=a.device) for _ in range(2))
    a.sample_uniform(out=na, seed=9, ply=0)
    b.sample_uniform(out=nb, seed=9, ply=0)
    for k in range(20):
        a.step(na.clone(), next_actions=na, policy_seed=9, ply=k + 1)
        b.step(nb.clone(), next_actions=nb, policy_seed=9, ply=k + 1)
        if k == 10:
            a.successors()
        for name in ("obs", "mask", "reward", "terminated", "flags"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
    assert a.download().tobytes() == b.download().tobytes()


def test_an_edited_card_table(orc):
    """FREE (cards with id % 7 == 0 cost nothing): a context of its own card table, parity at 65 tables."""
    cards, nobles = et.free_tables()
    e = engine(65, 2, cards=cards, nobles=nobles)
    e.reset(seeds=list(range(900, 965)))
    sr.random_plies(e, 12, seed=21)
    with et.oracle_tables(orc, cards, nobles):
        R = sr.oracle_pairs(orc, e.download())
    sr.compare(all_planes(e), R, "FREE")
    buys = R["flags"][15:27] & sr.LEGAL
    assert buys.any()


def random_pick_planes(n, seed):
    rs = np.random.default_rng(seed)
    kinds = np.array([0, 0, sr.LEGAL, sr.LEGAL, sr.LEGAL | sr.DREW, sr.LEGAL | sr.TERMINATED,
                      sr.LEGAL | sr.TERMINATED | sr.TURN_LIMIT], np.uint8)
    flags = kinds[rs.integers(0, len(kinds), (45, n))]
    flags[:, rs.random(n) < 0.1] = 0  # tables without a legal action
    value = np.round(rs.normal(size=(45, n)), 1).astype(np.float32)  # one decimal: ties are common
    reward = rs.choice(np.array([1.0, -1.0, 0.0, -0.1], np.float32), (45, n))
    for x, p in ((np.float32("nan"), 0.05), (np.float32("inf"), 0.03), (np.float32("-inf"), 0.03)):
        value[rs.random((45, n)) < p] = x
    col = rs.random(n)
    value[:, col < 0.1] = np.float32("nan")   # all-NaN tables
    value[:, col > 0.9] = np.float32("inf")   # q = -inf everywhere with sign -1
    return flags, reward, value


@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_pick_against_the_reference(n, sign):
    import torch
    from splendor_gym.search import pick, pick_reference
    flags, reward, value = random_pick_planes(n, 100 + n)
    want_a, want_q = pick_reference(flags, reward, value, sign)
    dev = torch.device("cuda:0")
    f, r, v = (torch.from_numpy(x).to(dev) for x in (flags, reward, value))
    best = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    act = pick(f, r, v, sign, best_q=best)
    assert act.cpu().numpy().tobytes() == want_a.tobytes()
    assert best.cpu().numpy().tobytes() == want_q.tobytes()
    if n > 1:
        assert (want_a < 0).any() and (want_a > 0).any()


def golden_fused():
    from safetensors.torch import load_file
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.policy import ActorCritic
    m = ActorCritic().to("cuda:0").eval()
    m.load_state_dict(load_file(os.path.join(GOLD, "ppo_splendor_latest.safetensors"), device="cuda:0"))
    return FusedActorCritic(m)


def zero_critic_fused():
    import torch
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.policy import ActorCritic
    m = ActorCritic().to("cuda:0").eval()
    with torch.no_grad():
        for p in m.critic.parameters():
            p.zero_()
    return FusedActorCritic(m)


def test_policy_equals_its_three_calls():
    """OnePlyValuePolicy.act == pick_reference over a separate successors call and a separate SPL_ACT_VALUE call
    on the same rows: same kernels, same inputs, so equal."""
    from splendor_gym.search import OnePlyValuePolicy, pick_reference
    fused = golden_fused()
    n = 130
    e = engine(n, 2)
    e.reset(seeds=list(range(5000, 5000 + n)))
    sr.random_plies(e, 30, seed=4)
    pol = OnePlyValuePolicy(fused)
    got = pol.act(e).cpu().numpy().copy()
    again = pol.act(e).cpu().numpy()
    s = e.successors()
    value = fused.get_value(s.obs_u8.view(45 * n, 300)).view(45, n)
    want, _ = pick_reference(s.flags.cpu().numpy(), s.reward.cpu().numpy(), value.cpu().numpy(), -1.0)
    assert got.tobytes() == want.tobytes() == again.tobytes()
    legal = (s.flags.cpu().numpy() & sr.LEGAL) != 0
    live = legal.any(axis=0)
    assert live.any() and legal[got[live], np.flatnonzero(live)].all() and (got[~live] == -1).all()
    assert len(set(got[live].tolist())) > 1  # the critic prefers different moves on different tables


def winning_buy_table(orc):
    """Two players, seat 1 to move at 14 prestige with every visible card affordable (bonuses, no nobles to earn),
    the game-over bit already set by seat 0 at 15: a purchase worth a point ends the game in seat 1's favour
    (15 : 15, fewer cards), every other move loses it."""
    for seed in range(200):
        v = orc.initial_state(2, seed)
        if any(orc.cards[c][2] >= 1 for c in v["board"] if c >= 0):
            break
    v["players"][0].update(prestige=15, bonuses=[8, 8, 8, 8, 8])
    v["players"][1].update(prestige=14, bonuses=[7, 7, 7, 7, 7], tokens=[0] * 6)
    v.update(nobles=[], to_play=1, game_over=1, move_count=41, turn_count=21)
    return v


def test_policy_with_a_zero_critic(orc):
    from splendor_gym.search import OnePlyValuePolicy
    pol = OnePlyValuePolicy(zero_critic_fused())
    e = engine(2, 2)
    e.reset(seeds=[11, 12])
    assert pol.act(e).tolist() == [0, 0]  # a fresh deal: every q ties, the lowest legal action
    v = winning_buy_table(orc)
    e.upload(view_to_table(v), first=1)
    act = pol.act(e).tolist()
    assert act[0] == 0
    a = act[1]
    s = e.successors()
    f, r = s.flags.cpu().numpy()[:, 1], s.reward.cpu().numpy()[:, 1]
    assert 15 <= a < 27 and f[a] & sr.LEGAL and f[a] & sr.TERMINATED and r[a] == 1.0
    assert orc.cards[v["board"][a - 15]][2] >= 1
    assert (f[:15] & sr.TERMINATED).all() and (r[:15][(f[:15] & sr.LEGAL) != 0] == -1.0).all()  # the takes lose
    assert a == int(np.flatnonzero((f & sr.LEGAL != 0) & (r == 1.0))[0])


def test_policy_refuses_three_players():
    from splendor_gym.search import OnePlyValuePolicy
    pol = OnePlyValuePolicy(zero_critic_fused())
    e = engine(4, 3)
    e.reset(seeds=[1, 2, 3, 4])
    with pytest.raises(ValueError):
        pol.act(e)
    from splendor_gym.fused_policy import FusedActorCritic
    with pytest.raises(ValueError):
        OnePlyValuePolicy(FusedActorCritic(pol.fused.model, with_critic=False))


def test_refusals_launch_nothing():
    from splendor_gym import _native
    e = engine(65, 2)
    e.reset(seeds=list(range(65)))
    s = sr.prefilled(e)
    want = {k: getattr(s, k).clone() for k in s.__slots__}
    full = dict(obs_u8=s.obs_u8.data_ptr(), obs=s.obs.data_ptr(), flags=s.flags.data_ptr(), reward=s.reward.data_ptr(),
                mask_bits=s.mask_bits.data_ptr(), winner=s.winner.data_ptr())
    call = lambda desc, **kw: e.lib.spl_successors(e.ctx, desc, ctypes.byref(_native.SuccArgs(**{**full, **kw})), e.stream())
    desc = ctypes.byref(e.desc)
    assert call(desc, obs=None, obs_u8=None) == -1 and b"at least one" in e.lib.spl_last_error()
    assert call(desc, obs_u8=s.obs_u8.data_ptr() + 4) == -1 and b"aligned" in e.lib.spl_last_error()
    assert call(desc, obs=s.obs.data_ptr() + 8) == -1 and b"aligned" in e.lib.spl_last_error()
    assert call(None) == -1 and b"null arena" in e.lib.spl_last_error()
    null_base = _native.ArenaDesc(None, e.desc.bytes, e.n, 2, 0, 0)
    assert call(ctypes.byref(null_base)) == -1 and b"null arena" in e.lib.spl_last_error()
    e.torch.cuda.synchronize()
    for k, w in want.items():
        assert e.torch.equal(getattr(s, k).view(e.torch.uint8), w.view(e.torch.uint8)), k
    assert call(desc) == 0  # the same block, complete: accepted


def test_checked_build():
    """One parity case at 65 tables through the bounds-check build, in a child process (the library is chosen
    at load time): equal to the oracle, no invariant violation recorded."""
    assert os.path.exists(CHECKED), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, SPLENDOR_AMD_LIB=CHECKED)
    r = subprocess.run([sys.executable, os.path.join(HERE, "successors_checked_child.py")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["pairs"] == 45 * 65 and res["legal"] > 0
    assert res["flags"] == 0, f"invariant violations recorded: {res['flags']:#x}"
