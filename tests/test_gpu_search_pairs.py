"""The ragged one-ply search on the device (include/splendor_search.h, SPL_SEARCH_PAIRS): spl_successors_pairs against
the dense spl_successors call on the same arena, pair for pair (the dense call is held to the CPU oracle by
tests/test_gpu_successors.py) — random positions, a block that is over, crafted states, the MT continuation, an edited
card table, the bounds-check build — its overflow and read-only contracts, spl_search_pick_pairs against its numpy
restatement bit for bit, and OnePlyValuePolicy(compact=True) against the dense policy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edited_tables as et
import successors_ref as sr
from oracle.oracle import Oracle, view_to_table
from test_gpu_successors import crafted_engine, golden_fused, heavy_tables, late_table, random_pick_planes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CHECKED = os.path.join(os.path.dirname(HERE), "splendor-gym_amd", "splendor_gym", "libsplendor_amd_checked.so")
FILL = 0xAB
PLANES = ("obs_u8", "flags", "reward", "pair", "mask_bits", "winner")


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


def dense_planes(eng):
    """The dense call's planes on the host, under pairs_reference's names."""
    s = eng.successors(obs=False, obs_u8=True, mask_bits=True, winner=True)
    return {k: getattr(s, k).cpu().numpy() for k in ("flags", "reward", "obs_u8", "mask_bits", "winner")}


def prefilled_pairs(eng, rows, capacity, guard=256):
    """A SuccessorPairs of `capacity` whose planes hold `rows` >= capacity rows, every one inside an allocation of its
    own with `guard` bytes before and after, all bytes FILL.  Returns it and the allocations by plane name."""
    import torch
    from splendor_gym.device import SuccessorPairs
    whole, view = {}, {}
    nb = (eng.n + 63) // 64
    for k, count, width, dt in (("obs_u8", rows, 300, torch.uint8), ("flags", rows, 1, torch.uint8),
                                ("reward", rows, 1, torch.float32), ("pair", rows, 1, torch.int32),
                                ("mask_bits", rows, 1, torch.int64), ("winner", rows, 1, torch.int8),
                                ("legal", eng.n, 1, torch.int64), ("base", nb + 1, 1, torch.int32)):
        nbytes = count * width * torch.empty((), dtype=dt).element_size()
        whole[k] = torch.full((guard + nbytes + guard,), FILL, dtype=torch.uint8, device=eng.device)
        x = whole[k][guard:guard + nbytes].view(dt)
        view[k] = x.view(count, width) if width > 1 else x
    return SuccessorPairs(capacity=capacity, **view), whole


def host(pairs):
    """The host copies of a SuccessorPairs' planes, legal as uint64."""
    got = {k: getattr(pairs, k).cpu().numpy() for k in PLANES + ("base",)}
    got["legal"] = pairs.legal.cpu().numpy().view(np.uint64)
    return got


def guards_untouched(whole, guard=256):
    for k, w in whole.items():
        w = w.cpu().numpy()
        assert (w[:guard] == FILL).all() and (w[-guard:] == FILL).all(), f"{k}: bytes outside the plane were written"


def compare_with_dense(eng, tag, capacity=None):
    """One pairs call with every plane into canary-guarded buffers against the dense call on the same arena: legal,
    base and m, the order of `pair`, and every plane of every pair; nothing outside the planes or past m written.
    Returns (dense planes, the reference's pairs, the call's planes)."""
    from splendor_gym.search import pairs_reference
    D = dense_planes(eng)
    R = pairs_reference(D)
    m = int(R["base"][-1])
    cap = max(m, 1) if capacity is None else capacity
    assert cap >= m
    pairs, whole = prefilled_pairs(eng, cap + 3, cap)
    eng.successor_pairs(mask_bits=True, winner=True, out=pairs)
    assert pairs.total() == m, tag
    got = host(pairs)
    n = eng.n
    legal = np.zeros(n, np.uint64)  # the OR of the dense LEGAL flags
    for a in range(45):
        legal |= ((D["flags"][a] & sr.LEGAL) != 0).astype(np.uint64) << np.uint64(a)
    np.testing.assert_array_equal(got["legal"], legal, err_msg=f"{tag} legal")
    np.testing.assert_array_equal(got["base"], R["base"], err_msg=f"{tag} base")
    pair = got["pair"][:m]
    a, t = pair // n, pair % n
    keys = list(zip((t // 64).tolist(), a.tolist(), t.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == m, f"{tag}: pair is not in the contract's order"
    np.testing.assert_array_equal(pair, R["pair"], err_msg=f"{tag} pair")
    assert ((D["flags"][a, t] & sr.LEGAL) != 0).all()
    # every pair p < m: the row's 300 bytes and the small planes equal the dense element pair[p]
    np.testing.assert_array_equal(got["obs_u8"][:m], D["obs_u8"][a, t], err_msg=f"{tag} rows")
    np.testing.assert_array_equal(got["flags"][:m], D["flags"][a, t], err_msg=f"{tag} flags")
    assert got["reward"][:m].tobytes() == D["reward"][a, t].tobytes(), f"{tag} reward"
    np.testing.assert_array_equal(got["mask_bits"][:m], D["mask_bits"][a, t], err_msg=f"{tag} mask_bits")
    np.testing.assert_array_equal(got["winner"][:m], D["winner"][a, t], err_msg=f"{tag} winner")
    for k in PLANES:  # nothing at or past m
        assert (got[k][m:].view(np.uint8) == FILL).all(), f"{tag} {k}: written past m"
    guards_untouched(whole)
    return D, R, got


PLIES = {2: 70, 3: 40, 4: 25}  # random games last ~77 plies at 2p and ~29 at 4p: by then some tables are over, not all


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("P", [2, 3, 4])
def test_parity_with_the_dense_call(P, n):
    """Uniform-random plies from seeded deals without autoreset, then every pair against the dense call: single,
    partial, full, full + 1 and three blocks with a partial last."""
    e = engine(n, P)
    e.reset(seeds=list(range(300 * P + n, 300 * P + 2 * n)))
    sr.random_plies(e, PLIES[P] if n >= 63 else 20, seed=7 * P + n)
    _, R, got = compare_with_dense(e, f"P={P} n={n}")
    if n >= 63:  # the comparison saw tables that are over, live ones, and moves that drew
        assert (got["legal"] == 0).any() and (got["legal"] != 0).any()
        assert (R["flags"] & sr.DREW).any()


def over_table(orc, P):
    v = orc.initial_state(P, 5)
    v.update(game_over=1, to_play=0)
    return view_to_table(v)


@pytest.mark.parametrize("P", [2, 4])
def test_a_whole_block_that_is_over(orc, P):
    """130 tables of which 64..127 are over: block 1 has no pair, base[1] == base[2], and block 2's pairs follow
    block 0's directly."""
    e = engine(130, P)
    e.reset(seeds=list(range(130)))
    sr.random_plies(e, 20, seed=2)
    e.upload(np.stack([over_table(orc, P)] * 64), first=64)
    _, R, got = compare_with_dense(e, f"block over P={P}")
    assert not got["legal"][64:128].any() and got["base"][1] == got["base"][2] > 0 and got["base"][3] > got["base"][2]
    # every table over: m = 0 and nothing but legal and base is written
    e.upload(np.stack([over_table(orc, P)] * 130))
    _, R, got = compare_with_dense(e, f"all over P={P}")
    assert got["base"].tolist() == [0, 0, 0, 0]


def test_crafted_states_and_a_late_table(orc, edge_cases):
    """tests/golden/edge_cases.json at two players (token returns, nobles, the turn limit, reserved buys, empty
    decks, terminal tables) and a table at move 301: its pairs' rows carry move_count 302 in bytes 295 and 297."""
    e, cs = crafted_engine(edge_cases, 2, [late_table(orc)])
    _, R, got = compare_with_dense(e, "crafted")
    late = len(cs)
    m = int(got["base"][-1])
    mine = np.flatnonzero(got["pair"][:m] % e.n == late)
    assert len(mine) > 0
    assert (got["obs_u8"][mine, 297] == 1).all() and (got["obs_u8"][mine, 295] == (302 & 0xFF)).all()
    assert (got["flags"][mine] & (sr.TERMINATED | sr.TURN_LIMIT) == sr.TERMINATED | sr.TURN_LIMIT).all()
    over = [i for i, c in enumerate(cs) if c["exception"] == "RuntimeError"]
    assert over and not got["legal"][over].any()


def test_the_continuation_path(orc, edge_cases):
    """Stream limit 1: every token return of the crafted token cases and of tables holding hundreds of tokens runs
    the full-state MT continuation; the pairs written under it equal the dense call's under the product's limit."""
    from splendor_gym import _native
    from splendor_gym.search import pairs_reference
    lib = _native.load_library()
    recs = [view_to_table(c["before"]) for c in edge_cases if c["P"] == 2 and c["name"].startswith("token_")]
    assert len(recs) >= 3
    recs = np.stack(recs + heavy_tables(orc, 24, 5))
    e = engine(len(recs), 2)
    e.reset(seeds=list(range(len(recs))))
    e.upload(recs)
    R = pairs_reference(dense_planes(e))
    m = int(R["base"][-1])
    try:
        _native.check(lib, lib.spl_debug_set_stream_limit(1))
        pairs = e.successor_pairs(capacity=m, mask_bits=True, winner=True)
        e.torch.cuda.synchronize()
    finally:
        _native.check(lib, lib.spl_debug_set_stream_limit(454))
    got = host(pairs)
    assert got["base"].tolist() == R["base"].tolist()
    for k in PLANES:
        assert got[k][:m].tobytes() == R[k].tobytes(), k


def test_an_edited_card_table():
    """FREE (cards with id % 7 == 0 cost nothing): a context of its own card table, 65 tables."""
    cards, nobles = et.free_tables()
    e = engine(65, 2, cards=cards, nobles=nobles)
    e.reset(seeds=list(range(900, 965)))
    sr.random_plies(e, 12, seed=21)
    D, _, _ = compare_with_dense(e, "FREE")
    assert (D["flags"][15:27] & sr.LEGAL).any()  # purchases


def runs_of(R, n):
    """[(start, end)] of the (block, action) runs of a reference's pairs, in order."""
    a, t = R["pair"] // n, R["pair"] % n
    key = (t // 64) * 45 + a
    cut = np.flatnonzero(np.diff(key)) + 1
    starts = np.concatenate(([0], cut))
    return list(zip(starts.tolist(), np.concatenate((cut, [len(key)])).tolist()))


def test_overflow_writes_whole_runs_below_capacity_only():
    """capacity = m / 2 with planes of m rows inside canary-guarded allocations: legal and base are complete
    (base[-1] == m), the runs that fit whole below capacity are written and equal the reference's, and every other
    byte — the cut run's rows below capacity, every index >= capacity, the guards — is untouched."""
    from splendor_gym.search import pairs_reference
    n = 130
    e = engine(n, 2)
    e.reset(seeds=list(range(700, 700 + n)))
    sr.random_plies(e, 40, seed=9)
    R = pairs_reference(dense_planes(e))
    m = int(R["base"][-1])
    runs = runs_of(R, n)
    cut_inside = [cap for cap in range(m // 2, m // 2 + 64) if not any(e_ == cap for _, e_ in runs)]
    cap = cut_inside[0]  # about m / 2, and inside a run, so that a run is cut
    pairs, whole = prefilled_pairs(e, m, cap)
    e.successor_pairs(mask_bits=True, winner=True, out=pairs)
    assert pairs.total() == m and m > cap
    got = host(pairs)
    np.testing.assert_array_equal(got["legal"], R["legal"])
    np.testing.assert_array_equal(got["base"], R["base"])
    written = np.zeros(m, bool)
    for s, e_ in runs:
        written[s:e_] = e_ <= cap
    assert written.any() and not written[:cap].all() and not written[cap:].any()
    for k in PLANES:
        x, want = got[k].reshape(m, -1), R[k].reshape(m, -1)
        assert x[written].tobytes() == want[written].tobytes(), f"{k}: a run that fits"
        assert (x[~written].view(np.uint8) == FILL).all(), f"{k}: written outside the runs that fit"
    guards_untouched(whole)


def test_read_only_and_deterministic():
    """The arena's bytes are the same after a call, two calls write the same bytes, and a trajectory does not see a
    call in it."""
    import torch
    n = 130
    a, b = engine(n, 2), engine(n, 2)
    for e in (a, b):
        e.reset(seeds=list(range(40, 40 + n)))
        sr.random_plies(e, 25, seed=3)
    before = a.arena.clone()
    s1 = a.successor_pairs(mask_bits=True, winner=True)
    assert torch.equal(a.arena, before)
    s2 = a.successor_pairs(mask_bits=True, winner=True)
    assert torch.equal(a.arena, before)
    m = s1.total()
    assert 0 < m == s2.total() <= s1.capacity
    for k in PLANES + ("legal", "base"):
        x, y = getattr(s1, k), getattr(s2, k)
        rows = m if k in PLANES else x.shape[0]
        assert torch.equal(x[:rows].contiguous().view(torch.uint8), y[:rows].contiguous().view(torch.uint8)), k
    na, nb = (torch.zeros(n, dtype=torch.int32, device=a.device) for _ in range(2))
    a.sample_uniform(out=na, seed=9, ply=0)
    b.sample_uniform(out=nb, seed=9, ply=0)
    for k in range(20):
        a.step(na.clone(), next_actions=na, policy_seed=9, ply=k + 1)
        b.step(nb.clone(), next_actions=nb, policy_seed=9, ply=k + 1)
        if k == 10:
            a.successor_pairs()
        for name in ("obs", "mask", "reward", "terminated", "flags"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
    assert a.download().tobytes() == b.download().tobytes()


def device_pick(R, sign, capacity, n):
    """pick_pairs over a reference's planes on the device (one spare element behind each: m may be 0)."""
    import torch
    from splendor_gym.search import pick_pairs
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.concatenate((x, np.zeros(1, x.dtype)))).to(dev)
    best = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    legal = torch.from_numpy(R["legal"].view(np.int64)).to(dev)
    base = torch.from_numpy(R["base"]).to(dev)
    act = pick_pairs(legal, base, up(R["flags"]), up(R["reward"]), up(R["value"]), sign, capacity=capacity, best_q=best)
    return act.cpu().numpy(), best.cpu().numpy()


@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_pick_pairs_against_the_reference(n, sign):
    from splendor_gym.search import pairs_reference, pick_pairs_reference, pick_reference
    flags, reward, value = random_pick_planes(n, 100 + n)  # NaN, +-inf, ties, tables without a legal action
    R = pairs_reference(dict(flags=flags, reward=reward, value=value))
    m = int(R["base"][-1])
    want_a, want_q = pick_pairs_reference(R["legal"], R["base"], R["flags"], R["reward"], R["value"], sign)
    dense_a, dense_q = pick_reference(flags, reward, value, sign)
    assert want_a.tobytes() == dense_a.tobytes() and want_q.tobytes() == dense_q.tobytes()
    act, best = device_pick(R, sign, max(m, 1), n)
    assert act.tobytes() == want_a.tobytes()
    assert best.tobytes() == want_q.tobytes()
    if n > 1:
        assert (want_a < 0).any() and (want_a > 0).any()


def test_pick_pairs_with_a_capacity_below_m():
    """A pair at or beyond the capacity takes no part: tables of the last block lose some or all of their pairs."""
    from splendor_gym.search import pairs_reference, pick_pairs_reference
    n = 130
    flags, reward, value = random_pick_planes(n, 77)
    R = pairs_reference(dict(flags=flags, reward=reward, value=value))
    m = int(R["base"][-1])
    cap = m // 2
    full_a, _ = pick_pairs_reference(R["legal"], R["base"], R["flags"], R["reward"], R["value"], -1.0)
    want_a, want_q = pick_pairs_reference(R["legal"], R["base"], R["flags"], R["reward"], R["value"], -1.0, capacity=cap)
    assert (want_a != full_a).any() and (want_a[:64] == full_a[:64]).all()
    poisoned = {k: R[k].copy() for k in R}
    poisoned["value"][cap:] = np.float32(-1e30)  # sign -1: q = 1e30 would win wherever it were read
    poisoned["flags"][cap:] = sr.LEGAL
    act, best = device_pick(poisoned, -1.0, cap, n)
    assert act.tobytes() == want_a.tobytes() and best.tobytes() == want_q.tobytes()


def policy_engine(n=130):
    e = engine(n, 2)
    e.reset(seeds=list(range(5000, 5000 + n)))
    sr.random_plies(e, 30, seed=4)
    return e


def test_compact_policy_equals_the_dense_policy():
    """OnePlyValuePolicy(compact=True).act == compact=False at 130 tables with the golden checkpoint: the actions, and
    best_q bit for bit (the critic's value of a row does not depend on its place in the batch); the same with an
    initial capacity of 1, through the grow-and-reissue path."""
    import torch
    from splendor_gym.search import OnePlyValuePolicy
    fused = golden_fused()
    e = policy_engine()
    n = e.n
    q = lambda: torch.full((n,), 7.0, dtype=torch.float32, device=e.device)
    qd, qc, qg = q(), q(), q()
    dense = OnePlyValuePolicy(fused).act(e, best_q=qd).cpu().numpy().copy()
    pol = OnePlyValuePolicy(fused, compact=True)
    got = pol.act(e, best_q=qc).cpu().numpy().copy()
    again = pol.act(e).cpu().numpy().copy()
    m = pol.critic_rows
    assert n < m < 12 * n
    assert got.tobytes() == dense.tobytes() == again.tobytes()
    assert qc.cpu().numpy().tobytes() == qd.cpu().numpy().tobytes()
    assert len(set(dense[dense >= 0].tolist())) > 1
    grow = OnePlyValuePolicy(fused, compact=True, capacity=1)
    assert grow.act(e, best_q=qg).cpu().numpy().tobytes() == dense.tobytes()
    assert grow._held[1].capacity == (5 * m + 3) // 4 and grow.critic_rows == m
    assert qg.cpu().numpy().tobytes() == qd.cpu().numpy().tobytes()
    assert grow.act(e).cpu().numpy().tobytes() == dense.tobytes()  # the grown buffers, written again


def test_compact_policy_with_every_table_over(orc):
    from splendor_gym.search import OnePlyValuePolicy
    fused = golden_fused()
    e = engine(65, 2)
    e.reset(seeds=list(range(65)))
    e.upload(np.stack([over_table(orc, 2)] * 65))
    pol = OnePlyValuePolicy(fused, compact=True)

    def no_call(*a, **kw):
        raise AssertionError("the critic was called with no pair to value")
    fused.get_value = no_call
    assert pol.act(e).tolist() == [-1] * 65 and pol.critic_rows == 0


def test_checked_build():
    """Parity with the dense call and an overflowing call at 65 tables through the bounds-check build, in a child
    process (the library is chosen at load time): no invariant violation recorded."""
    assert os.path.exists(CHECKED), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, SPLENDOR_AMD_LIB=CHECKED)
    r = subprocess.run([sys.executable, os.path.join(HERE, "successor_pairs_checked_child.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["pairs"] > 65 and res["overflow_total"] == res["pairs"]
    assert res["flags"] == 0, f"invariant violations recorded: {res['flags']:#x}"
