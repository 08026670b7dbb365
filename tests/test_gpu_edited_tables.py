"""Trajectory parity on edited card and noble tables (tests/edited_tables.py): every comparison is bit for
bit against the CPU oracle evaluating the same tables (orc_set_tables), through the C-ABI.

The canonical table never makes a purchase legal on a fresh deal, ends an episode about once in 77 plies
and hardly ever asks compute_winner to break a tie or awards a noble; FREE, SUDDEN and NOBLE do those all
the time, inside spl_step and inside every rollout kernel shape.  Each run asserts on the ORACLE's side
that it reached the path it is there for (edited_tables.check_coverage; the same floors hold for the
oracle alone in tests/test_edited_tables_host.py, where the observed counts are recorded).
"""
import copy

import numpy as np
import pytest

import edited_tables as et
from oracle.oracle import Oracle, OracleVec, table_to_view, view_to_table
from schema import canon
from test_gpu_legal_cache import check_cache
from test_gpu_parity import bits_of, engine, run_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return Oracle()


# ---- spl_step chains ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,P,seed", [("FREE", 2, 2101), ("SUDDEN", 2, 2102), ("NOBLE", 2, 2103), ("SUDDEN", 3, 3102),
                                         ("FREE", 4, 4101), ("NOBLE", 4, 4103)])
def test_spl_step_chain(orc, name, P, seed):
    """1 000 tables (a partial last wave), 200 plies of the device uniform policy with injected illegal and
    out-of-range actions, the default refill period: every output of every ply, the terminal rows, the
    fused policy's next action (against its host restatement on the oracle's mask) and the table state
    four times.  On the oracle's side (test_edited_tables_host.py has the same runs): FREE 2 223 of 2 557
    fresh deals with a legal purchase at 2 players, 3 308 of 3 829 at 4; SUDDEN 27.3 ends per table, 6.1 %
    of them ties at 2 players, 20.8 and 10.0 % at 3; NOBLE 9.07 awards per table at 2 players."""
    cards, nobles = et.TABLES[name]()
    seen = []

    def watch(vec):
        seen.append(et.Coverage(vec))
        return seen[0]

    with et.oracle_tables(orc, cards, nobles):
        run_parity(orc, P, 1000, 200, None, seed, True, check_state_every=50, cards=cards, nobles=nobles, watch=watch,
                   host_policy=et.host_uniform)
    et.check_coverage(name, P, seen[0], 200)


# ---- every rollout kernel shape against the oracle --------------------------------------------------------
ROLL_N, ROLL_K, ROLL_LAUNCHES, ROLL_ENV_SEED, ROLL_SEED = 1000, 48, 2, 5, 3
_roll_refs = {}


def roll_reference(orc, name, P):
    """The oracle's replay of ROLL_LAUNCHES x ROLL_K steps on table `name`, computed once per (name, P)
    and shared by the kernel shapes: the actions are recorded by a twin engine's spl_step chain (each
    step takes the previous step's next_actions), the oracle replays them."""
    import torch
    key = (name, P)
    if key in _roll_refs:
        return _roll_refs[key]
    cards, nobles = et.TABLES[name]()
    n, steps = ROLL_N, ROLL_K * ROLL_LAUNCHES
    seeds = [ROLL_ENV_SEED + i for i in range(n)]
    twin = engine(n, P, refill_period=16, cards=cards, nobles=nobles)
    twin.reset(seeds=seeds)
    ta = torch.zeros(n, dtype=torch.int32, device=twin.device)
    twin.sample_uniform(out=ta, seed=ROLL_SEED, ply=0)
    acts = torch.empty((steps, n), dtype=torch.int32, device=twin.device)
    for k in range(steps):
        acts[k] = ta
        na = torch.empty_like(ta)
        twin.step(ta, next_actions=na, policy_seed=ROLL_SEED, ply=1 + k)
        ta = na
    A = acts.cpu().numpy()
    with et.oracle_tables(orc, cards, nobles):
        vec = OracleVec(orc, n, P, seeds)
        cov = et.Coverage(vec, window=16)
        refs = []
        for k in range(steps):
            refs.append(vec.step(A[k], want_final=True))
            cov.update(refs[-1])
        tables = [canon(vec.table(t)) for t in range(n)]
    c = et.check_coverage(name, P, cov, steps)
    if name == "SUDDEN" and P == 2:
        assert c["max_in_window"] > 3, c  # some table spent its pool of three deals inside a refill period
    _roll_refs[key] = dict(first=A[0].copy(), last=ta.cpu().numpy(), refs=refs, tables=tables)
    return _roll_refs[key]


@pytest.mark.parametrize("P,name,pipeline", [(2, "SUDDEN", False), (2, "SUDDEN", "always"), (2, "SUDDEN", "half"),
                                             (2, "SUDDEN", "dealer"), (2, "SUDDEN", "dealer2"), (2, "SUDDEN", "quad"),
                                             (2, "FREE", "quad"), (2, "FREE", "dealer"), (3, "SUDDEN", "dealer"),
                                             (4, "FREE", "dealer2"), (4, "FREE", "quad")])
def test_rollout_shapes_against_the_oracle(orc, P, name, pipeline):
    """Two 48-step launches into a per-step store, refill period 16, 1 000 tables: obs, mask, reward,
    terminated, flags, winner and the terminal final_obs rows of every step, the next action after each
    launch and every table's downloaded state at the end equal the oracle's replay.  (Against the oracle,
    not a step chain: both sides of a chain comparison share autoreset_table.)  On the oracle's side:
    SUDDEN 13.2 ends per table at 2 players, up to 4 resets of one table inside one refill period (the
    pool is spent), 10.0 at 3 players; FREE 894 of 1 027 fresh deals with a legal purchase at 2 players,
    1 462 of 1 698 at 4."""
    import torch
    ref = roll_reference(orc, name, P)
    cards, nobles = et.TABLES[name]()
    n, K = ROLL_N, ROLL_K
    e = engine(n, P, refill_period=16, pipeline=pipeline, cards=cards, nobles=nobles)
    e.reset(seeds=[ROLL_ENV_SEED + i for i in range(n)])
    dev = e.device
    a = torch.from_numpy(ref["first"]).to(dev)
    out = {"obs": torch.empty((K, n, 297), dtype=torch.int32, device=dev),
           "mask": torch.empty((K, n, 45), dtype=torch.int8, device=dev),
           "reward": torch.empty((K, n), dtype=torch.float32, device=dev),
           "terminated": torch.empty((K, n), dtype=torch.uint8, device=dev),
           "flags": torch.empty((K, n), dtype=torch.uint8, device=dev),
           "winner": torch.empty((K, n), dtype=torch.int8, device=dev),
           "final_obs": torch.zeros((K, n, 297), dtype=torch.int32, device=dev)}
    for launch in range(ROLL_LAUNCHES):
        na = torch.empty_like(a)
        e.rollout(K, actions=a, next_actions=na, policy_seed=ROLL_SEED, ply=1 + launch * K, out=out)
        a = na
        got = {k: v.cpu().numpy() for k, v in out.items()}
        masks = bits_of(got["mask"])
        for k in range(K):
            r = ref["refs"][launch * K + k]
            where = f"{pipeline} launch {launch} step {k}"
            np.testing.assert_array_equal(got["flags"][k], r["flags"], err_msg=where + " flags")
            np.testing.assert_array_equal(masks[k], r["mask"], err_msg=where + " mask")
            np.testing.assert_array_equal(got["obs"][k], r["obs"], err_msg=where + " obs")
            np.testing.assert_array_equal(got["reward"][k], r["reward"], err_msg=where + " reward")
            np.testing.assert_array_equal(got["terminated"][k], r["terminated"], err_msg=where + " terminated")
            np.testing.assert_array_equal(got["winner"][k], r["winner"], err_msg=where + " winner")
            rows = np.flatnonzero(r["terminated"])
            np.testing.assert_array_equal(got["final_obs"][k][rows], r["final_obs"][rows], err_msg=where + " final")
    np.testing.assert_array_equal(a.cpu().numpy(), ref["last"])
    recs = e.download()
    for t in range(n):
        assert canon(table_to_view(recs[t])) == ref["tables"][t], (pipeline, t)


# ---- a free card on a fresh deal (the constant fresh-deal mask does not hold) -----------------------------
@pytest.mark.parametrize("step_tail", [0, 1, 2])
def test_fresh_deal_with_a_free_card(orc, step_tail):
    """FREE, autoreset on, each spl_step shape: tables crafted one move from their end (the last player of
    the round to move, a player at 15 prestige) are stepped until SPL_F_RESET shows.  That step's mask is
    spl_legal of the new deal (and the oracle's), the cache entry too, and the fused policy drew from it;
    the next spl_step, buying a free visible card wherever there is one, is not flagged SPL_F_ILLEGAL and
    equals Oracle.env_step in every output and in the resulting state."""
    import torch
    cards, nobles = et.free_tables()
    n, seed = 256, 17
    e = engine(n, 2, cards=cards, nobles=nobles, step_tail=step_tail)
    e.reset(seeds=range(900, 900 + n))
    recs = e.download()
    recs["to_play"] = 1
    recs["move_count"] = 1
    recs["players"]["prestige"][:, 1] = 15
    e.upload(recs)
    nxt = torch.zeros(n, dtype=torch.int32, device=e.device)
    reset = np.zeros(n, bool)
    for k in range(4):
        acts = e.legal(out=torch.empty((n, 45), dtype=torch.int8, device=e.device)).to(torch.int32).argmax(dim=1)
        e.step(acts.to(torch.int32), next_actions=nxt, policy_seed=seed, ply=k + 1)
        reset = (e.flags.cpu().numpy() & et.F_RESET) != 0
        if reset.any():
            break
    assert k == 0 and reset.all()  # the crafted move ends every game
    mask = bits_of(e.mask.cpu().numpy())
    legal = bits_of(e.legal(out=torch.empty((n, 45), dtype=torch.int8, device=e.device)).cpu().numpy())
    bad = np.flatnonzero(mask != legal)
    assert bad.size == 0, (bad[:8], [hex(int(x)) for x in (mask[bad[:4]] ^ legal[bad[:4]])])
    check_cache(e, "autoreset under FREE")
    views = [table_to_view(r) for r in e.download()]
    with et.oracle_tables(orc, cards, nobles):
        ref_mask = np.array([orc.legal(v) for v in views], np.uint64)
        np.testing.assert_array_equal(mask, ref_mask)
        np.testing.assert_array_equal(nxt.cpu().numpy(), et.host_uniform(ref_mask, seed, 1))
        free = (ref_mask & et.BUY_VISIBLE) != 0
        assert 2 * int(free.sum()) >= n, int(free.sum())  # a free card is visible on most deals
        low = lambda m: (int(m) & -int(m)).bit_length() - 1
        acts = np.array([low(m & et.BUY_VISIBLE) if f else low(m) for m, f in zip(ref_mask, free)], np.int32)
        e.step(torch.from_numpy(acts).to(e.device))
        flags = e.flags.cpu().numpy()
        assert not (flags & et.F_ILLEGAL).any(), np.flatnonzero(flags & et.F_ILLEGAL)[:8]
        obs, m2 = e.obs.cpu().numpy(), bits_of(e.mask.cpu().numpy())
        rew, term = e.reward.cpu().numpy(), e.terminated.cpu().numpy()
        after = e.download()
        for i in range(n):
            ref = orc.env_step(views[i], int(acts[i]))
            assert not ref["error"] and not ref["terminated"], i
            np.testing.assert_array_equal(obs[i], ref["obs"], err_msg=str(i))
            assert int(m2[i]) == ref["mask"] and rew[i] == np.float32(ref["reward"]) and term[i] == 0, i
            assert int(flags[i]) == ref["flags"], i
            assert canon(table_to_view(after[i])) == canon(ref["after"]), i


# ---- the legal-mask cache ---------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["always", "dealer2", "quad"])
@pytest.mark.parametrize("name", ["FREE", "SUDDEN"])
def test_legal_mask_cache_under_edited_tables(name, pipeline):
    """After reset, after 40 spl_step calls and after one rollout(32) of each rollout family, the cache equals
    spl_legal of every stored state under the context's own tag (test_gpu_legal_cache.check_cache)."""
    import torch
    cards, nobles = et.TABLES[name]()
    n, seed = 1024, 5
    e = engine(n, 2, refill_period=16, pipeline=pipeline, cards=cards, nobles=nobles)
    e.reset(seeds=range(n))
    tag = check_cache(e, "reset(seed)")
    a = torch.zeros(n, dtype=torch.int32, device=e.device)
    e.sample_uniform(out=a, seed=seed, ply=0)
    for k in range(40):
        na = torch.empty_like(a)
        e.step(a, next_actions=na, policy_seed=seed, ply=1 + k)
        a = na
    assert check_cache(e, "step") == tag
    na = torch.empty_like(a)
    e.rollout(32, actions=a, next_actions=na, policy_seed=seed, ply=100)
    assert check_cache(e, f"rollout {pipeline}") == tag


# ---- the fused scripted policies ------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("name", ["SUDDEN", "FREE"])
def test_device_scripted_policies_under_edited_tables(name, policy):
    """test_gpu_parity.test_device_scripted_policies on SUDDEN and FREE (1 024 tables, 40 plies with
    autoreset): SPL_POLICY_GREEDY_V1 equals the host greedy_opponent_v1 on the device's own obs / mask, every
    SPL_POLICY_BASIC_PRIORITY choice lies in the reference's preferred set.  Both host functions read only
    the observation, so they hold for any table; the reset rows' masks are the ones the policy drew from."""
    import torch
    from splendor_gym.opponents import greedy_opponent_v1
    cards, nobles = et.TABLES[name]()
    n = 1024
    e = engine(n, 2, cards=cards, nobles=nobles)
    e.reset(seeds=range(100, 100 + n))
    a = torch.zeros(n, dtype=torch.int32, device=e.device)
    nxt = torch.zeros_like(a)
    e.sample_uniform(out=a, seed=9, ply=0)
    resets = bought = 0
    for k in range(40):
        e.step(a, next_actions=nxt, policy=policy, policy_seed=9, ply=k + 1)
        obs, mask, got = e.obs.cpu().numpy(), e.mask.cpu().numpy(), nxt.cpu().numpy()
        fresh = (e.flags.cpu().numpy() & et.F_RESET) != 0
        resets += int(fresh.sum())
        bought += int((fresh & (got >= 15) & (got <= 26)).sum())
        rows = np.union1d(np.arange(0, n, 7), np.flatnonzero(fresh))  # every reset row and a sample of the rest
        for i in rows:
            info = {"action_mask": mask[i]}
            legal = np.flatnonzero(mask[i])
            if policy == 1:
                assert got[i] == greedy_opponent_v1(obs[i], info), (k, i)
                continue
            if len(legal) == 0:
                assert got[i] == 0
                continue
            vis = legal[(legal >= 15) & (legal <= 26)]
            if len(vis):
                pts = np.array([obs[i][32 + (x - 15) * 13 + 2] for x in vis])
                allowed = vis[pts == pts.max()]
            else:
                allowed = next(legal[(legal >= lo) & (legal <= hi)] for lo, hi in ((42, 44), (0, 9), (10, 14), (27, 41), (0, 44))
                               if len(legal[(legal >= lo) & (legal <= hi)]))
            assert got[i] in allowed, (k, i, got[i], allowed)
        e.sample_uniform(out=a, seed=11, ply=k)  # keep the tables moving with uniform play
    assert resets > 0
    if name == "FREE":
        assert bought > 0  # both scripts prefer a purchase: on a fresh deal only a free card offers one


# ---- prestige near the top of its byte ------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 4])
def test_prestige_near_the_top_of_the_byte(orc, P):
    """Card points 120 (ids divisible by 3) and noble points 100: movers holding 14 prestige buy a 120-point
    tier-1 card, with tokens (134 afterwards) or with bonuses that also earn a noble (234 = 14 + 120 + 100,
    the most the PRESTIGE pair can reach and spl_ctx_create's bound for it); one step without autoreset,
    outputs and state against Oracle.env_step, for every seat."""
    import torch
    cards, nobles = et.prestige_tables()
    views, acts, want = [], [], []
    with et.oracle_tables(orc, cards, nobles):
        for seed in range(40):
            v = orc.initial_state(P, 5000 + seed)
            slots = [k for k, c in enumerate(v["board"]) if c >= 0 and c % 3 == 0 and cards[c, 0] == 1]
            if not slots:
                continue
            k = slots[0]
            cost = [int(x) for x in cards[v["board"][k], 3:8]]
            for tp in range(P):
                for noble in (False, True):
                    w = copy.deepcopy(v)
                    w["to_play"], w["move_count"] = tp, tp
                    pl = w["players"][tp]
                    pl["prestige"] = 14
                    if noble:
                        pl["bonuses"] = [4, 4, 4, 4, 4]
                    else:
                        pl["tokens"] = cost + [0]
                        w["bank"] = [b - c for b, c in zip(w["bank"][:5], cost)] + [w["bank"][5]]
                        assert min(w["bank"]) >= 0
                    views.append(w)
                    acts.append(15 + k)
                    want.append(234 if noble else 134)
            if len(views) >= 16 * P:
                break
        n = len(views)
        assert n >= 16 * P
        e = engine(n, P, cards=cards, nobles=nobles)
        e.reset(seeds=range(n))
        e.upload(np.stack([view_to_table(v) for v in views]))
        e.step(torch.tensor(acts, dtype=torch.int32, device=e.device), autoreset=False)
        flags, obs, mask = e.flags.cpu().numpy(), e.obs.cpu().numpy(), bits_of(e.mask.cpu().numpy())
        rew, term, win = e.reward.cpu().numpy(), e.terminated.cpu().numpy(), e.winner.cpu().numpy()
        after = e.download()
        for i, v in enumerate(views):
            ref = orc.env_step(v, acts[i])
            assert not ref["error"] and not ref["flags"] & et.F_ILLEGAL, i
            assert ref["after"]["players"][v["to_play"]]["prestige"] == want[i], (i, want[i])  # the case is what it says
            assert canon(table_to_view(after[i])) == canon(ref["after"]), i
            np.testing.assert_array_equal(obs[i], ref["obs"], err_msg=str(i))
            assert int(mask[i]) == ref["mask"] and rew[i] == np.float32(ref["reward"]), i
            assert term[i] == ref["terminated"] and int(flags[i]) == ref["flags"], i
            assert int(win[i]) == ref["after"]["winner"], i
