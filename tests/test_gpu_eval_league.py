"""The on-device evaluation league (include/splendor_eval.h, splendor_gym.evaluation.DeviceEvaluator):
the scripted kernel against the step kernel's fused policies and the host greedy_v2, the league against
the existing batched evaluator group by group, greedy_v2 against the reference fixture, graph replay
against eager launches, and the trainer's flags."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, STEPS, SEED = 777, 40, 9  # 777: a partial last wave

INT_KEYS = ("n", "wins", "losses", "draws", "unfinished")
FLOAT_KEYS = ("win_rate", "win_rate_ci95", "avg_turns", "avg_prestige", "illegal_action_rate")


def same_stats(got, want, keys_int=INT_KEYS):
    for k in keys_int:
        assert got[k] == want[k], (k, got, want)
    for k in FLOAT_KEYS:
        assert got[k] == pytest.approx(want[k], abs=1e-12), (k, got, want)


def scripted(obs, mask, **kw):
    from splendor_gym.opponents import ScriptedOpponents
    return ScriptedOpponents(**kw)(obs, mask)


def compact(obs):
    import torch
    from splendor_gym.selfplay import compact_rows
    return compact_rows(obs, torch.zeros(obs.shape[0], 300, dtype=torch.uint8, device=obs.device))


# ---------------------------------------------------------------------------------------------
# (a) the observation-fed policies against the step kernel's state-fed ones
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [0, 1, 2])
def test_scripted_kernel_equals_fused_policies(policy):
    """After every step of 40 plies of uniform play the scripted kernel, on the step's own obs / mask
    with the same seed, ply and table keys, answers exactly what policy_action answered inside the step
    kernel — from int32 rows, from compact rows, and with the ply split into ply = 1 + a device base.
    Both run the cascades of csrc/spl_scripted.h: this pins the kernel that feeds them from the observation
    to the one that feeds them from the table's state."""
    import torch
    from splendor_gym.device import Engine
    names = {0: "random", 1: "greedy_v1", 2: "basic_priority"}
    e = Engine(N, 2, device="cuda:0")
    e.reset(seeds=list(range(100, 100 + N)))
    a = torch.zeros(N, dtype=torch.int32, device=e.device)
    nxt = torch.zeros(N, dtype=torch.int32, device=e.device)
    base = torch.zeros(1, dtype=torch.int64, device=e.device)
    for k in range(STEPS):
        e.sample_uniform(out=a, seed=3, ply=k)
        e.step(a, next_actions=nxt, policy=policy, policy_seed=SEED, ply=k + 1)
        got = scripted(e.obs, e.mask, name=names[policy], seed=SEED, ply=k + 1)
        assert torch.equal(got, nxt), (k, (got != nxt).nonzero()[:5].tolist())
        got = scripted(compact(e.obs), e.mask, name=names[policy], seed=SEED, ply=k + 1)
        assert torch.equal(got, nxt), ("u8", k)
        base.fill_(k)
        got = scripted(e.obs, e.mask, name=names[policy], seed=SEED, ply=1, ply_base=base)
        assert torch.equal(got, nxt), ("ply_base", k)
    e.close()


def test_scripted_kernel_empty_mask_and_table_key():
    """No legal action: every policy answers 0, as policy_action does.  table_key replaces table0 + t."""
    import torch
    from splendor_gym.device import Engine
    e = Engine(130, 2, device="cuda:0")
    obs, mask = e.reset(seeds=list(range(130)))
    empty = torch.zeros_like(mask)
    for name in ("random", "greedy_v1", "basic_priority", "greedy_v2"):
        out = torch.full((130,), -7, dtype=torch.int32, device=e.device)
        scripted(obs, empty, name=name, seed=SEED, out=out)
        assert (out == 0).all(), name
    key = torch.arange(130, dtype=torch.int64, device=e.device) + 5
    for name in ("random", "basic_priority"):
        assert torch.equal(scripted(obs, mask, name=name, seed=SEED, ply=4, table_key=key),
                           scripted(obs, mask, name=name, seed=SEED, ply=4, table0=5))
    assert not torch.equal(scripted(obs, mask, name="random", seed=SEED, ply=4, table_key=key),
                           scripted(obs, mask, name="random", seed=SEED, ply=4))
    e.close()


# ---------------------------------------------------------------------------------------------
# (b) greedy_v2 against the host callable
# ---------------------------------------------------------------------------------------------
class _Bank:
    """env_ref stand-in of greedy_opponent_v2_factory: state.bank read from an observation."""
    class _S:
        bank = None

    def __init__(self):
        self.state = self._S()


def host_v2(obs, mask):
    from splendor_gym.scripts.eval_suite import greedy_opponent_v2_factory
    ref = _Bank()
    policy = greedy_opponent_v2_factory(ref)
    out = np.zeros(len(obs), np.int32)
    for i in range(len(obs)):
        ref.state.bank = [int(x) for x in obs[i, :5]]
        out[i] = policy(obs[i], {"action_mask": mask[i]})
    return out


def branch_of(mask, action):
    m = np.flatnonzero(mask)
    if len(m) == 0:
        return "empty"
    if ((m >= 15) & (m <= 26)).any() or (m >= 42).any():
        return "buy"
    if ((m >= 10) & (m <= 14)).any():
        return "take2" if ((m >= 10) & (m <= 14)).sum() > 1 else "take2_single"
    if (m <= 9).any():
        return "take3" if (m <= 9).sum() > 1 else "take3_single"
    return "reserve"


def crafted_rows():
    """(obs, mask) rows that reach every branch whatever natural play does: bank counts in obs[0:5]."""
    rows = [([4, 5, 3, 3, 2], [10, 12, 13, 1, 4]),       # take-2: colours 2 and 3 tie at 3 -> the first, 12
            ([0, 7, 7, 7, 7], [11, 14]),                 # take-2: the scarcest colour is not legal; 11 ties 14 -> 11
            ([5, 1, 5, 1, 0], [13, 14, 10]),             # take-2: minimum at the last colour, 14
            ([4, 5, 3, 3, 2], [1, 4, 7, 9]),             # take-3: sums 12, 9, 10, 8 -> 9
            ([2, 2, 2, 2, 2], [3, 5, 8]),                # take-3: all tie -> the first, 3
            ([7, 0, 7, 0, 7], [0, 2, 6, 4]),             # take-3: combos (0,1,2) 14, (0,1,4) 14, (1,2,3) 7, (0,2,4) 21 -> 6
            ([1, 1, 1, 1, 1], [27, 33, 41]),             # highest reserve: 41
            ([1, 1, 1, 1, 1], [28, 30]),                 # highest reserve: 30
            ([1, 1, 1, 1, 1], []),                       # empty: 0
            ([1, 1, 1, 1, 1], [20, 43, 5, 11, 30]),      # visible buy first
            ([1, 1, 1, 1, 1], [43, 44, 3, 12, 29])]      # reserved buy when no visible one
    obs = np.zeros((len(rows), 297), np.int32)
    mask = np.zeros((len(rows), 45), np.int8)
    for i, (bank, legal) in enumerate(rows):
        obs[i, :5] = bank
        mask[i, legal] = 1
    return obs, mask


def test_greedy_v2_equals_host_callable():
    import torch
    from splendor_gym.device import Engine
    e = Engine(N, 2, device="cuda:0")
    e.reset(seeds=list(range(500, 500 + N)))
    a = torch.zeros(N, dtype=torch.int32, device=e.device)
    seen = set()
    for k in range(STEPS):
        e.sample_uniform(out=a, seed=4, ply=k)
        e.step(a)
        got = scripted(e.obs, e.mask, name="greedy_v2").cpu().numpy()
        got8 = scripted(compact(e.obs), e.mask, name="greedy_v2").cpu().numpy()
        obs, mask = e.obs.cpu().numpy(), e.mask.cpu().numpy()
        want = host_v2(obs, mask)
        assert np.array_equal(got, want), (k, np.flatnonzero(got != want)[:5])
        assert np.array_equal(got8, want), ("u8", k)
        seen |= {branch_of(mask[i], want[i]) for i in range(N)}
    obs, mask = crafted_rows()
    want = host_v2(obs, mask)
    assert want.tolist() == [12, 11, 14, 9, 3, 6, 41, 30, 0, 20, 43]
    dobs, dmask = torch.from_numpy(obs).to(e.device), torch.from_numpy(mask).to(e.device)
    assert scripted(dobs, dmask, name="greedy_v2").cpu().numpy().tolist() == want.tolist()
    assert scripted(compact(dobs), dmask, name="greedy_v2").cpu().numpy().tolist() == want.tolist()
    seen |= {branch_of(mask[i], want[i]) for i in range(len(want))}
    assert {"buy", "take2", "take3", "reserve", "empty"} <= seen, seen
    e.close()


def test_mixed_policy_of_keep_and_unknown_id():
    """All five ids striped across the lanes of one wave (and a partial second one): each row equals its
    policy's scalar run, SPL_EVAL_KEEP rows keep the sentinel, an unknown id is counted and left alone."""
    import torch
    from splendor_gym import _native
    from splendor_gym.device import Engine
    from splendor_gym.opponents import ScriptedOpponents
    n = 100
    e = Engine(n, 2, device="cuda:0")
    a = torch.zeros(n, dtype=torch.int32, device=e.device)
    e.reset(seeds=list(range(n)))
    for k in range(12):  # a few plies in, so that buys and differing banks exist
        e.sample_uniform(out=a, seed=4, ply=k)
        e.step(a)
    obs, mask = e.obs, e.mask
    ids = [0, 1, 2, 3, _native.EVAL_KEEP]
    names = {0: "random", 1: "greedy_v1", 2: "basic_priority", 3: "greedy_v2"}
    policy_of = torch.tensor([ids[t % 5] for t in range(n)], dtype=torch.int32, device=e.device)
    policy_of[37], policy_of[99] = 9, -2  # unknown
    out = torch.full((n,), -7, dtype=torch.int32, device=e.device)
    opp = ScriptedOpponents(policy_of=policy_of, seed=SEED, ply=6)
    assert opp(obs, mask, out=out) is out
    alone = {p: scripted(obs, mask, name=names[p], seed=SEED, ply=6).cpu().numpy() for p in names}
    got, pol = out.cpu().numpy(), policy_of.cpu().numpy()
    for t in range(n):
        if pol[t] in names:
            assert got[t] == alone[pol[t]][t], (t, pol[t])
        else:
            assert got[t] == -7, (t, pol[t])
    assert int(opp.errors) == 2
    e.close()


# ---------------------------------------------------------------------------------------------
# (c) the league against eval_vs_opponent, group by group
# ---------------------------------------------------------------------------------------------
def trained_fused():
    import torch  # noqa: F401
    from safetensors.torch import load_file
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.policy import ActorCritic
    m = ActorCritic().to("cuda:0").eval()
    m.load_state_dict(load_file(os.path.join(GOLD, "ppo_splendor_latest.safetensors"), device="cuda:0"))
    return FusedActorCritic(m)


def always_zero(obs, mask):
    import torch
    return torch.zeros(obs.shape[0], dtype=torch.int32, device=obs.device)


def league_agent(kind):
    from splendor_gym.evaluation import first_legal_policy, last_legal_policy
    if kind == "fused":
        f = trained_fused()
        return f, (lambda obs, mask: f.greedy(obs, mask)), f.opponent()
    fn = {"first_legal": first_legal_policy, "last_legal": last_legal_policy, "zero": always_zero}[kind]
    return fn, fn, fn


LEAGUE = ("random", "greedy_v1", "basic", "self_play")


def check_league(kind, n_games, seed, max_turns, graph=True):
    from splendor_gym.evaluation import DeviceEvaluator, eval_vs_opponent
    agent, policy, self_opp = league_agent(kind)
    ev = DeviceEvaluator(n_games=n_games, opponents=LEAGUE, device="cuda:0", graph=graph)
    got = ev.run(agent, seed=seed, max_turns=max_turns)
    ev.close()
    assert tuple(got) == LEAGUE
    for g, name in enumerate(LEAGUE):
        opp = {"random": "random", "greedy_v1": "greedy_v1", "basic": "basic_priority", "self_play": self_opp}[name]
        want = eval_vs_opponent(policy, opponent=opp, n_games=n_games, seed=seed + g, device="cuda:0",
                                max_turns=max_turns)
        assert set(got[name]) == set(want)
        print(kind, name, got[name])
        same_stats(got[name], want)
    return got


@pytest.mark.parametrize("kind,max_turns", [("first_legal", 1000), ("last_legal", 1000), ("fused", 1000), ("zero", 30)])
def test_league_equals_eval_vs_opponent(kind, max_turns):
    """37 games per group (group borders inside waves): every key of every group equals the existing
    evaluator's for that opponent alone, with seed + g."""
    got = check_league(kind, 37, 11, max_turns)
    if kind == "zero":  # the agent stalls on an illegal action: the turn budget ends the run
        assert any(r["unfinished"] > 0 for r in got.values()) and any(r["illegal_action_rate"] > 0 for r in got.values())
    else:
        assert all(r["unfinished"] == 0 for r in got.values())


def test_league_of_one_game():
    check_league("last_legal", 1, 5, 1000)


# ---------------------------------------------------------------------------------------------
# (d) greedy_v2 against the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4))
def test_greedy_v2_reproduces_the_reference(case):
    from splendor_gym.evaluation import DeviceEvaluator, eval_vs_opponent, first_legal_policy, last_legal_policy
    with open(os.path.join(GOLD, "eval_v2.json")) as f:
        c = json.load(f)[case]
    agent = {"first_legal": first_legal_policy, "last_legal": last_legal_policy}[c["agent"]]
    ev = DeviceEvaluator(n_games=c["n_games"], opponents=("greedy_v2",), device="cuda:0")
    league = ev.run(agent, seed=c["seed"])["greedy_v2"]
    ev.close()
    single = eval_vs_opponent(agent, opponent="greedy_v2", n_games=c["n_games"], seed=c["seed"], device="cuda:0")
    for got in (league, single):
        same_stats(got, c["result"], keys_int=("n", "wins", "losses", "draws"))
        assert got["unfinished"] == 0


# ---------------------------------------------------------------------------------------------
# (e) graph replay against eager launches
# ---------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    from splendor_gym.evaluation import DeviceEvaluator
    agent = trained_fused()
    replayed = DeviceEvaluator(n_games=65, device="cuda:0", graph=True, chunk=8)
    eager = DeviceEvaluator(n_games=65, device="cuda:0", graph=False, chunk=8)
    a, b = replayed.run(agent, seed=2), eager.run(agent, seed=2)
    assert replayed.replays > 0 and eager.replays == 0
    assert a == b, (a, b)
    assert all(r["unfinished"] == 0 for r in a.values())
    # a second run replays from the first chunk on: no stale ply, seed or playing state
    before = replayed.replays
    c = replayed.run(agent, seed=31)
    assert replayed.replays > before
    eager.close()
    fresh = DeviceEvaluator(n_games=65, device="cuda:0", graph=False, chunk=8)
    d = fresh.run(agent, seed=31)
    assert c == d, (c, d)
    assert c != a
    replayed.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------
# (f) the trainer's flags
# ---------------------------------------------------------------------------------------------
def test_trainer_eval_flags(capsys):
    from splendor_gym.scripts import ppo_device
    base = ["--num-envs", "256", "--num-steps", "8", "--total-timesteps", "4096"]
    ppo_device.main(base + ["--eval-every-updates", "1", "--eval-games", "16"])
    lines = capsys.readouterr().out.splitlines()
    heads = [i for i, ln in enumerate(lines) if ln.startswith("evaluation at step ")]
    updates = [i for i, ln in enumerate(lines) if ln.startswith("update ")]
    assert len(updates) == 2 and len(heads) == 3
    assert heads[0] < updates[0] < heads[1] < updates[1] < heads[2]  # before update 1, then after each
    for h in heads:
        block = lines[h + 1:h + 6]
        assert [ln.split(":")[0].strip() for ln in block] == [f"eval vs {o}" for o in
                                                              ("random", "greedy_v1", "basic", "self_play", "greedy_v2")]
        for ln in block:
            for word in ("win_rate", "+-", "avg_turns", "avg_prestige", "illegal_action_rate"):
                assert word in ln, ln
    ppo_device.main(base)
    out = capsys.readouterr().out
    assert "eval" not in out and len([ln for ln in out.splitlines() if ln.startswith("update ")]) == 2
