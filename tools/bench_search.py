"""Timings of the one-ply search primitives (include/splendor_search.h) on one MI355X.

    python tools/bench_search.py [--tables 65536 1600] [--repeats 15] [--games 400] [--out profiles/search/bench_search.json]
    python tools/bench_search.py --ab plain=<lib> nt=<lib> ... [--rounds 5]      (row store policy / LDS shape A/B)
    python tools/bench_search.py --part pairs [--tables ...] [--out profiles/search/bench_search_pairs.json]
                                     (the legal pairs only: spl_successors_pairs and the compact decision against the dense ones)

HIP events around each arm on one stream, the arms alternating, medians over `repeats`; two untimed calls of
every arm first.
  (a) spl_successors, compact rows only, against the only way to get the same rows without it: per action a
      copy of the arena buffer, then spl_step with that constant action, autoreset off, compact-only outputs,
      45 times (`step_chain`; `equal` records that the rows of the legal pairs are the same bytes)
  (b) the call's output bytes / time beside the store rate of the headline rollout
  (c) OnePlyValuePolicy.act as a whole and split into its three calls, and the share of legal pairs
  (d) evaluation.eval_vs_opponent at `games` games against greedy_v1 and basic_priority: the golden
      checkpoint's greedy actor, and the one-ply policy over the same checkpoint's critic
--ab: one child process per library and round (SPLENDOR_AMD_LIB), alternating, each timing successors + critic
at 65 536 tables; medians per library.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "splendor-gym_amd")]

HEADLINE_STORE_TBS = 5.6  # the store rate the headline rollout reaches


def timed(torch, arms, repeats, warmup=2):
    """{name: [ms per call]}: every arm once per round, in turn, each between two events."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    return ms


def stats(v):
    return {"median_us": round(1e3 * statistics.median(v), 2), "min_us": round(1e3 * min(v), 2),
            "max_us": round(1e3 * max(v), 2)}


def golden_fused(torch, dev):
    from safetensors.torch import load_file
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.policy import ActorCritic
    model = ActorCritic().to(dev).eval()
    model.load_state_dict(load_file(os.path.join(REPO, "tests", "golden", "ppo_splendor_latest.safetensors"), device=str(dev)))
    return FusedActorCritic(model)


def midgame(Engine, torch, n, dev, plies=30):
    e = Engine(n, 2, device=dev)
    e.reset(seeds=list(range(n)))
    na = torch.zeros(n, dtype=torch.int32, device=dev)
    e.sample_uniform(out=na, seed=1, ply=0)
    for k in range(plies):
        e.step(na.clone(), next_actions=na, policy_seed=1, ply=k + 1)
    return e


def pair_only(args):
    """--part pair: successors + critic at 65 536 tables with the loaded library; one JSON line."""
    import torch
    from splendor_gym.device import Engine
    dev = torch.device("cuda:0")
    n = 65536
    fused = golden_fused(torch, dev)
    e = midgame(Engine, torch, n, dev)
    s = e.successors(mask_bits=False)
    rows = s.obs_u8.view(45 * n, 300)
    value = torch.empty(45 * n, 1, dtype=torch.float32, device=dev)
    ms = timed(torch, {"successors": lambda: e.successors(mask_bits=False, out=s),
                       "critic": lambda: fused.get_value(rows, out=value),
                       "pair": lambda: (e.successors(mask_bits=False, out=s), fused.get_value(rows, out=value))},
               args.repeats)
    print(json.dumps({k: stats(v) for k, v in ms.items()}))


def pairs_part(args):
    """--part pairs: the ragged form against the dense one, same protocol: the pairs call against the dense call, and
    the compact decision against the dense decision with its split (successors / read-back / critic / pick)."""
    import torch
    from splendor_gym.device import Engine
    from splendor_gym.search import OnePlyValuePolicy, pick, pick_pairs

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    fused = golden_fused(torch, dev)
    sizes = {}
    for n in args.tables:
        e = midgame(Engine, torch, n, dev)
        s = e.successors(mask_bits=False)
        p = e.successor_pairs()
        m = p.total()
        assert m <= p.capacity
        rows = s.obs_u8.view(45 * n, 300)
        value = torch.empty(45 * n, 1, dtype=torch.float32, device=dev)
        value_m = torch.empty(p.capacity, 1, dtype=torch.float32, device=dev)
        action = torch.empty(n, dtype=torch.int32, device=dev)
        dense, compact = OnePlyValuePolicy(fused), OnePlyValuePolicy(fused, compact=True)
        arms = {"successors": lambda: e.successors(mask_bits=False, out=s),
                "successor_pairs": lambda: e.successor_pairs(out=p),
                "critic_45n": lambda: fused.get_value(rows, out=value),
                "critic_m": lambda: fused.get_value(p.obs_u8[:m], out=value_m[:m]),
                "pick": lambda: pick(s.flags, s.reward, value, -1.0, out=action),
                "pick_pairs": lambda: pick_pairs(p.legal, p.base, p.flags, p.reward, value_m, -1.0, capacity=m, out=action),
                "read_back": lambda: p.total(),
                "act_dense": lambda: dense.act(e),
                "act_compact": lambda: compact.act(e)}
        ms = timed(torch, arms, args.repeats)
        med = {k: statistics.median(v) for k, v in ms.items()}
        same = bool(torch.equal(dense.act(e).clone(), compact.act(e)))
        sizes[str(n)] = {
            "us": {k: stats(v) for k, v in ms.items()},
            "legal_pairs_m": m, "legal_share_of_pairs": round(m / (45 * n), 4),
            "ratio_successors_over_pairs": round(med["successors"] / med["successor_pairs"], 2),
            "ratio_act_dense_over_compact": round(med["act_dense"] / med["act_compact"], 2),
            "act_compact_share": {k: round(med[k] / med["act_compact"], 3)
                                  for k in ("successor_pairs", "read_back", "critic_m", "pick_pairs")},
            "act_dense_share": {k: round(med[k] / med["act_dense"], 3) for k in ("successors", "critic_45n", "pick")},
            "pairs_output_bytes": m * (300 + 1 + 4 + 4) + 8 * n, "dense_output_bytes": 45 * n * (300 + 1 + 4),
            "equal_actions": same}
        e.close()
        del s, p, rows, value, value_m, dense, compact
        torch.cuda.empty_cache()
    line = json.dumps({"metric": "one-ply search over the legal pairs only against the dense form, 2 players, mid-game tables, "
                                 "one MI355X",
                       "timing": f"HIP events around each arm, arms alternating, medians of {args.repeats} (min and max are "
                                 "the rounds' spread); two untimed calls of every arm first; read_back is the 4-byte "
                                 "device read of m on an idle stream",
                       "tables": sizes})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def ab(args):
    libs = dict(x.split("=", 1) for x in args.ab)
    runs = {k: [] for k in libs}
    for _ in range(args.rounds):
        for name, lib in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "pair", "--repeats", str(args.repeats)],
                               env=dict(os.environ, SPLENDOR_AMD_LIB=os.path.abspath(lib)), capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:
                print(name, "FAILED", r.stderr[-2000:])
                raise SystemExit(1)
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {name: {arm: {"median_of_medians_us": statistics.median(x[arm]["median_us"] for x in rs),
                        "medians_us": [x[arm]["median_us"] for x in rs]} for arm in rs[0]} for name, rs in runs.items()}
    line = json.dumps({"metric": "spl_successors (compact rows) + SPL_ACT_VALUE over its rows, 2p x 65 536 tables, one MI355X",
                       "timing": f"HIP events, one process per library and round, {args.rounds} rounds alternating, "
                                 f"{args.repeats} calls per arm and process", "libraries": out})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, nargs="+", default=[65536, 1600])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--games", type=int, default=400)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--part", type=str, default="all")
    ap.add_argument("--ab", type=str, nargs="+", default=[])
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.ab:
        return ab(args)
    if args.part == "pair":
        return pair_only(args)
    if args.part == "pairs":
        return pairs_part(args)

    import torch
    from splendor_gym import _native
    from splendor_gym.device import Engine
    from splendor_gym.evaluation import eval_vs_opponent
    from splendor_gym.search import OnePlyValuePolicy, pick

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    fused = golden_fused(torch, dev)
    sizes = {}
    for n in args.tables:
        e = midgame(Engine, torch, n, dev)
        twin = Engine(n, 2, device=dev)
        s = e.successors(mask_bits=False)
        chain_rows = torch.zeros(45, n, 300, dtype=torch.uint8, device=dev)
        consts = [torch.full((n,), a, dtype=torch.int32, device=dev) for a in range(45)]

        def step_chain():
            for a in range(45):
                twin.arena.copy_(e.arena)
                twin.step(consts[a], autoreset=False, final_obs=False, obs_u8=chain_rows[a])

        rows = s.obs_u8.view(45 * n, 300)
        value = torch.empty(45 * n, 1, dtype=torch.float32, device=dev)
        action = torch.empty(n, dtype=torch.int32, device=dev)
        pol = OnePlyValuePolicy(fused)
        arms = {"successors": lambda: e.successors(mask_bits=False, out=s),
                "step_chain": step_chain,
                "critic": lambda: fused.get_value(rows, out=value),
                "pick": lambda: pick(s.flags, s.reward, value, -1.0, out=action),
                "act": lambda: pol.act(e)}
        ms = timed(torch, arms, args.repeats)
        legal = (s.flags & _native.SUCC_LEGAL) != 0
        # the chain's rows of illegal pairs are the unchanged table's row, the call's are zero: compare the legal ones
        equal = bool(torch.equal(s.obs_u8[legal], chain_rows[legal]))
        med = {k: statistics.median(v) for k, v in ms.items()}
        out_bytes = 45 * n * (300 + 1 + 4)
        rate = out_bytes / (med["successors"] * 1e-3) / 1e12
        sizes[str(n)] = {
            "us": {k: stats(v) for k, v in ms.items()},
            "ratio_step_chain_over_successors": round(med["step_chain"] / med["successors"], 2),
            "equal_rows_of_legal_pairs": equal,
            "successors_output_bytes": out_bytes,
            "successors_store_rate_TBs": round(rate, 3),
            "ratio_to_headline_store_rate": round(rate / HEADLINE_STORE_TBS, 3),
            "act_share": {k: round(med[k] / med["act"], 3) for k in ("successors", "critic", "pick")},
            "legal_share_of_pairs": round(float(legal.float().mean()), 4)}
        twin.close()
        e.close()
        del s, chain_rows, rows, value, pol
        torch.cuda.empty_cache()

    greedy = lambda obs, mask: fused.greedy(obs, mask)
    strength = {}
    for opp in ("greedy_v1", "basic_priority"):
        strength[opp] = {"greedy_actor": eval_vs_opponent(greedy, opponent=opp, n_games=args.games, seed=0, device=dev),
                         "one_ply_value": eval_vs_opponent(OnePlyValuePolicy(fused), opponent=opp, n_games=args.games, seed=0,
                                                           device=dev)}
    line = json.dumps({"metric": "one-ply successors and the value-lookahead policy, 2 players, one MI355X",
                       "timing": f"HIP events around each arm, arms alternating, medians of {args.repeats}; two untimed "
                                 "calls of every arm first",
                       "headline_store_rate_TBs": HEADLINE_STORE_TBS, "tables": sizes,
                       "strength": {"games": args.games, "checkpoint": "tests/golden/ppo_splendor_latest.safetensors",
                                    "vs": strength}})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
