"""Timings of the on-device evaluation league (splendor_gym.evaluation.DeviceEvaluator) beside the way the
same numbers were obtained before it: evaluation.eval_vs_opponent called once per opponent kind.

    python tools/bench_eval.py [--games 400 16384] [--repeats 5] [--out profiles/eval/bench_eval.json]

Per size, one evaluation of the trained reference checkpoint (greedy) per arm, the arms alternating,
medians over `repeats`; every arm ends in a device-to-host copy, so a host clock around the call is the
evaluation's wall time:
  league_graph / league_eager    DeviceEvaluator.run, 5 groups (random, greedy_v1, basic, greedy_v2,
                                 self_play), chunk turns as a hipGraph / as eager launches
  league4_graph / league4_eager  the same without greedy_v2: the four kinds the per-kind loop can play
  per_kind                       eval_vs_opponent for random, greedy_v1, basic_priority and the agent's own
                                 network in turn (a fresh env per call, one host synchronisation per turn)
The league4 arms and per_kind compute the same statistics; `equal` records that they did.  One untimed
call of every arm comes first (code objects, allocator, graph capture).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "splendor-gym_amd")]

FOUR = ("random", "greedy_v1", "basic", "self_play")
FIVE = ("random", "greedy_v1", "basic", "greedy_v2", "self_play")


def same(a, b):
    """the same groups with the same statistics (counts equal, means within 1e-12)"""
    return a.keys() == b.keys() and all(
        a[g].keys() == b[g].keys() and all(abs(a[g][k] - b[g][k]) <= 1e-12 for k in a[g]) for g in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, nargs="+", default=[400, 16384])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from safetensors.torch import load_file
    from splendor_gym.evaluation import DeviceEvaluator, eval_vs_opponent
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.policy import ActorCritic
    from splendor_gym.seeding import pcg64_states

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model = ActorCritic().to(dev).eval()
    model.load_state_dict(load_file(os.path.join(REPO, "tests", "golden", "ppo_splendor_latest.safetensors"), device=str(dev)))
    agent = FusedActorCritic(model)
    policy = lambda obs, mask: agent.greedy(obs, mask)

    sizes = {}
    for n in args.games:
        evs = {"league_graph": DeviceEvaluator(n, FIVE, device=dev, chunk=args.chunk, graph=True),
               "league_eager": DeviceEvaluator(n, FIVE, device=dev, chunk=args.chunk, graph=False),
               "league4_graph": DeviceEvaluator(n, FOUR, device=dev, chunk=args.chunk, graph=True),
               "league4_eager": DeviceEvaluator(n, FOUR, device=dev, chunk=args.chunk, graph=False)}

        def per_kind():
            out = {}
            for g, name in enumerate(FOUR):
                opp = {"basic": "basic_priority", "self_play": agent.opponent()}.get(name, name)
                out[name] = eval_vs_opponent(policy, opponent=opp, n_games=n, seed=g, device=dev)
            return out

        arms = {name: (lambda ev=ev: ev.run(agent, seed=0)) for name, ev in evs.items()}
        arms["per_kind"] = per_kind
        results = {name: fn() for name, fn in arms.items()}  # untimed: warm-up and the capture
        torch.cuda.synchronize(dev)
        secs = {name: [] for name in arms}
        for _ in range(args.repeats):
            for name, fn in arms.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                secs[name].append(time.perf_counter() - t0)
        med = {name: statistics.median(v) for name, v in secs.items()}

        # the host's share of every arm above: the per-game seeds (eval_vs_opponent draws them one scalar
        # call at a time, the league as one array) and their PCG64 states (seeding.pcg64_states), which
        # Engine.reset uploads — no device work
        def seeding(groups, scalar_draws):
            t0 = time.perf_counter()
            for g in range(groups):
                rng = np.random.RandomState(g)
                pcg64_states([int(rng.randint(1e9)) for _ in range(n)] if scalar_draws
                             else rng.randint(1e9, size=n).tolist())
            return time.perf_counter() - t0
        host = {"league": statistics.median(seeding(5, False) for _ in range(args.repeats)),
                "league4": statistics.median(seeding(4, False) for _ in range(args.repeats)),
                "per_kind": statistics.median(seeding(4, True) for _ in range(args.repeats))}
        turns = max(r["avg_turns"] for r in results["league_graph"].values())
        sizes[str(n)] = {
            "ms": {name: round(1e3 * v, 2) for name, v in med.items()},
            "ms_min_max": {name: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for name, v in secs.items()},
            "host_seeding_ms": {name: round(1e3 * v, 2) for name, v in host.items()},
            "ms_less_host_seeding": {name: round(1e3 * (v - host[name.split("_")[0] if name != "per_kind" else name]), 2)
                                     for name, v in med.items()},
            "ratio_per_kind_over_league4_graph": round(med["per_kind"] / med["league4_graph"], 2),
            "ratio_per_kind_over_league4_eager": round(med["per_kind"] / med["league4_eager"], 2),
            "ratio_league_eager_over_graph": round(med["league_eager"] / med["league_graph"], 2),
            "equal": {"league4_graph_vs_per_kind": same(results["league4_graph"], results["per_kind"]),
                      "league4_eager_vs_per_kind": same(results["league4_eager"], results["per_kind"]),
                      "league_graph_vs_eager": same(results["league_graph"], results["league_eager"])},
            "graph_replays_per_run": evs["league_graph"].replays / (args.repeats + 1),
            "longest_group_avg_turns": round(turns, 1),
            "win_rates": {k: round(v["win_rate"], 4) for k, v in results["league_graph"].items()}}
        for ev in evs.values():
            ev.close()
    line = json.dumps({"metric": "one evaluation of the trained checkpoint, one MI355X", "repeats": args.repeats,
                       "chunk": args.chunk,
                       "timing": "host clock around one whole call (each ends in a device-to-host copy), arms alternating, "
                                 "medians; one untimed call of every arm first",
                       "games_per_opponent": sizes})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
