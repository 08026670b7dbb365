"""Fixture for the bank-aware greedy_v2 opponent: the REFERENCE scripts/eval_suite.py eval_vs_opponent
with deterministic agents (first legal action, last legal action) against
greedy_opponent_v2_factory(env), `env` being the SplendorEnv inside each game's SelfPlayWrapper — so
the opponent reads the bank from env.state and the scarcity branches are the ones pinned (without an
env the reference falls back to a uniform bank).  Same (seed, n_games) pairs as eval.json.  Loaded as
in make_golden.py.

    python tests/golden/make_golden_eval_v2.py     # here, with the reference present
"""
import json
import os

import numpy as np

import make_golden as mg  # noqa: F401  (installs the reference + gymnasium stand-in)
from make_golden_eval import first_legal, last_legal

HERE = os.path.dirname(os.path.abspath(__file__))


if __name__ == "__main__":
    from splendor_gym.envs import SplendorEnv
    from splendor_gym.scripts import eval_suite as es
    from splendor_gym.wrappers.selfplay import SelfPlayWrapper

    def make_env():
        inner = SplendorEnv(num_players=2)
        env = SelfPlayWrapper(inner, opponent_policy=es.greedy_opponent_v2_factory(inner))
        env.reset(seed=0)
        return env

    out = []
    for agent_name, agent in (("first_legal", first_legal), ("last_legal", last_legal)):
        for seed, n in ((0, 60), (7, 40)):
            res = es.eval_vs_opponent(make_env, agent, n_games=n, seed=seed)
            out.append({"agent": agent_name, "opponent": "greedy_v2", "seed": seed, "n_games": n,
                        "result": {k: (float(v) if isinstance(v, (float, np.floating)) else int(v)) for k, v in res.items()}})
            print(agent_name, seed, res)
    with open(os.path.join(HERE, "eval_v2.json"), "w") as f:
        json.dump(out, f, indent=1)
