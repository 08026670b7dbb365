"""Batched evaluation against scripted or network opponents (reference scripts/eval_suite.py).

`eval_vs_opponent` plays `n_games` games at once, one table per game, with the reference's
per-game seeds (np.random.RandomState(seed).randint(1e9) per game) and statistics
(eval_suite.py:162-208), keeping its conventions:
  * the agent is player 0 behind SelfPlayWrapper: when the opponent's move ends the game the
    agent's reward is minus the opponent's step reward (selfplay.py:54-58), so a turn-limit draw
    (-0.1 for the mover) counts as a win, as in the reference;
  * avg_prestige is the prestige of player (to_play - 1) % 2 at the end, i.e. of the opponent;
  * an action outside the legal mask counts toward illegal_action_rate (with no legal move the
    env's draw follows).  The reference then raises from SelfPlayWrapper for a non-empty mask;
    here the table simply stays at the agent's turn.
`agent_policy` is a batched callable (obs int32 [N,297], mask int8 [N,45]) -> actions [N];
`opponent` is a device policy name or a batched callable (see splendor_gym.selfplay).

`DeviceEvaluator` is the whole suite of training_utils.run_evaluation_suite in one batch: every
opponent kind plays at once, each table against its own kind, the tally stays on the device
(include/splendor_eval.h) and the turns replay as a linear hipGraph.
"""
import ctypes

import numpy as np
import torch

from . import _native
from .opponents import SCRIPTED_POLICIES, ScriptedOpponents
from .selfplay import DualStepVectorEnv

_OPP_PRESTIGE = 30   # obs: the other player's prestige (engine/encode.py:138-142); to_play == 0 at the end
_TURN_COUNT = 293    # obs: turn_count (encode.py:183)


def first_legal_policy(obs, mask):
    """Lowest legal action id (0 with none legal) for every row."""
    return torch.argmax(mask, dim=1).to(torch.int32)


def last_legal_policy(obs, mask):
    """Highest legal action id (0 with none legal) for every row."""
    last = mask.shape[1] - 1 - torch.argmax(torch.flip(mask, dims=[1]), dim=1)
    return torch.where(mask.any(dim=1), last, torch.zeros_like(last)).to(torch.int32)


@torch.no_grad()
def eval_vs_opponent(agent_policy, opponent="greedy_v1", n_games=400, seed=0, device=None, max_turns=1000):
    rng = np.random.RandomState(seed)
    seeds = [int(rng.randint(1e9)) for _ in range(n_games)]
    env = DualStepVectorEnv(n_games, device=device, opponent=opponent, opponent_obs=False)
    try:
        if hasattr(agent_policy, "bind"):  # a policy that reads the tables themselves (search.OnePlyValuePolicy)
            agent_policy.bind(env)
        obs, info = env.reset(seeds=seeds)
        dev = env.device
        playing = torch.ones(n_games, dtype=torch.bool, device=dev)
        result = torch.zeros(n_games, dtype=torch.float32, device=dev)
        turns = torch.zeros(n_games, dtype=torch.int32, device=dev)
        prestige = torch.zeros(n_games, dtype=torch.int32, device=dev)
        checks = torch.zeros((), dtype=torch.int64, device=dev)
        illegal = torch.zeros((), dtype=torch.int64, device=dev)
        for _ in range(max_turns):
            mask = info["action_mask"]
            a = torch.as_tensor(agent_policy(obs, mask), device=dev).to(torch.int32)
            legal_a = mask.gather(1, a.clamp(0, mask.shape[1] - 1).long()[:, None])[:, 0] != 0
            checks += playing.sum()
            illegal += (playing & ~legal_a).sum()
            obs, _, _, opp_reward, done, info = env.dual_step(a)
            ended = playing & done
            r = torch.where(info["game_ended_on"] == 1, info["agent_step_reward"], -opp_reward)
            final = info["final_observation"]
            result = torch.where(ended, r, result)
            turns = torch.where(ended, final[:, _TURN_COUNT], turns)
            prestige = torch.where(ended, final[:, _OPP_PRESTIGE], prestige)
            playing &= ~done
            if not bool(playing.any()):
                break
        res = result.cpu().numpy()
        n = n_games
        wins, losses = int((res > 0).sum()), int((res < 0).sum())
        p = wins / max(1, n)
        return {"n": n, "wins": wins, "losses": losses, "draws": n - wins - losses, "win_rate": p,
                "win_rate_ci95": float(1.96 * np.sqrt(p * (1 - p) / max(1, n))),
                "avg_turns": float(turns.double().mean()), "avg_prestige": float(prestige.double().mean()),
                "illegal_action_rate": float(illegal) / max(1, int(checks)),
                "unfinished": int(playing.sum())}
    finally:
        env.close()


_LEAGUE_IDS = dict(SCRIPTED_POLICIES, self_play=_native.EVAL_KEEP)
del _LEAGUE_IDS["keep"]


def _expand_rows(u8):
    """int32 [n, 297] observations of compact uint8 [n, 300] rows (selfplay.compact_rows inverted)."""
    obs = u8[:, :_native.OBS_DIM].to(torch.int32)
    obs[:, 295] += u8[:, 297].to(torch.int32) << 8
    return obs


class _LeagueOpponent:
    """DualStepVectorEnv's callable opponent of a DeviceEvaluator: the agent's own greedy forward on the
    self_play groups' slices, then the scripted kernel on every other row (SPL_EVAL_KEEP rows keep the
    forward's choice)."""
    accepts_u8 = True

    def __init__(self, ev):
        self.ev = ev

    def __call__(self, obs_u8, mask):
        ev = self.ev
        out = ev.env.opp_actions
        for g in ev._self_groups:
            ev._self_play_act(g, obs_u8, mask, out)
        if ev._scripted is not None:
            ev._scripted(obs_u8, mask, out=out)
        return out


class DeviceEvaluator:
    """run_evaluation_suite (training_utils.py:237-260) in one batch on the device.

    One DualStepVectorEnv of G * n_games tables, group g = tables [g * n, (g + 1) * n) playing
    opponents[g]: "random", "greedy_v1", "basic" (= "basic_priority"), "greedy_v2" or "self_play" (the
    agent's own greedy forward).  Game j of group g is seeded with draw j of
    np.random.RandomState(seed + g).randint(1e9) (run_evaluation_suite's seed = update_seed + i), its
    Philox key is j and the ply is 1 + the dual steps played so far, so each group's result equals
    eval_vs_opponent(agent, opponent, n_games, seed + g) whichever groups share the batch.

    run(agent) -> {name: stats}, stats as eval_vs_opponent returns them.  agent: a FusedActorCritic
    (played greedily) or any batched callable (obs int32 [N, 297], mask int8 [N, 45]) -> actions [N].

    A turn is: agent act, spl_eval_check, the dual step with the scripted kernel between its two
    phases, spl_eval_tally; after every `chunk` turns spl_eval_reduce and one [G, 8] copy to the host,
    which ends the loop when no table is unfinished (or at max_turns).  graph=True with a capturable
    agent (a FusedActorCritic, or a callable with a true `capturable` attribute) runs the first chunk
    eagerly, captures the chunk as one linear single-stream hipGraph and replays it; the ply lives in
    the env's device step counter, so a replay draws what the eager loop would."""

    def __init__(self, n_games, opponents=("random", "greedy_v1", "basic", "greedy_v2", "self_play"), device=None,
                 policy_seed=0, chunk=16, graph=True):
        opponents = tuple(opponents)
        if n_games < 1 or not opponents or chunk < 1:
            raise ValueError("n_games, chunk and the number of opponents must be positive")
        for name in opponents:
            if name not in _LEAGUE_IDS:
                raise ValueError(f"unknown opponent {name!r}; choose {sorted(_LEAGUE_IDS)}")
        if len(set(opponents)) != len(opponents):
            raise ValueError("each opponent kind may appear once (the results are keyed by name)")
        self.n_games, self.opponents, self.chunk, self.graph = int(n_games), opponents, int(chunk), bool(graph)
        n, G = self.n_games, len(opponents)
        self.lib = _native.load_library()
        counter_dev = torch.device(device) if device is not None else torch.device("cuda")
        if counter_dev.index is None:
            counter_dev = torch.device("cuda", torch.cuda.current_device())
        self._counter = torch.zeros(1, dtype=torch.int64, device=counter_dev)
        self.env = DualStepVectorEnv(G * n, device=counter_dev, opponent=_LeagueOpponent(self), policy_seed=policy_seed,
                                     opponent_obs=False, step_counter=self._counter, agent_obs_u8=True)
        dev = self.device = self.env.device
        N = G * n
        ids = [_LEAGUE_IDS[name] for name in opponents]
        self._self_groups = [g for g, i in enumerate(ids) if i == _native.EVAL_KEEP]
        self._scripted = None
        if len(self._self_groups) < G:
            self._scripted = ScriptedOpponents(
                policy_of=torch.tensor(ids, dtype=torch.int32, device=dev).repeat_interleave(n).contiguous(),
                seed=policy_seed, ply_base=self._counter, ply=1,
                table_key=torch.arange(n, dtype=torch.int64, device=dev).repeat(G).contiguous())
        self._group_of = torch.arange(G, dtype=torch.int32, device=dev).repeat_interleave(n).contiguous()
        z = lambda dt: torch.zeros(N, dtype=dt, device=dev)
        self.action = z(torch.int32)
        self.playing, self.result = z(torch.uint8), z(torch.int8)
        self.turns, self.prestige, self.checks, self.illegal = (z(torch.int32) for _ in range(4))
        self.totals = torch.zeros(G, _native.EVAL_COLS, dtype=torch.int64, device=dev)
        # a self_play slice whose mask rows start off a dword gets an aligned copy (spl_policy_act's rule)
        self._sp_mask = {g: torch.zeros(n, _native.NUM_ACTIONS, dtype=torch.int8, device=dev)
                         for g in self._self_groups if (g * n * _native.NUM_ACTIONS) % 4}
        env, e = self.env, self.env.eng
        p = lambda x: x.data_ptr()
        self._check = _native.EvalCheck(action=p(self.action), mask=p(e.mask), playing=p(self.playing),
                                        checks=p(self.checks), illegal=p(self.illegal))
        self._tally = _native.EvalTally(done=p(env.done), game_ended_on=p(env.game_ended_on),
                                        agent_step_reward=p(env.small_a[0]), opp_reward=p(env.opp_reward),
                                        final_obs=p(e.final_obs), playing=p(self.playing), result=p(self.result),
                                        turns=p(self.turns), prestige=p(self.prestige))
        self._reduce = _native.EvalReduce(group_of=p(self._group_of), playing=p(self.playing), result=p(self.result),
                                          turns=p(self.turns), prestige=p(self.prestige), checks=p(self.checks),
                                          illegal=p(self.illegal), out=p(self.totals))
        self._agent = None
        self._captured = None  # (agent, graph): the chunk captured for this agent
        self.replays = 0

    # ------------------------------------------------------------------------------------
    def _fused(self, agent):
        from .fused_policy import FusedActorCritic
        return isinstance(agent, FusedActorCritic)

    def _compact(self, agent):
        """Whether the agent's forward reads the compact uint8 rows."""
        return self._fused(agent) and agent.precision in ("fp32", "fp32_f16x2")

    def _agent_act(self):
        agent, env = self._agent, self.env
        e = env.eng
        if self._fused(agent):
            agent.greedy(env.agent_obs_u8 if self._compact(agent) else e.obs, e.mask, out=self.action)
        else:
            self.action.copy_(torch.as_tensor(agent(e.obs, e.mask), device=self.device).to(torch.int32))

    def _self_play_act(self, g, obs_u8, mask, out):
        agent, n = self._agent, self.n_games
        lo, hi = g * n, (g + 1) * n
        if self._compact(agent):
            m = mask[lo:hi]
            if g in self._sp_mask:
                m = self._sp_mask[g].copy_(m)
            agent.greedy(obs_u8[lo:hi], m, out=out[lo:hi])
        else:  # freshly allocated (aligned) int32 rows and mask for a generic forward
            fn = agent.greedy if self._fused(agent) else agent
            a = fn(_expand_rows(obs_u8[lo:hi]), mask[lo:hi].clone())
            out[lo:hi].copy_(torch.as_tensor(a, device=self.device).to(torch.int32))

    def _turns(self, k):
        """k turns and the reduction, launched on the current stream."""
        lib, env, N = self.lib, self.env, self.env.num_envs
        for _ in range(k):
            self._agent_act()
            stream = env.eng.stream()
            _native.check(lib, lib.spl_eval_check(N, ctypes.byref(self._check), stream))
            env.dual_step(self.action)
            _native.check(lib, lib.spl_eval_tally(N, ctypes.byref(self._tally), env.eng.stream()))
        _native.check(lib, lib.spl_eval_reduce(N, len(self.opponents), ctypes.byref(self._reduce), env.eng.stream()))

    def _capturable(self, agent):
        return self._fused(agent) or bool(getattr(agent, "capturable", False))

    @torch.no_grad()
    def run(self, agent, seed=0, max_turns=1000):
        n, G, env = self.n_games, len(self.opponents), self.env
        seeds = []
        for g in range(G):
            seeds += np.random.RandomState(seed + g).randint(1e9, size=n).tolist()  # the draws of n scalar calls
        self._agent = agent
        with torch.cuda.device(self.device):
            self._counter.zero_()
            env._ply = 0
            env.reset(seeds=seeds)
            self.playing.fill_(1)
            for x in (self.result, self.turns, self.prestige, self.checks, self.illegal, self.totals):
                x.zero_()
            use_graph = self.graph and self._capturable(agent)
            if self._captured is not None and self._captured[0] is not agent:
                self._captured = None
            played, totals = 0, None
            while played < max_turns:
                k = min(self.chunk, max_turns - played)
                if use_graph and k == self.chunk and self._captured is not None:
                    self._captured[1].replay()
                    self.replays += 1
                else:
                    self._turns(k)
                    if use_graph and k == self.chunk and self._captured is None:
                        # the eager chunk loaded every kernel and sized every buffer; capturing runs nothing
                        torch.cuda.synchronize(self.device)
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph):
                            self._turns(k)
                        self._captured = (agent, graph)
                played += k
                totals = self.totals.cpu().numpy()  # the one copy per chunk
                if not totals[:, 3].any():
                    break
            if totals is None:
                totals = self.totals.cpu().numpy()
        out = {}
        for g, name in enumerate(self.opponents):
            wins, losses, _, unfinished, turns, prestige, checks, illegal = (int(x) for x in totals[g])
            p = wins / max(1, n)
            out[name] = {"n": n, "wins": wins, "losses": losses, "draws": n - wins - losses, "win_rate": p,
                         "win_rate_ci95": float(1.96 * np.sqrt(p * (1 - p) / max(1, n))),
                         "avg_turns": turns / n, "avg_prestige": prestige / n,
                         "illegal_action_rate": illegal / max(1, checks), "unfinished": unfinished}
        return out

    def close(self):
        self._captured = None
        self.env.close()
