"""Scripted opponents of the reference evaluation suite, as per-env callables (obs, info) -> action
with the reference behaviour (scripts/eval_suite.py:9-78; wrappers/selfplay.py:66-73).

Their batched device forms are the SPL_POLICY_* policies of the step kernel
(`DualStepVectorEnv(opponent="greedy_v1" | "basic_priority" | "random")`): greedy_v1 is
deterministic and identical; the random choices of the other two use the device Philox stream
instead of numpy's global generator.  `ScriptedOpponents` is the batched callable over the scripted
kernel of include/splendor_eval.h: those three and the bank-aware greedy_v2 (eval_suite.py:80-128), one
kind for every table or a kind per table, its ply advancing on the device.
"""
import ctypes

import numpy as np

from . import _native
from .wrappers._common import random_opponent  # noqa: F401  (wrappers/selfplay.py:66-73)

BOARD_OBS_OFFSET = 32  # first visible card's 13 observation ints (engine/encode.py:144-147)

# spl_eval_scripted_act's policy ids by name (include/splendor_eval.h); "keep" rows are a network's
SCRIPTED_POLICIES = {"random": _native.POLICY_UNIFORM, "greedy_v1": _native.POLICY_GREEDY_V1,
                     "basic_priority": _native.POLICY_BASIC_PRIORITY, "basic": _native.POLICY_BASIC_PRIORITY,
                     "greedy_v2": _native.POLICY_GREEDY_V2, "keep": _native.EVAL_KEEP}


class ScriptedOpponents:
    """The scripted opponents as one batched device callable (obs_or_u8, mask) -> int32 actions [n]
    (spl_eval_scripted_act): `name` for every table, or a policy id per table (`policy_of`, int32 [n] of
    SCRIPTED_POLICIES values; EVAL_KEEP rows keep what `out` already holds, e.g. a network's choice).
    obs is int32 [n, 297] or the compact uint8 [n, 300] rows (accepts_u8: DualStepVectorEnv then writes
    those for it).  "random", "greedy_v1" and "basic_priority" answer what the step kernel's fused
    policies answer for the same (seed, table key, ply); "greedy_v2" is eval_suite.py:80-128 with the
    bank read from the observation.  The ply of call k is `ply` + *ply_base (an int64 [1] device
    tensor, e.g. the env's step counter, which a replayed graph advances); row t's Philox key is
    table_key[t] (int64 [n]) or table0 + t.  `errors` (int64 [1]) counts rows with an unknown id."""
    accepts_u8 = True

    def __init__(self, policy_of=None, name=None, seed=0, ply_base=None, table_key=None, ply=1, table0=0, out=None):
        torch = _native.require_gpu()
        self.torch, self.lib = torch, _native.load_library()
        if (policy_of is None) == (name is None):
            raise ValueError("ScriptedOpponents takes either policy_of or name")
        if name is not None and name not in SCRIPTED_POLICIES:
            raise ValueError(f"unknown scripted opponent {name!r}; choose {sorted(SCRIPTED_POLICIES)}")
        for what, x, dt in (("policy_of", policy_of, torch.int32), ("table_key", table_key, torch.int64),
                            ("ply_base", ply_base, torch.int64), ("out", out, torch.int32)):
            if x is not None and not (isinstance(x, torch.Tensor) and x.dtype == dt and x.is_cuda and x.is_contiguous()):
                raise ValueError(f"{what} must be a contiguous {dt} device tensor")
        self.policy_of, self.table_key, self.ply_base, self.out = policy_of, table_key, ply_base, out
        self.policy = SCRIPTED_POLICIES[name] if name is not None else 0
        self.seed, self.ply, self.table0 = int(seed), int(ply), int(table0)
        self.errors = None

    def __call__(self, obs, mask, out=None):
        t = self.torch
        n = obs.shape[0]
        u8 = obs.dtype == t.uint8
        if (obs.dtype not in (t.int32, t.uint8) or obs.dim() != 2 or not obs.is_contiguous()
                or obs.shape[1] != (_native.OBS_U8 if u8 else _native.OBS_DIM)):
            raise ValueError("obs must be contiguous int32 [n, 297] or uint8 [n, 300] rows")
        if mask.dtype not in (t.int8, t.uint8, t.bool) or tuple(mask.shape) != (n, _native.NUM_ACTIONS) or \
                not mask.is_contiguous() or mask.device != obs.device:
            raise ValueError("mask must be a contiguous int8 [n, 45] tensor on obs's device")
        for what, x in (("policy_of", self.policy_of), ("table_key", self.table_key)):
            if x is not None and (x.numel() != n or x.device != obs.device):
                raise ValueError(f"{what} must hold one entry per table on obs's device")
        out = out if out is not None else self.out
        if out is None:
            out = t.zeros(n, dtype=t.int32, device=obs.device)
        elif out.numel() != n or out.device != obs.device:
            raise ValueError("out must hold one int32 per table on obs's device")
        if self.errors is None:
            self.errors = t.zeros(1, dtype=t.int64, device=obs.device)
        p = lambda x: None if x is None else x.data_ptr()
        a = _native.EvalAct(mask=mask.data_ptr(), obs=None if u8 else obs.data_ptr(), obs_u8=obs.data_ptr() if u8 else None,
                            policy_of=p(self.policy_of), table_key=p(self.table_key), ply_base=p(self.ply_base),
                            action=out.data_ptr(), errors=self.errors.data_ptr(), seed=self.seed & (2**64 - 1),
                            ply=self.ply & (2**64 - 1), table0=self.table0, policy=self.policy)
        with t.cuda.device(obs.device):
            stream = ctypes.c_void_p(t.cuda.current_stream(obs.device).cuda_stream)
            _native.check(self.lib, self.lib.spl_eval_scripted_act(n, ctypes.byref(a), stream))
        return out


def greedy_opponent_v1(obs, info):
    """First legal action among buys (visible or reserved), else take-2, take-3, reserve
    (eval_suite.py:9-29)."""
    legal = np.flatnonzero(info["action_mask"])
    if len(legal) == 0:
        return 0
    buys = legal[((legal >= 15) & (legal <= 26)) | ((legal >= 42) & (legal <= 44))]
    for group in (buys, legal[(legal >= 10) & (legal <= 14)], legal[legal <= 9], legal[(legal >= 27) & (legal <= 41)]):
        if len(group):
            return int(group[0])
    return int(legal[0])


def basic_priority_opponent(obs, info):
    """Visible buy with the most points (random tie-break), else a random reserved buy, else a
    random take-3, take-2, reserve (eval_suite.py:32-78)."""
    legal = np.flatnonzero(info["action_mask"])
    if len(legal) == 0:
        return 0
    vis = legal[(legal >= 15) & (legal <= 26)]
    if len(vis):
        pts = np.array([int(obs[BOARD_OBS_OFFSET + (a - 15) * 13 + 2]) for a in vis])
        return int(np.random.choice(vis[pts == pts.max()]))
    for lo, hi in ((42, 44), (0, 9), (10, 14), (27, 41)):
        group = legal[(legal >= lo) & (legal <= hi)]
        if len(group):
            return int(np.random.choice(group))
    return int(legal[0])
