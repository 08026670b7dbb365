"""One-ply search on the device (include/splendor_search.h).

`OnePlyValuePolicy(fused)` plays argmax_a q(a) with a trained critic: Engine.successors writes the
45 successors of every table as compact rows, one SPL_ACT_VALUE call values all 45 n rows, and
spl_search_pick takes the best legal action per table — three launches, nothing on the host.
q(a) is the mover's reward where the move ends the game and minus the critic's value of the
successor otherwise: the critic values a position for the player to move, and in a two-player game
the next player's loss is the mover's gain.

`pick_reference` is the pick in numpy, the oracle of the kernel's tests.
"""
import ctypes

import numpy as np

from . import _native
from ._native import NUM_ACTIONS, OBS_U8, SUCC_LEGAL, SUCC_TERMINATED, PickArgs, check


def pick_reference(flags, reward, value, sign):
    """spl_search_pick on the host: flags uint8, reward and value float32, each [45, n].  Returns
    (action int32 [n], best_q float32 [n]): the legal a of greatest q = TERMINATED ? reward :
    sign * value, compared with q > best from best = -inf (a NaN never wins, the lowest a wins a
    tie); the first legal a if no comparison succeeds; -1 if none is legal."""
    flags = np.asarray(flags, np.uint8)
    reward = np.asarray(reward, np.float32)
    value = np.asarray(value, np.float32)
    if not (flags.shape == reward.shape == value.shape and flags.ndim == 2 and flags.shape[0] == NUM_ACTIONS):
        raise ValueError("flags, reward and value must be [45, n]")
    n = flags.shape[1]
    with np.errstate(invalid="ignore"):
        q = np.where((flags & SUCC_TERMINATED) != 0, reward, np.float32(sign) * value).astype(np.float32)
    legal = (flags & SUCC_LEGAL) != 0
    best = np.full(n, -np.inf, np.float32)
    act = np.full(n, -1, np.int32)
    first = np.full(n, -1, np.int32)
    for a in range(NUM_ACTIONS):
        first = np.where(legal[a] & (first < 0), a, first).astype(np.int32)
        with np.errstate(invalid="ignore"):
            better = legal[a] & (q[a] > best)
        best = np.where(better, q[a], best).astype(np.float32)
        act = np.where(better, a, act).astype(np.int32)
    return np.where(act >= 0, act, first).astype(np.int32), best


def pick(flags, reward, value, sign, out=None, best_q=None):
    """spl_search_pick over [45, n] device planes (value may be [45 n, 1], as the critic wrote it):
    int32 [n] actions into `out`, the greatest q into `best_q` when given."""
    torch = _native.require_gpu()
    lib = _native.load_library()
    n = flags.shape[1]
    dev = flags.device
    if flags.dtype != torch.uint8 or tuple(flags.shape) != (NUM_ACTIONS, n) or not flags.is_contiguous():
        raise ValueError("flags must be a contiguous uint8 [45, n] tensor")
    for name, x in (("reward", reward), ("value", value)):
        if x.dtype != torch.float32 or x.numel() != NUM_ACTIONS * n or not x.is_contiguous() or x.device != dev:
            raise ValueError(f"{name} must be a contiguous float32 tensor of 45 n elements on {dev}")
    action = out if out is not None else torch.empty(n, dtype=torch.int32, device=dev)
    a = PickArgs(flags=flags.data_ptr(), reward=reward.data_ptr(), value=value.data_ptr(), action=action.data_ptr(),
                 best_q=None if best_q is None else best_q.data_ptr(), sign=float(sign))
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib, lib.spl_search_pick(n, ctypes.byref(a), stream))
    return action


class OnePlyValuePolicy:
    """argmax_a q(a) over the one-ply successors, q from the critic of `fused` (a FusedActorCritic
    with a critic and an fp32 image).  Two players only: minus the next player's value is the mover's
    value only in a two-player game.

    act(engine) -> int32 [n] (-1 for a table without a legal action).  As a batched policy callable
    (obs, mask) -> actions it acts on the engine it was bound to: bind(env) stores the engine of an
    env that has one (DualStepVectorEnv.eng; evaluation.eval_vs_opponent binds its env)."""

    def __init__(self, fused):
        if not getattr(fused, "with_critic", False) or getattr(fused, "precision", None) not in ("fp32", "fp32_f16x2"):
            raise ValueError("OnePlyValuePolicy needs a FusedActorCritic with a critic and an fp32 image")
        self.fused = fused
        self.engine = None
        self._held = None  # (engine, Successors, value, action): one engine's 45 n rows at a time

    def act(self, engine, out=None):
        if engine.P != 2:
            raise ValueError("OnePlyValuePolicy plays two-player tables only")
        if engine.device != self.fused.device:
            raise ValueError("the engine and the critic must be on one device")
        if self._held is None or self._held[0] is not engine:
            torch = engine.torch
            self._held = (engine, None,
                          torch.empty(NUM_ACTIONS * engine.n, 1, dtype=torch.float32, device=engine.device),
                          torch.empty(engine.n, dtype=torch.int32, device=engine.device))
        _, succ, value, action = self._held
        succ = engine.successors(obs=False, obs_u8=True, mask_bits=False, winner=False, out=succ)
        self._held = (engine, succ, value, action)
        self.fused.get_value(succ.obs_u8.view(NUM_ACTIONS * engine.n, OBS_U8), out=value)
        return pick(succ.flags, succ.reward, value, -1.0, out=action if out is None else out)

    def bind(self, env):
        engine = getattr(env, "eng", None) or getattr(env, "engine", None)
        if engine is None:
            raise ValueError("bind: the env has no engine (eng)")
        if engine.P != 2:
            raise ValueError("OnePlyValuePolicy plays two-player tables only")
        self.engine = engine
        return self

    def __call__(self, obs, mask):
        if self.engine is None:
            raise RuntimeError("OnePlyValuePolicy: bind(env) first")
        return self.act(self.engine).clamp_(min=0)  # a table without a legal action: 0, as the scripted policies answer
