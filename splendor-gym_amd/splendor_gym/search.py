"""One-ply search on the device (include/splendor_search.h).

`OnePlyValuePolicy(fused)` plays argmax_a q(a) with a trained critic: Engine.successors writes the
45 successors of every table as compact rows, one SPL_ACT_VALUE call values all 45 n rows, and
spl_search_pick takes the best legal action per table — three launches, nothing on the host.
q(a) is the mover's reward where the move ends the game and minus the critic's value of the
successor otherwise: the critic values a position for the player to move, and in a two-player game
the next player's loss is the mover's gain.

`pick_reference` is the pick in numpy, the oracle of the kernel's tests.

About one pair in six is legal.  `OnePlyValuePolicy(fused, compact=True)` values the legal pairs only:
Engine.successor_pairs writes them compacted in a fixed order (by 64-table block, then action, then table), the
critic sees m rows instead of 45 n, and spl_search_pick_pairs (`pick_pairs`) picks over them — the same actions,
for one 4-byte read of m per decision.  `pairs_reference` and `pick_pairs_reference` restate the two calls in numpy.
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


def _pair_order(legal_bits):
    """The (a, t) of the set elements of a bool [45, n] plane in the contract's order: by (t // 64, a, t)."""
    a, t = np.nonzero(legal_bits)
    order = np.lexsort((t, a, t // 64))
    return a[order], t[order]


def pairs_reference(dense):
    """spl_successors_pairs' planes from dense ones, on the host.  `dense`: a mapping of [45, n, ...] arrays (or an
    object with such attributes, e.g. a Successors; tensors are copied to the host) holding `flags` and any of
    reward, obs_u8, mask_bits, winner, value.  Returns a dict of the same planes compacted to the pairs with
    SUCC_LEGAL, in the contract's order (by 64-table block, then action, then table), plus
      pair  int32 [m]: the dense index a * n + t,
      legal uint64 [n]: bit a set where (t, a) is legal,
      base  int32 [ceil(n / 64) + 1]: the exclusive prefix of the blocks' pair counts, base[-1] = m."""
    names = ("flags", "reward", "obs_u8", "mask_bits", "winner", "value")
    get = dense.get if hasattr(dense, "get") else lambda k: getattr(dense, k, None)
    planes = {}
    for k in names:
        x = get(k)
        if x is not None:
            planes[k] = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    flags = planes.get("flags")
    if flags is None or flags.ndim != 2 or flags.shape[0] != NUM_ACTIONS:
        raise ValueError("pairs_reference needs a [45, n] flags plane")
    n = flags.shape[1]
    for k, x in planes.items():
        if x.shape[:2] != (NUM_ACTIONS, n):
            raise ValueError(f"{k} must be [45, {n}, ...]")
    bits = (flags & SUCC_LEGAL) != 0
    a, t = _pair_order(bits)
    out = {k: np.ascontiguousarray(x[a, t]) for k, x in planes.items()}
    out["pair"] = (a * n + t).astype(np.int32)
    out["legal"] = (bits.astype(np.uint64) << np.arange(NUM_ACTIONS, dtype=np.uint64)[:, None]).sum(axis=0, dtype=np.uint64)
    nb = (n + 63) // 64
    counts = np.bincount(t // 64, minlength=nb)
    out["base"] = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return out


def pick_pairs_reference(legal, base, flags, reward, value, sign, capacity=None):
    """spl_search_pick_pairs on the host: legal uint64 [n], base int32 [ceil(n / 64) + 1], and flags, reward, value
    over the pairs in the contract's order.  pick_reference's semantics; a pair whose index is >= capacity
    (default: the planes' length) takes no part.  Returns (action int32 [n], best_q float32 [n])."""
    legal = np.asarray(legal).astype(np.uint64)
    base = np.asarray(base, np.int64)
    flags = np.asarray(flags, np.uint8).reshape(-1)
    reward = np.asarray(reward, np.float32).reshape(-1)
    value = np.asarray(value, np.float32).reshape(-1)
    n = legal.shape[0]
    if base.shape != ((n + 63) // 64 + 1,):
        raise ValueError("base must be [ceil(n / 64) + 1]")
    cap = min(len(flags), len(reward), len(value)) if capacity is None else int(capacity)
    if cap > min(len(flags), len(reward), len(value)):
        raise ValueError("capacity exceeds the planes")
    bits = ((legal[None, :] >> np.arange(NUM_ACTIONS, dtype=np.uint64)[:, None]) & np.uint64(1)) != 0
    a, t = _pair_order(bits)
    blk = t // 64
    first_of_block = np.searchsorted(blk, blk, side="left")  # the sorted list is block-major
    idx = base[blk] + (np.arange(len(t)) - first_of_block)
    keep = idx < cap
    a, t, idx = a[keep], t[keep], idx[keep]
    f = np.zeros((NUM_ACTIONS, n), np.uint8)
    r = np.zeros((NUM_ACTIONS, n), np.float32)
    v = np.zeros((NUM_ACTIONS, n), np.float32)
    f[a, t] = flags[idx] | np.uint8(SUCC_LEGAL)
    r[a, t] = reward[idx]
    v[a, t] = value[idx]
    return pick_reference(f, r, v, sign)


def pick_pairs(legal, base, flags, reward, value, sign, capacity=None, out=None, best_q=None):
    """spl_search_pick_pairs over a SuccessorPairs' device planes and the critic's values of its rows (value may be
    [m, 1]): int32 [n] actions into `out`, the greatest q into `best_q` when given.  capacity: the pairs the planes
    hold (default: the shortest plane's length); a pair at or beyond it takes no part."""
    torch = _native.require_gpu()
    lib = _native.load_library()
    n = legal.shape[0]
    dev = legal.device
    if legal.dtype != torch.int64 or legal.dim() != 1 or not legal.is_contiguous():
        raise ValueError("legal must be a contiguous int64 [n] tensor")
    if base.dtype != torch.int32 or tuple(base.shape) != ((n + 63) // 64 + 1,) or not base.is_contiguous() or base.device != dev:
        raise ValueError(f"base must be a contiguous int32 [ceil(n / 64) + 1] tensor on {dev}")
    for name, x, dt in (("flags", flags, torch.uint8), ("reward", reward, torch.float32), ("value", value, torch.float32)):
        if x.dtype != dt or not x.is_contiguous() or x.device != dev or x.numel() < 1:
            raise ValueError(f"{name} must be a contiguous non-empty {dt} tensor on {dev}")
    held = min(flags.numel(), reward.numel(), value.numel())
    cap = held if capacity is None else int(capacity)
    if not 1 <= cap <= held:
        raise ValueError("capacity must be 1 .. the planes' length")
    action = out if out is not None else torch.empty(n, dtype=torch.int32, device=dev)
    a = _native.PickPairsArgs(legal=legal.data_ptr(), base=base.data_ptr(), flags=flags.data_ptr(), reward=reward.data_ptr(),
                              value=value.data_ptr(), action=action.data_ptr(),
                              best_q=None if best_q is None else best_q.data_ptr(), sign=float(sign), capacity=cap)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib, lib.spl_search_pick_pairs(n, ctypes.byref(a), stream))
    return action


class OnePlyValuePolicy:
    """argmax_a q(a) over the one-ply successors, q from the critic of `fused` (a FusedActorCritic
    with a critic and an fp32 image).  Two players only: minus the next player's value is the mover's
    value only in a two-player game.

    act(engine) -> int32 [n] (-1 for a table without a legal action).  As a batched policy callable
    (obs, mask) -> actions it acts on the engine it was bound to: bind(env) stores the engine of an
    env that has one (DualStepVectorEnv.eng; evaluation.eval_vs_opponent binds its env).

    compact=True values the legal pairs only (Engine.successor_pairs, spl_search_pick_pairs): the critic sees m
    rows instead of 45 n.  The row count of the critic call comes from the host, so a decision then reads m back
    (4 bytes, the one host step), and calls again with buffers of 1.25 m rows if they were too small (the
    tables were only read).  capacity: the rows to start with (default 12 n).  The actions are the same."""

    def __init__(self, fused, compact=False, capacity=None):
        if not getattr(fused, "with_critic", False) or getattr(fused, "precision", None) not in ("fp32", "fp32_f16x2"):
            raise ValueError("OnePlyValuePolicy needs a FusedActorCritic with a critic and an fp32 image")
        self.fused = fused
        self.compact = bool(compact)
        self.capacity = capacity
        self.engine = None
        self._held = None  # (engine, Successors or SuccessorPairs, value, action): one engine's rows at a time
        self.critic_rows = None  # compact: the rows of the last decision's critic call (0: no call)

    def _act_compact(self, engine, out=None, best_q=None):
        torch = engine.torch
        if self._held is None or self._held[0] is not engine:
            pairs = engine.successor_pairs(capacity=self.capacity)
            self._held = (engine, pairs, torch.empty(pairs.capacity, 1, dtype=torch.float32, device=engine.device),
                          torch.empty(engine.n, dtype=torch.int32, device=engine.device))
        else:
            engine.successor_pairs(out=self._held[1])
        _, pairs, value, action = self._held
        m = pairs.total()
        if m > pairs.capacity:  # a run was cut: larger buffers and the call again (the arena was only read)
            pairs = engine.successor_pairs(capacity=(5 * m + 3) // 4)
            value = torch.empty(pairs.capacity, 1, dtype=torch.float32, device=engine.device)
            self._held = (engine, pairs, value, action)
        self.critic_rows = m
        if m:
            self.fused.get_value(pairs.obs_u8[:m], out=value[:m])
        return pick_pairs(pairs.legal, pairs.base, pairs.flags, pairs.reward, value, -1.0, capacity=max(m, 1),
                          out=action if out is None else out, best_q=best_q)

    def act(self, engine, out=None, best_q=None):
        """int32 [n] actions; best_q: a float32 [n] tensor for the greatest q of every table, when given"""
        if engine.P != 2:
            raise ValueError("OnePlyValuePolicy plays two-player tables only")
        if engine.device != self.fused.device:
            raise ValueError("the engine and the critic must be on one device")
        if self.compact:
            return self._act_compact(engine, out, best_q)
        if self._held is None or self._held[0] is not engine:
            torch = engine.torch
            self._held = (engine, None,
                          torch.empty(NUM_ACTIONS * engine.n, 1, dtype=torch.float32, device=engine.device),
                          torch.empty(engine.n, dtype=torch.int32, device=engine.device))
        _, succ, value, action = self._held
        succ = engine.successors(obs=False, obs_u8=True, mask_bits=False, winner=False, out=succ)
        self._held = (engine, succ, value, action)
        self.fused.get_value(succ.obs_u8.view(NUM_ACTIONS * engine.n, OBS_U8), out=value)
        return pick(succ.flags, succ.reward, value, -1.0, out=action if out is None else out, best_q=best_q)

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
