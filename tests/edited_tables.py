"""Edited card and noble tables for the parity tests, and what a test needs to run the CPU oracle on
them (tests/test_gpu_edited_tables.py, tests/test_edited_tables_host.py).

spl_ctx_create takes any card table (tier, bonus colour, points, five costs) and any noble table; the
canonical one never reaches some of the paths an edited one reaches all the time (a purchase legal on a
fresh deal, an episode every few plies, tie-breaks between winners, a noble on most turns).  The tables
below are formulas over the project's own engine/data/tables.json:

  FREE    cards with id % 7 == 0 cost nothing
  SUDDEN  every card is worth 15 points and no cost exceeds 1: the first purchase ends the game at the
          end of its round, so episodes last a few plies and ties between winners are common
  NOBLE   canonical cards; noble requirements capped at 1, none at all for the even nobles; noble i is
          worth 1 + i % 5 points
  PRESTIGE  cards with id % 3 == 0 are worth 120 points, every noble 100: a mover with 14 prestige who
          buys such a card and earns a noble holds 234, near the top of the packed prestige byte

The oracle's tables are global to its library (orc_set_tables) and other test modules share the
process: oracle_tables() restores the canonical pair on the way out.
"""
import contextlib

import numpy as np

from oracle.oracle import TABLE_DTYPE, load_tables

F_ILLEGAL, F_DRAW, F_TURN_LIMIT, F_AFTER_TERMINAL, F_OOB, F_RESET = 1, 2, 4, 8, 16, 32
BUY_VISIBLE = np.uint64(((1 << 12) - 1) << 15)  # actions 15..26


def canonical():
    cards, nobles = load_tables()
    return cards.astype(np.int32).copy(), nobles.astype(np.int32).copy()


def free_tables():
    cards, nobles = canonical()
    cards[np.arange(90) % 7 == 0, 3:8] = 0
    return cards, nobles


def sudden_tables():
    cards, nobles = canonical()
    cards[:, 2] = 15
    cards[:, 3:8] = np.minimum(cards[:, 3:8], 1)
    return cards, nobles


def noble_tables():
    cards, nobles = canonical()
    nobles[:, :5] = np.minimum(nobles[:, :5], 1)
    nobles[0::2, :5] = 0
    nobles[:, 5] = 1 + np.arange(10) % 5
    return cards, nobles


def prestige_tables():
    cards, nobles = canonical()
    cards[np.arange(90) % 3 == 0, 2] = 120
    nobles[:, 5] = 100
    return cards, nobles


TABLES = {"FREE": free_tables, "SUDDEN": sudden_tables, "NOBLE": noble_tables, "PRESTIGE": prestige_tables}


@contextlib.contextmanager
def oracle_tables(orc, cards, nobles):
    """The oracle library evaluates (cards, nobles) inside the block and the canonical pair after it."""
    c = np.ascontiguousarray(cards, np.int32)
    n = np.ascontiguousarray(nobles, np.int32)
    assert c.shape == (90, 8) and n.shape == (10, 6)
    orc.L.orc_set_tables(c.ctypes.data, n.ctypes.data)
    try:
        yield orc
    finally:
        orc.L.orc_set_tables(orc.cards.ctypes.data, orc.nobles.ctypes.data)


# ---- the device uniform-random policy on the host (csrc/spl_rng.h philox4x32, spl_scripted.h) -----------
_M32 = np.uint64(0xFFFFFFFF)


def _philox_x(c0, c1, c2, c3, k0, k1):
    """Word x of Philox4x32-10 over uint64 arrays holding 32-bit values."""
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> s32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0


def host_uniform(mask, seed, ply, table0=0):
    """spl_sample_uniform / the fused SPL_POLICY_UNIFORM draw for tables table0.. over the uint64 legal
    masks `mask`: Philox(seed; table, ply) scaled to the legal count picks the k-th legal action (0 when
    no action is legal)."""
    mask = np.asarray(mask, np.uint64)
    n = len(mask)
    t = np.arange(table0, table0 + n, dtype=np.uint64)
    full = lambda v: np.full(n, v, np.uint64)
    rx = _philox_x(t & _M32, t >> np.uint64(32), full(ply & 0xFFFFFFFF), full((ply >> 32) & 0xFFFFFFFF),
                   full(seed & 0xFFFFFFFF), full((seed >> 32) & 0xFFFFFFFF))
    bits = ((mask[:, None] >> np.arange(45, dtype=np.uint64)) & np.uint64(1)).astype(np.int64)
    count = bits.sum(axis=1)
    k = ((rx * count.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    pos = np.argmax(np.cumsum(bits, axis=1) > k[:, None], axis=1)
    return np.where(count > 0, pos, 0).astype(np.int32)


def injected(acts, rs):
    """run_parity's injection of illegal and (rarely) out-of-range actions into `acts` (three draws of the
    generator `rs` per ply, in this order)."""
    n = len(acts)
    inj = rs.random(n)
    acts = np.where(inj < 0.03, rs.integers(0, 45, n), acts)
    return np.where(inj > 0.998, rs.choice([-1, 45, 99], n), acts).astype(np.int32)


# ---- what a run reached, counted on the oracle's side ---------------------------------------------------
def _slots(vec):
    """The oracle's batched slots as a structured view of their table records."""
    dt = np.dtype({"names": ["s"], "formats": [TABLE_DTYPE], "offsets": [0], "itemsize": vec.slot_size})
    return np.ndarray(vec.n, dtype=dt, buffer=vec.buf)["s"]


class Coverage:
    """Counts over the steps of one OracleVec: episode ends, ends without a winner that are neither the
    turn limit nor a table without a legal move (compute_winner found a tie), fresh deals and those with a
    purchase bit in the oracle's mask, noble awards (a player's noble count growing in a step that did not
    end the episode; the last move's own award is not counted), and the most resets one table saw within
    one window of `window` steps (a pool of three deals per refill period is spent past three)."""

    def __init__(self, vec, window=0):
        self.vec, self.n = vec, vec.n
        self.ends = self.ties = self.deals = self.deals_with_purchase = self.awards = 0
        self.window, self.steps = window, 0
        self.in_window = np.zeros(vec.n, np.int64)
        self.max_in_window = 0
        self.nobles = self._noble_count()

    def _noble_count(self):
        s = _slots(self.vec)
        return s["players"]["n_nobles"][:, :self.vec.P].sum(axis=1).astype(np.int64)

    def update(self, ref):
        term = ref["terminated"] != 0
        reset = (ref["flags"] & F_RESET) != 0
        self.ends += int(term.sum())
        self.ties += int((term & (ref["winner"] < 0) & ((ref["flags"] & (F_DRAW | F_TURN_LIMIT)) == 0)).sum())
        self.deals += int(reset.sum())
        self.deals_with_purchase += int((reset & ((ref["mask"] & BUY_VISIBLE) != 0)).sum())
        now = self._noble_count()
        self.awards += int(((now > self.nobles) & ~reset).sum())
        self.nobles = now
        if self.window:
            if self.steps % self.window == 0:
                self.in_window[:] = 0
            self.in_window += reset
            self.max_in_window = max(self.max_in_window, int(self.in_window.max()))
        self.steps += 1

    def summary(self):
        return dict(ends=self.ends, ties=self.ties, deals=self.deals, deals_with_purchase=self.deals_with_purchase,
                    awards=self.awards, max_in_window=self.max_in_window, n=self.n)


def check_coverage(name, P, cov, plies):
    """The floors a run on table `name` must reach on the oracle's side (so a passing comparison cannot have
    skipped the path); those per table are scaled from 200 plies to the run's length."""
    c, scale = cov.summary(), plies / 200.0
    if name == "FREE":
        assert c["deals"] > 0 and 2 * c["deals_with_purchase"] >= c["deals"], c
    if name == "SUDDEN":
        assert c["ends"] >= 15 * scale * c["n"], c
        assert c["ties"] >= 0.02 * c["ends"], c
    if name == "NOBLE" and P == 2:
        assert c["awards"] >= 4 * scale * c["n"], c
    return c


def oracle_step_chain(orc, name, P, n, plies, seed, window=0):
    """The oracle's side of test_gpu_parity.run_parity on table `name`, alone: the device uniform policy
    restated on the host (host_uniform) with run_parity's injected actions.  Returns the Coverage."""
    from oracle.oracle import OracleVec
    cards, nobles = TABLES[name]()
    with oracle_tables(orc, cards, nobles):
        vec = OracleVec(orc, n, P, [seed + i for i in range(n)])
        cov = Coverage(vec, window)
        rs = np.random.default_rng(seed)
        nxt = host_uniform(vec.mask, seed, 0)
        for k in range(plies):
            ref = vec.step(injected(nxt, rs))
            cov.update(ref)
            nxt = host_uniform(ref["mask"], seed, k + 1)
    return cov


def oracle_rollout_chain(orc, name, P, n, steps, env_seed0, policy_seed, window=16):
    """The oracle's side of a rollout of `steps` steps from reset(seeds=env_seed0..) under the device
    uniform policy (plies 1..steps after the draw of ply 0), alone.  Returns the Coverage."""
    from oracle.oracle import OracleVec
    cards, nobles = TABLES[name]()
    with oracle_tables(orc, cards, nobles):
        vec = OracleVec(orc, n, P, [env_seed0 + i for i in range(n)])
        cov = Coverage(vec, window)
        nxt = host_uniform(vec.mask, policy_seed, 0)
        for k in range(steps):
            ref = vec.step(nxt)
            cov.update(ref)
            nxt = host_uniform(ref["mask"], policy_seed, k + 1)
    return cov
