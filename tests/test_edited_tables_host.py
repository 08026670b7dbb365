"""The edited tables of tests/edited_tables.py on the CPU oracle alone: the runs of
tests/test_gpu_edited_tables.py, with the device uniform policy restated on the host, reach the paths
they are there for (the floors that module asserts again on the oracle's side of each GPU run), and the
oracle's tables are the canonical ones afterwards."""
import numpy as np
import pytest

import edited_tables as et
from oracle.oracle import Oracle

FRESH = ((1 << 15) - 1) | (((1 << 15) - 1) << 27)  # kFreshDealMask (csrc/spl_engine_rules.h)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def test_tables_are_formulas_over_the_canonical_pair():
    cards, nobles = et.canonical()
    free, _ = et.free_tables()
    assert (free[::7, 3:8] == 0).all() and np.array_equal(np.delete(free, np.s_[::7], 0), np.delete(cards, np.s_[::7], 0))
    sud, n2 = et.sudden_tables()
    assert (sud[:, 2] == 15).all() and sud[:, 3:8].max() == 1 and np.array_equal(n2, nobles)
    assert np.array_equal(sud[:, 3:8] > 0, cards[:, 3:8] > 0) and np.array_equal(sud[:, :2], cards[:, :2])
    c3, nob = et.noble_tables()
    assert np.array_equal(c3, cards) and (nob[0::2, :5] == 0).all() and nob[:, :5].max() == 1
    assert nob[:, 5].tolist() == [1, 2, 3, 4, 5, 1, 2, 3, 4, 5]
    pc, pn = et.prestige_tables()
    assert 14 + int(pc[:, 2].max()) + int(pn[:, 5].max()) == 234


@pytest.mark.parametrize("name,P,seed", [("FREE", 2, 2101), ("SUDDEN", 2, 2102), ("NOBLE", 2, 2103), ("SUDDEN", 3, 3102),
                                         ("FREE", 4, 4101), ("NOBLE", 4, 4103)])
def test_step_chain_runs_reach_their_paths(orc, name, P, seed):
    """1 000 tables, 200 plies, the seeds of test_spl_step_chain.  Observed: FREE 2 223 of 2 557 fresh deals
    with a legal purchase (2 players; 3 308 of 3 829 at 4), SUDDEN 27.3 ends per table and 6.1 % ties at 2
    players, 20.8 and 10.0 % at 3, NOBLE 9.07 awards per table at 2 players."""
    cov = et.oracle_step_chain(orc, name, P, 1000, 200, seed)
    et.check_coverage(name, P, cov, 200)
    assert orc.legal(orc.initial_state(P, 1)) == FRESH  # canonical tables again


@pytest.mark.parametrize("name,P", [("SUDDEN", 2), ("FREE", 2), ("SUDDEN", 3), ("FREE", 4)])
def test_rollout_runs_reach_their_paths(orc, name, P):
    """1 000 tables, 96 steps in 16-step refill periods, the seeds of test_rollout_shapes_against_the_oracle.
    Observed: SUDDEN 13.2 ends per table at 2 players with up to 4 resets of one table inside one refill
    period (the pool of three deals is spent: inline deals, the dealer's spent-pool batch), 10.0 at 3
    players; FREE 894 of 1 027 fresh deals with a legal purchase at 2 players, 1 462 of 1 698 at 4."""
    cov = et.oracle_rollout_chain(orc, name, P, 1000, 96, 5, 3)
    c = et.check_coverage(name, P, cov, 96)
    if name == "SUDDEN" and P == 2:
        assert c["max_in_window"] > 3, c


def test_free_card_on_a_fresh_deal_is_buyable(orc):
    """What kFreshDealMask assumes (no purchase on a fresh deal) fails under FREE, and only there."""
    cards, nobles = et.free_tables()
    with et.oracle_tables(orc, cards, nobles):
        masks = [orc.legal(orc.initial_state(2, s)) for s in range(200)]
    assert sum(1 for m in masks if m & int(et.BUY_VISIBLE)) > 100
    assert all((m & ~int(et.BUY_VISIBLE)) == FRESH for m in masks)
    assert orc.legal(orc.initial_state(2, 0)) == FRESH
