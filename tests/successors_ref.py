"""What the successor tests share (tests/test_gpu_successors.py and its checked-build child): the CPU oracle's
answer for every (table, action) pair of a batch of downloaded tables, output buffers pre-filled with 0xAB, and
the comparison of one Engine.successors call against that answer.  Test infrastructure only."""
import numpy as np

from oracle.oracle import OBS_DIM, F_DRAW, F_ILLEGAL, F_TURN_LIMIT

LEGAL, TERMINATED, TURN_LIMIT, DREW = 0x01, 0x02, 0x04, 0x08  # SPL_SUCC_*
A = 45


def oracle_pairs(orc, recs):
    """Oracle.env_step(view_t, a) for every table record of `recs` (Engine.download()) and every action, through
    the same library call on a copy of the record.  The planes hold, for pairs that are not legal, the constants
    spl_successors states (zero rows, flags 0, reward 0, mask 0, winner -1)."""
    n = len(recs)
    R = dict(flags=np.zeros((A, n), np.uint8), obs=np.zeros((A, n, OBS_DIM), np.int32),
             u8=np.zeros((A, n, 300), np.uint8), mask=np.zeros((A, n), np.uint64), reward=np.zeros((A, n), np.float32),
             winner=np.full((A, n), -1, np.int8))
    obs = np.zeros(OBS_DIM, np.int32)
    mask, rew = np.zeros(1, np.uint64), np.zeros(1, np.float32)
    term, flags, hf = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    fr = np.zeros(4, np.float32)
    for t in range(n):
        terminal = bool(recs[t]["game_over"]) and int(recs[t]["to_play"]) == 0
        legal = 0 if terminal else int(orc.L.orc_legal(recs[t:t + 1].ctypes.data))
        for a in range(A):
            r = recs[t:t + 1].copy()
            err = orc.L.orc_env_step(r.ctypes.data, a, obs.ctypes.data, mask.ctypes.data, rew.ctypes.data,
                                     term.ctypes.data, flags.ctypes.data, fr.ctypes.data, hf.ctypes.data)
            ok = err == 0 and not (int(flags[0]) & (F_ILLEGAL | F_DRAW))
            # LEGAL <=> bit a of Oracle.legal(view_t) on a table that is not over
            assert ok == bool((legal >> a) & 1), (t, a, err, int(flags[0]), legal)
            if not ok:
                assert r.tobytes() == recs[t:t + 1].tobytes() or (int(flags[0]) & F_DRAW), (t, a)
                continue
            after = r[0]
            drew = bool((after["deck_len"] != recs[t]["deck_len"]).any())
            R["flags"][a, t] = LEGAL | (TERMINATED if term[0] else 0) | \
                (TURN_LIMIT if int(flags[0]) & F_TURN_LIMIT else 0) | (DREW if drew else 0)
            R["obs"][a, t] = obs
            R["u8"][a, t, :OBS_DIM] = obs & 0xFF
            R["u8"][a, t, 297] = int(after["move_count"]) >> 8
            assert obs[295] == int(after["move_count"]) and (np.delete(obs, 295) < 256).all()
            R["mask"][a, t] = mask[0]
            R["reward"][a, t] = rew[0]
            R["winner"][a, t] = int(after["winner"])
    return R


def prefilled(eng, obs=True, obs_u8=True, mask_bits=True, winner=True):
    """A Successors whose every byte is 0xAB: an element the call does not write shows."""
    import torch
    from splendor_gym.device import Successors
    n = eng.n

    def new(shape, dt):
        nb = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        return torch.full((nb,), 0xAB, dtype=torch.uint8, device=eng.device).view(dt).view(shape)
    return Successors(obs=new((A, n, OBS_DIM), torch.int32) if obs else None,
                      obs_u8=new((A, n, 300), torch.uint8) if obs_u8 else None,
                      flags=new((A, n), torch.uint8), reward=new((A, n), torch.float32),
                      mask_bits=new((A, n), torch.int64) if mask_bits else None,
                      winner=new((A, n), torch.int8) if winner else None)


def planes(s):
    """The host copies of a Successors' planes (None for a plane it lacks)."""
    get = lambda x: None if x is None else x.cpu().numpy()
    return dict(flags=get(s.flags), obs=get(s.obs), u8=get(s.obs_u8), reward=get(s.reward), winner=get(s.winner),
                mask=None if s.mask_bits is None else s.mask_bits.cpu().numpy().view(np.uint64))


def compare(got, R, tag=""):
    """Every plane of `got` (planes()) against the oracle's: legal pairs equal the step's outputs, the others
    hold their constants (R was built with them)."""
    np.testing.assert_array_equal(got["flags"], R["flags"], err_msg=f"{tag} flags")
    assert got["reward"].tobytes() == R["reward"].tobytes(), f"{tag} reward"
    for k in ("obs", "u8", "mask", "winner"):
        if got[k] is not None:
            np.testing.assert_array_equal(got[k], R[k], err_msg=f"{tag} {k}")


def random_plies(eng, plies, seed):
    """`plies` uniform-random plies without autoreset: tables that end stay over."""
    import torch
    na = torch.zeros(eng.n, dtype=torch.int32, device=eng.device)
    eng.sample_uniform(out=na, seed=seed, ply=0)
    for k in range(plies):
        eng.step(na.clone(), autoreset=False, next_actions=na, policy_seed=seed, ply=k + 1)
