"""gymnasium-0.29-compatible seeding, reduced to what the device needs.

The reference env draws each episode's engine seed from its gymnasium ``np_random``
(envs/splendor_env.py:42-43): ``Generator(PCG64(SeedSequence(seed)))`` created by
``reset(seed=...)`` and continued by later ``reset()`` calls.  The GPU continues that PCG64
stream itself (csrc/spl_rng.h, Pcg64); the host only turns a user seed into the initial PCG64
state — SeedSequence hashing is host-side setup, not per-step work.
"""
import numpy as np

MASK64 = (1 << 64) - 1


def pcg64_state(seed):
    """[state_hi, state_lo, inc_hi, inc_lo] of PCG64(SeedSequence(seed)) (seed None = fresh entropy)."""
    st = np.random.PCG64(np.random.SeedSequence(seed)).state["state"]
    s, inc = int(st["state"]), int(st["inc"])
    return [(s >> 64) & MASK64, s & MASK64, (inc >> 64) & MASK64, inc & MASK64]


_PCG_MULT = (2549297995355413924 << 64) | 4865540595714422341  # PCG_DEFAULT_MULTIPLIER_128


def _pcg64_states_u32(seeds):
    """pcg64_state for an array of seeds in [0, 2**32), all at once: numpy's SeedSequence hash of the
    one-word entropy [seed] (pool of four uint32, the constants of numpy/random/bit_generator.pyx;
    the hash constants do not depend on the data, so every seed runs the same uint32 operations),
    generate_state(4, uint64), then PCG64's pcg_setseq_128_srandom_r."""
    u32 = np.uint32
    x = np.asarray(seeds, dtype=np.uint64).astype(u32)
    const = [0x43b0d7e5]  # INIT_A, advanced by MULT_A at every hashmix

    def hashmix(v):
        v = v ^ u32(const[0])
        const[0] = (const[0] * 0x931e8875) & 0xFFFFFFFF
        v = v * u32(const[0])
        return v ^ (v >> u32(16))

    def mix(a, b):
        r = u32(0xca01f9dd) * a - u32(0x4973f715) * b
        return r ^ (r >> u32(16))

    with np.errstate(over="ignore"):
        pool = [hashmix(x)] + [hashmix(np.zeros_like(x)) for _ in range(3)]
        for src in range(4):
            for dst in range(4):
                if src != dst:
                    pool[dst] = mix(pool[dst], hashmix(pool[src]))
        words, c = [], 0x8b51f9dd  # INIT_B, advanced by MULT_B
        for i in range(8):
            v = pool[i % 4] ^ u32(c)
            c = (c * 0x58f38ded) & 0xFFFFFFFF
            v = v * u32(c)
            words.append((v ^ (v >> u32(16))).astype(np.uint64))
        u64 = np.uint64
        s_hi, s_lo, i_hi, i_lo = ((words[2 * i] | (words[2 * i + 1] << u64(32))) for i in range(4))  # little-endian pairs
        # 128-bit values as (hi, lo) uint64 pairs: inc = (initseq << 1) | 1; from state 0 the two steps
        # around `state += initstate` leave state = (inc + initstate) * MULT + inc (mod 2**128)
        inc_hi, inc_lo = (i_hi << u64(1)) | (i_lo >> u64(63)), (i_lo << u64(1)) | u64(1)
        a_lo = inc_lo + s_lo
        a_hi = inc_hi + s_hi + (a_lo < inc_lo).astype(u64)
        m_hi, m_lo, low = u64(_PCG_MULT >> 64), u64(_PCG_MULT & MASK64), u64(0xFFFFFFFF)
        a0, a1, b0, b1 = a_lo & low, a_lo >> u64(32), m_lo & low, m_lo >> u64(32)  # a_lo * m_lo, 64 x 64 -> 128
        p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
        mid = (p00 >> u64(32)) + (p01 & low) + (p10 & low)
        p_lo = (p00 & low) | (mid << u64(32))
        p_hi = p11 + (p01 >> u64(32)) + (p10 >> u64(32)) + (mid >> u64(32)) + a_lo * m_hi + a_hi * m_lo
        st_lo = p_lo + inc_lo
        st_hi = p_hi + inc_hi + (st_lo < p_lo).astype(u64)
    return np.stack([st_hi, st_lo, inc_hi, inc_lo], axis=1)


def pcg64_states(seeds):
    """uint64[n, 4] PCG64 states for a sequence of seeds (None entries draw fresh entropy).  Seeds that
    all fit 32 bits — every seed the envs and the evaluators derive — are hashed together in numpy
    (a Python call per seed is most of a large reset's time); anything else goes seed by seed."""
    seeds = list(seeds)
    if seeds and all(isinstance(s, (int, np.integer)) and 0 <= s < 2**32 for s in seeds):
        return _pcg64_states_u32(seeds)
    return np.array([pcg64_state(None if s is None else int(s)) for s in seeds], dtype=np.uint64).reshape(-1, 4)


def vector_seeds(seed, num_envs):
    """gymnasium SyncVectorEnv.reset seed expansion: int -> [seed + i], list kept, None -> None."""
    if seed is None:
        return None
    if isinstance(seed, (int, np.integer)):
        return [int(seed) + i for i in range(num_envs)]
    seeds = list(seed)
    if len(seeds) != num_envs:
        raise ValueError(f"expected {num_envs} seeds, got {len(seeds)}")
    return seeds
