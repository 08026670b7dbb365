#pragma once
// spl_engine_deal.h — a new episode's deal and a table's way between HBM and registers: the Fisher-Yates deal from
// one engine seed into a deck record (Deal, deal_into, rec_deal, fresh_state), the PCG and pool planes, deal_next,
// the state words and the legal-mask cache (load_tab / store_*, LegalCache), the constant tables into LDS
// (load_tables_lds / dma_tables_lds), legal_of and the fused policies (policy_action).
#include "../../include/splendor_amd.h"
#include "spl_engine_args.h"
#include "spl_engine_base.h"
#include "spl_engine_rules.h"
#include "spl_layout.h"
#include "spl_rng.h"
#include "spl_scripted.h"

namespace spl {

// ------------------------------------------------------------------------------------------
// deal: engine/state.py:181-211 initial_state's shuffles, from one engine seed
// ------------------------------------------------------------------------------------------
// Fisher–Yates (Lib/random.py:389-394) over tier 1, 2, 3 decks then the nobles, driven by ONE
// uniform loop over MT outputs: every lane advances its own stream by one output per
// iteration and its own shuffle state machine accepts or rejects it (_randbelow), so the cost
// is the wave's maximum output count, not the sum of per-draw maxima.
struct Deal {
    uint32_t board[3], nob0, nob1;  // SW_BOARD.., SW_NOB0, SW_NOB1 of the dealt table
};
__device__ __forceinline__ Deal empty_deal() { return Deal{{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, 0xFFFFFFFFu, 0xFFu}; }

__device__ __forceinline__ uint32_t deal_into(uint32_t seed, int P, uint8_t *rec, uint8_t *scr, Deal &out,
                                              uint32_t *mtx) {
    for (int i = 0; i < 100; ++i) scr[i] = (uint8_t)(i < 90 ? i : i - 90);
    MTStream ms;
    ms.init(seed);
    int d = 0, base = 0, i = 39;
    uint32_t flags = 0;
    // _randbelow(i + 1) on output y; a rejected draw (or a finished lane, or `on` false) swaps x[i]
    // with itself.  The caller's LDS reads of the two bytes overlap the next output's computation.
    auto shuffle_step = [&](uint32_t y, bool on, auto &&between) {
        const int n = i + 1;
        const int r = (int)(y >> (32 - bit_length((uint32_t)n)));
        const bool acc = on && d < 4 && r < n;
        const int ai = base + i, ar = base + (acc ? r : i);
        SPL_CHECK(ai >= 0 && ai < 100 && ar >= 0 && ar < 100, BC_SCRATCH);
        const uint8_t xi = scr[ai], xr = scr[ar];
        between();
        scr[ai] = xr;
        scr[ar] = xi;
        const int i2 = acc ? i - 1 : i;
        const bool adv = acc && i2 == 0;  // deck finished: tier 2, tier 3, then the nobles
        d += adv ? 1 : 0;
        base = adv ? (d == 1 ? 40 : (d == 2 ? 70 : 90)) : base;
        i = adv ? (d == 1 ? 29 : (d == 2 ? 19 : 9)) : i2;
    };
    const int limit = min(g_stream_limit, MTStream::kMaxOut);
    uint32_t y = ms.next(0);
    for (int j = 0;; ++j) {
        if (!__any(d < 4)) break;
        if (j >= limit) break;  // lanes still shuffling continue below
        shuffle_step(y, true, [&] {
            if (j + 1 < limit) y = ms.next(j + 1);
        });
    }
    // Continuation past the streamed outputs (never met in natural play): one lane at
    // a time, its full MT19937 state in the LDS region mtx, from output kMaxOut on.
    for (uint64_t slow = __ballot(d < 4); slow; slow &= slow - 1) {
        if (lane_id() == __ffsll((unsigned long long)slow) - 1) {
            LaneMT mt{mtx, 0};
            mt.init(seed);
            mt.start_at(limit);
            while (d < 4) shuffle_step(mt.next(), true, [] {});
        }
    }
    // deck bytes (list order; the 4 dealt cards per tier sit past deck_len)
    const uint32_t *s1 = reinterpret_cast<const uint32_t *>(scr);  // 4-byte aligned scratch
    uint32_t *r1 = reinterpret_cast<uint32_t *>(rec);
#pragma unroll
    for (int q = 0; q < 24; ++q) r1[q] = s1[q];
#pragma unroll
    for (int t = 0; t < 3; ++t) {  // board[tier][i] = deck.pop()
        const int b = tier_base(t), n = tier_size(t);
        out.board[t] = (uint32_t)scr[b + n - 1] | ((uint32_t)scr[b + n - 2] << 8) | ((uint32_t)scr[b + n - 3] << 16) |
                       ((uint32_t)scr[b + n - 4] << 24);
    }
    const int nn = P + 1 < 10 ? P + 1 : 10;  // state.py:194 (<= 5 for P <= 4)
    out.nob0 = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) out.nob0 |= (s < nn ? (uint32_t)scr[90 + s] : 0xFFu) << (8 * s);
    out.nob1 = nn > 4 ? (uint32_t)scr[94] : 0xFFu;
    uint32_t *rw = reinterpret_cast<uint32_t *>(rec);
#pragma unroll
    for (int k = 0; k < 3; ++k) rw[kRecTail / 4 + k] = out.board[k];
    rw[kRecTail / 4 + 3] = out.nob0;
    rw[kRecTail / 4 + 4] = out.nob1;
    rw[kRecSeed / 4] = seed;
    return flags;
}

// the board / noble words of a dealt record (its bytes 96..115)
__device__ __forceinline__ Deal rec_deal(const uint8_t *rec) {
    const uint32_t *rw = reinterpret_cast<const uint32_t *>(rec);
    Deal d;
#pragma unroll
    for (int k = 0; k < 3; ++k) d.board[k] = rw[kRecTail / 4 + k];
    d.nob0 = rw[kRecTail / 4 + 3];
    d.nob1 = rw[kRecTail / 4 + 4];
    return d;
}

template <int P>
__device__ __forceinline__ void fresh_state(Tab<P> &T, uint32_t status, const Deal &d) {
    constexpr uint32_t nn = P + 1 < 10 ? P + 1 : 10;
    T.sw[SW_BANK0] = 0x04040404u;                       // DEFAULT_BANK, state.py:26-33
    T.sw[SW_BANK1] = 4u | (5u << 8) | (0u << 16) | (1u << 24);  // to_play 0, turn_count 1
    T.sw[SW_MISC] = status;                              // move_count 0, winner None
    T.sw[SW_BOARD] = d.board[0];
    T.sw[SW_BOARD + 1] = d.board[1];
    T.sw[SW_BOARD + 2] = d.board[2];
    T.sw[SW_DECK] = 36u | (26u << 8) | (16u << 16) | (nn << 24);  // 40, 30, 20 minus the 4 dealt
    T.sw[SW_NOB0] = d.nob0;
    T.sw[SW_NOB1] = d.nob1;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        T.pw[q][0] = T.pw[q][1] = T.pw[q][2] = 0u;
        T.pw[q][3] = 0xFFFFFF00u;
    }
}

__device__ __forceinline__ Pcg64 load_pcg(const KArena &A, int t) {
    const uint64_t *p = reinterpret_cast<const uint64_t *>(A.pcg + (size_t)t * kPcgBytes);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p + 4);
    Pcg64 g;
    g.s_hi = p[0];
    g.s_lo = p[1];
    g.inc_hi = p[2];
    g.inc_lo = p[3];
    g.has32 = q[0];
    g.u32 = q[1];
    return g;
}
__device__ __forceinline__ void store_pcg(const KArena &A, int t, const Pcg64 &g) {
    uint64_t *p = reinterpret_cast<uint64_t *>(A.pcg + (size_t)t * kPcgBytes);
    uint32_t *q = reinterpret_cast<uint32_t *>(p + 4);
    p[0] = g.s_hi;
    p[1] = g.s_lo;
    p[2] = g.inc_hi;
    p[3] = g.inc_lo;
    q[0] = g.has32;
    q[1] = g.u32;
}

__device__ __forceinline__ Deal load_pool(const KArena &A, int t) {
    SPL_CHECK(t >= 0 && t < A.n, BC_TABLE);
    Deal d;
#pragma unroll
    for (int k = 0; k < 3; ++k) d.board[k] = A.pool[(size_t)(PL_BOARD + k) * A.n + t];
    d.nob0 = A.pool[(size_t)PL_NOB0 * A.n + t];
    d.nob1 = A.pool[(size_t)PL_NOB1 * A.n + t];
    return d;
}
__device__ __forceinline__ void store_pool(const KArena &A, int t, const Deal &d) {
    SPL_CHECK(t >= 0 && t < A.n, BC_TABLE);
#pragma unroll
    for (int k = 0; k < 3; ++k) A.pool[(size_t)(PL_BOARD + k) * A.n + t] = d.board[k];
    A.pool[(size_t)PL_NOB0 * A.n + t] = d.nob0;
    A.pool[(size_t)PL_NOB1 * A.n + t] = d.nob1;
}

// Deal the next episode into slot record `slot` from the table's engine-seed stream
// (envs/splendor_env.py:43-44: reset() continues self.np_random).  Returns SPL_F_* bits.
// A table never reset with a seed has no stream: it deals engine seed 0 (documented in
// splendor_amd.h) and its record stays unseeded.
template <int P>
__device__ __forceinline__ uint32_t deal_next(const KArena &A, int t, int slot, uint8_t *scr, Deal &d, uint32_t *mtx) {
    Pcg64 g = load_pcg(A, t);
    uint32_t seed = 0u;
    if (g.valid()) {
        seed = g.engine_seed();
        store_pcg(A, t, g);
    }
    return deal_into(seed, P, slot_rec(A, t, slot), scr, d, mtx);
}

template <int P>
__device__ __forceinline__ void load_tab(Tab<P> &T, const KArena &A, int t) {
    SPL_CHECK(t >= 0 && t < A.n, BC_TABLE);
#pragma unroll
    for (int w = 0; w < SW_COUNT; ++w) T.sw[w] = A.planes[(size_t)w * A.n + t];
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) T.pw[q][k] = A.planes[(size_t)pw_index(q, k) * A.n + t];
}

// The table state and its legal-mask cache entry: `legal` is legal_moves of T (as computed under the
// context tagged `tag`), or anything with tag 0 when the storing kernel does not know it.  Every
// kernel that stores state goes through here, so no stale mask survives a state change.
template <int P>
__device__ __forceinline__ void store_words(const Tab<P> &T, const KArena &A, int t) {  // state words only
    SPL_CHECK(t >= 0 && t < A.n, BC_TABLE);
#pragma unroll
    for (int w = 0; w < SW_COUNT; ++w) A.planes[(size_t)w * A.n + t] = T.sw[w];
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) A.planes[(size_t)pw_index(q, k) * A.n + t] = T.pw[q][k];
}
// `tag`: KTables::mtag (the shift drops its flag bit) or 0
__device__ __forceinline__ void store_legal(const KArena &A, int t, uint64_t legal, uint32_t tag) {
    static_assert(kLegalTagShift == 16 && kLegalTagMax == 0xFFFFu, "the tag is the low half of KTables::mtag");
    A.legal[t] = (uint32_t)legal;
    A.legal[A.n + t] = ((uint32_t)(legal >> 32) & kLegalHiBits) | (tag << kLegalTagShift);
}
template <int P>
__device__ __forceinline__ void store_tab(const Tab<P> &T, const KArena &A, int t, uint64_t legal, uint32_t tag) {
    store_words(T, A, t);
    store_legal(A, t, legal, tag);
}

// the cached legal mask of table t's stored state, if it was computed under context tag `tag`
struct LegalCache {
    uint32_t lo, hi;
    // tag 0 is "unknown" on both sides: an entry a crafted upload left, and a context without a tag of its
    // own (card_table_tag ran out) never trusts an entry
    // (`tag`: KTables::mtag, its flag bit above the tag ignored)
    __device__ __forceinline__ bool known(uint32_t tag) const {
        return (tag & kLegalTagMax) != 0u && (hi >> kLegalTagShift) == (tag & kLegalTagMax);
    }
    __device__ __forceinline__ uint64_t mask() const { return (uint64_t)lo | ((uint64_t)(hi & kLegalHiBits) << 32); }
};
__device__ __forceinline__ LegalCache load_legal(const KArena &A, int t) {
    return LegalCache{A.legal[t], A.legal[A.n + t]};
}

__device__ __forceinline__ void load_tables_lds(Consts &L, const KTables &Tb) {
    for (int i = lane_id(); i < 90; i += 64) L.cards[i] = Tb.cards[i];
    if (lane_id() < 10) L.nobles[lane_id()] = Tb.nobles[lane_id()];
}
// The same tables by LDS-DMA from ONE wave (global_load_lds, 16 B per lane: 90 card records, then the
// 80-B noble array as five 16-B pieces): no registers and no LDS write instructions, and the issuing
// wave's own vmcnt covers their landing — a later s_waitcnt vmcnt(0) of that wave makes them readable
// to it, and a barrier after that to the workgroup.
typedef __attribute__((address_space(3))) void lds_void_t;
__device__ __forceinline__ void dma_tables_lds(Consts &L, const KTables &Tb) {
    const int lane = lane_id();
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(Tb.cards + lane), (lds_void_t *)&L.cards[0], 16, 0, 0);
    if (lane < 26)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(Tb.cards + 64 + lane), (lds_void_t *)&L.cards[64],
                                         16, 0, 0);
    if (lane < 5)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint8_t *>(Tb.nobles) + 16 * lane,
                                         (lds_void_t *)&L.nobles[0], 16, 0, 0);
}

template <int P>
__device__ __forceinline__ uint64_t legal_of(const Tab<P> &T, const Consts &L) {
    uint32_t w[4];
    get_player(T, get_to_play(T.sw), w);
    const Pl p = unpack_pl(w);
    int bank[6];
    get_bank(T.sw, bank);
    return legal_mask(T.sw, p, bank, L);
}

// the fused policies (spl_scripted.h) for a table whose state is in registers
template <int P>
__device__ __forceinline__ int policy_action(int policy, uint64_t m, const Tab<P> &T, const Consts &L,
                                             uint64_t seed, uint64_t table, uint64_t ply) {
    if (policy == SPL_POLICY_GREEDY_V1) return greedy_v1(m);
    if (policy == SPL_POLICY_BASIC_PRIORITY)  // board points: obs[32 + 13k + 2]
        return basic_priority(m, [&](int k, bool) { return (int)bget(card_rec(L, board_get(T.sw, k)).x, 2); }, seed,
                              table, ply);
    return sample_uniform(m, seed, table, ply);
}

}  // namespace spl
