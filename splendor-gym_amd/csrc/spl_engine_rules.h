#pragma once
// spl_engine_rules.h — the game's rules on one table held in registers (Tab<P>): pack and unpack, bank and board
// access, legal_mask / action_legal / any_legal, pay_for_card, the deck records, kFreshDealMask, the token return
// (MT stream and LUT), grant_noble, compute_winner and apply_action.  Per lane, no LDS staging beyond Consts, no
// global stores but the deck records.
#include "spl_engine_args.h"
#include "spl_engine_base.h"
#include "spl_layout.h"
#include "spl_rng.h"
#include "spl_scripted.h"

namespace spl {

template <int P>
struct Tab {
    uint32_t sw[SW_COUNT];
    uint32_t pw[P][4];
};

struct Pl {
    int tok[6], bon[5], pres, nres, rev, res[3];
};

__device__ __forceinline__ Pl unpack_pl(const uint32_t w[4]) {
    Pl p;
#pragma unroll
    for (int c = 0; c < 4; ++c) p.tok[c] = (int)bget(w[0], c);
    p.tok[4] = (int)bget(w[1], 0);
    p.tok[5] = (int)bget(w[1], 1);
    p.bon[0] = (int)bget(w[1], 2);
    p.bon[1] = (int)bget(w[1], 3);
    p.bon[2] = (int)bget(w[2], 0);
    p.bon[3] = (int)bget(w[2], 1);
    p.bon[4] = (int)bget(w[2], 2);
    p.pres = (int)bget(w[2], 3);
    p.nres = (int)(w[3] & 3u);
    p.rev = (int)((w[3] >> 2) & 7u);
#pragma unroll
    for (int i = 0; i < 3; ++i) p.res[i] = (int)bget(w[3], i + 1);
    return p;
}

__device__ __forceinline__ void pack_pl(const Pl &p, uint32_t w[4]) {
#ifdef SPL_BOUNDS_CHECK
    for (int c = 0; c < 6; ++c) SPL_CHECK(p.tok[c] >= 0 && p.tok[c] <= 255, BC_BYTE);
    for (int c = 0; c < 5; ++c) SPL_CHECK(p.bon[c] >= 0 && p.bon[c] <= 255, BC_BYTE);
    SPL_CHECK(p.pres >= 0 && p.pres <= 255 && p.nres >= 0 && p.nres <= 3, BC_BYTE);
#endif
    w[0] = (uint32_t)p.tok[0] | ((uint32_t)p.tok[1] << 8) | ((uint32_t)p.tok[2] << 16) | ((uint32_t)p.tok[3] << 24);
    w[1] = (uint32_t)p.tok[4] | ((uint32_t)p.tok[5] << 8) | ((uint32_t)p.bon[0] << 16) | ((uint32_t)p.bon[1] << 24);
    w[2] = (uint32_t)p.bon[2] | ((uint32_t)p.bon[3] << 8) | ((uint32_t)p.bon[4] << 16) | ((uint32_t)p.pres << 24);
    w[3] = ((uint32_t)p.nres & 3u) | (((uint32_t)p.rev & 7u) << 2) | (((uint32_t)p.res[0] & 0xFFu) << 8) |
           (((uint32_t)p.res[1] & 0xFFu) << 16) | (((uint32_t)p.res[2] & 0xFFu) << 24);
}

template <int P>
__device__ __forceinline__ void get_player(const Tab<P> &T, int p, uint32_t w[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // launder every player's word first: an asm inside the select would be executed
        // conditionally, i.e. compiled into one branch per word
        uint32_t o[P];
#pragma unroll
        for (int q = 0; q < P; ++q) o[q] = opaque(T.pw[q][k]);
        uint32_t v = o[0];
#pragma unroll
        for (int q = 1; q < P; ++q) v = (p == q) ? o[q] : v;
        w[k] = v;
    }
}

template <int P>
__device__ __forceinline__ void put_player(Tab<P> &T, int p, const uint32_t w[4]) {
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) T.pw[q][k] = (p == q) ? w[k] : T.pw[q][k];
}

__device__ __forceinline__ void get_bank(const uint32_t *sw, int bank[6]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) bank[c] = (int)bget(sw[SW_BANK0], c);
    bank[4] = (int)bget(sw[SW_BANK1], 0);
    bank[5] = (int)bget(sw[SW_BANK1], 1);
}

__device__ __forceinline__ void put_bank(uint32_t *sw, const int bank[6]) {
#ifdef SPL_BOUNDS_CHECK
    for (int c = 0; c < 6; ++c) SPL_CHECK(bank[c] >= 0 && bank[c] <= 255, BC_BYTE);
#endif
    sw[SW_BANK0] = (uint32_t)bank[0] | ((uint32_t)bank[1] << 8) | ((uint32_t)bank[2] << 16) | ((uint32_t)bank[3] << 24);
    sw[SW_BANK1] = (sw[SW_BANK1] & 0xFFFF0000u) | (uint32_t)bank[4] | ((uint32_t)bank[5] << 8);
}

__device__ __forceinline__ int board_get(const uint32_t *sw, int k) {  // runtime k
    const uint32_t b0 = opaque(sw[SW_BOARD]), b1 = opaque(sw[SW_BOARD + 1]), b2 = opaque(sw[SW_BOARD + 2]);
    const uint32_t w = k < 4 ? b0 : (k < 8 ? b1 : b2);
    return (int)bget(w, k & 3);
}
__device__ __forceinline__ void board_set(uint32_t *sw, int k, uint32_t v) {  // runtime k
#pragma unroll
    for (int t = 0; t < 3; ++t) sw[SW_BOARD + t] = (k >> 2) == t ? bset(sw[SW_BOARD + t], k & 3, v) : sw[SW_BOARD + t];
}

__device__ __forceinline__ uint4 card_rec(const Consts &L, int id) { return L.cards[id < 90 ? id : 0]; }

__device__ __forceinline__ int card_cost(uint4 rec, int c) { return c < 4 ? (int)bget(rec.z, c) : (int)bget(rec.w, 0); }

// Packed 16-bit arithmetic for per-colour comparisons: two colours per dword, saturating
// subtraction in one v_pk_sub_u16 (clamp).  Byte fields are widened with one v_perm_b32.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t sat_sub16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a),
                                                                      __builtin_bit_cast(u16x2, b)));
}
// bytes i and j of w as the low and high 16-bit halves
__device__ __forceinline__ uint32_t widen2(uint32_t w, int i, int j) {
    return __builtin_amdgcn_perm(0u, w, 0x0C000C00u | ((uint32_t)j << 16) | (uint32_t)i);
}

// what the player can put toward each colour: tokens + bonuses, packed (w|b, g|r, k) + gold
struct Have {
    uint32_t wb, gr, k;
    int gold;
};
__device__ __forceinline__ Have have_of(const Pl &p) {
    Have h;
    h.wb = (uint32_t)(p.tok[0] + p.bon[0]) | ((uint32_t)(p.tok[1] + p.bon[1]) << 16);
    h.gr = (uint32_t)(p.tok[2] + p.bon[2]) | ((uint32_t)(p.tok[3] + p.bon[3]) << 16);
    h.k = (uint32_t)(p.tok[4] + p.bon[4]);
    h.gold = p.tok[5];
    return h;
}

// engine/state.py:61-71 can_afford: sum over colours of max(cost - bonus - tokens, 0) <= gold
// (max(max(cost - bonus, 0) - tokens, 0) == max(cost - bonus - tokens, 0) for tokens >= 0)
__device__ __forceinline__ bool afford(const Have &h, uint4 rec) {
    const uint32_t s = sat_sub16(widen2(rec.z, 0, 1), h.wb) + sat_sub16(widen2(rec.z, 2, 3), h.gr);
    const int need = (int)(s & 0xFFFFu) + (int)(s >> 16) + max((int)bget(rec.w, 0) - (int)h.k, 0);
    return h.gold >= need;
}

// engine/rules.py:40-93 legal_moves -> 45-bit mask
__device__ __forceinline__ uint64_t legal_mask(const uint32_t *sw, const Pl &p, const int bank[6], const Consts &L) {
    uint32_t avail = 0;
#pragma unroll
    for (int c = 0; c < 5; ++c) avail |= (bank[c] >= 1 ? 1u : 0u) << c;
    const int nav = __popc(avail);
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {  // :45-58 reduced take-3 rule
        const uint32_t cm = take3_mask(i);
        const bool ok = nav >= 3 ? ((cm & avail) == cm) : (nav >= 1 && (avail & cm) == avail);
        m |= (uint64_t)ok << i;
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) m |= (uint64_t)(bank[c] >= 4) << (10 + c);  // :61-63
    const bool can_res = p.nres < 3;
    const Have h = have_of(p);
    // every card record is read unconditionally (missing cards read record 0) and combined with
    // bitwise ops: `present && afford(card_rec(...))` compiled into 15 branches, each an LDS read
    // followed by its own lgkmcnt(0) wait — 15 serial LDS round trips per legal mask
    uint4 rec[15];
#pragma unroll
    for (int k = 0; k < 12; ++k) rec[k] = card_rec(L, (int)bget(sw[SW_BOARD + k / 4], k % 4));
#pragma unroll
    for (int i = 0; i < 3; ++i) rec[12 + i] = card_rec(L, p.res[i]);
#pragma unroll
    for (int k = 0; k < 12; ++k) {  // :66-80
        const uint32_t present = bget(sw[SW_BOARD + k / 4], k % 4) != 0xFFu ? 1u : 0u;
        const uint32_t aff = afford(h, rec[k]) ? 1u : 0u;
        m |= (uint64_t)(present & aff) << (15 + k);
        m |= (uint64_t)(present & (can_res ? 1u : 0u)) << (27 + k);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) m |= (uint64_t)(can_res && bget(sw[SW_DECK], t) > 0) << (39 + t);  // :83-86
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // :89-91
        const uint32_t held = i < p.nres ? 1u : 0u;
        const uint32_t aff = afford(h, rec[12 + i]) ? 1u : 0u;
        m |= (uint64_t)(held & aff) << (42 + i);
    }
    return m;
}

// engine/rules.py:40-93 restricted to one action (the env only needs mask[a]) ...
__device__ __forceinline__ bool action_legal(const uint32_t *sw, const Pl &p, const int bank[6], int a,
                                             const Consts &L) {
    if (a < 10) {
        uint32_t avail = 0;
#pragma unroll
        for (int c = 0; c < 5; ++c) avail |= (bank[c] >= 1 ? 1u : 0u) << c;
        const int nav = __popc(avail);
        const uint32_t cm = take3_mask(a);
        return nav >= 3 ? ((cm & avail) == cm) : (nav >= 1 && (avail & cm) == avail);
    }
    if (a < 15) {
        const int c = a - 10;
        const int b = c == 0 ? bank[0] : (c == 1 ? bank[1] : (c == 2 ? bank[2] : (c == 3 ? bank[3] : bank[4])));
        return b >= 4;
    }
    if (a < 27) {
        const int id = board_get(sw, a - 15);
        return id != 0xFF && afford(have_of(p), card_rec(L, id));
    }
    if (a < 39) return p.nres < 3 && board_get(sw, a - 27) != 0xFF;
    if (a < 42) return p.nres < 3 && bget(sw[SW_DECK], a - 39) > 0;
    const int i = a - 42;
    const int r0 = opaque(p.res[0]), r1 = opaque(p.res[1]), r2 = opaque(p.res[2]);
    return i < p.nres && afford(have_of(p), card_rec(L, i == 0 ? r0 : (i == 1 ? r1 : r2)));
}

// ... and whether ANY move is legal: with a non-gold colour in the bank some take-3 always is
// (rules.py:45-58), otherwise fall back to the full mask (rare).
__device__ __forceinline__ bool any_legal(const uint32_t *sw, const Pl &p, const int bank[6], const Consts &L) {
    const bool some_colour = bank[0] > 0 || bank[1] > 0 || bank[2] > 0 || bank[3] > 0 || bank[4] > 0;
    return some_colour || legal_mask(sw, p, bank, L) != 0ull;
}

// engine/rules.py:101-122 _pay_for_card
__device__ __forceinline__ void pay_for_card(Pl &p, int bank[6], uint4 rec) {
    const int gold_avail = p.tok[5];
    int gold_spent = 0;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const int disc = max(card_cost(rec, c) - p.bon[c], 0);
        const int spend = min(p.tok[c], disc);
        p.tok[c] -= spend;
        bank[c] += spend;
        const int rem = disc - spend;
        gold_spent += rem > 0 ? min(rem, gold_avail - gold_spent) : 0;
    }
    p.tok[5] -= gold_spent;
    bank[5] += gold_spent;
    const int colour = (int)bget(rec.w, 1);
#pragma unroll
    for (int c = 0; c < 5; ++c) p.bon[c] += colour == c ? 1 : 0;
    p.pres += (int)bget(rec.x, 2);
}

__device__ __forceinline__ uint8_t *slot_rec(const KArena &A, int t, int slot) {
    SPL_CHECK(t >= 0 && t < A.n, BC_TABLE);
    SPL_CHECK(slot >= 0 && slot < kSlotRecords, BC_SLOT);
    return A.slots + ((size_t)t * kSlotRecords + slot) * kSlotBytes;
}
// slot-record ring status (spl_layout.h)
__device__ __forceinline__ int active_of(uint32_t misc) { return (int)((misc >> ST_ACTIVE_SHIFT) & 3u); }
__device__ __forceinline__ int pend_of(uint32_t misc) { return (int)((misc >> ST_PEND_SHIFT) & 3u); }
__device__ __forceinline__ uint32_t ring_bits(int active, int pend) {
    return ((uint32_t)active << ST_ACTIVE_SHIFT) | ((uint32_t)pend << ST_PEND_SHIFT);
}
__device__ __forceinline__ const uint8_t *live_rec(const KArena &A, int t, uint32_t misc) {
    return slot_rec(A, t, active_of(misc));
}

// engine/rules.py:125-129 _refill_slot / deck.pop() of tier t.  `top` is the card at
// deck_len-1 of that tier, gathered from the live record at the top of the step (one action
// pops at most one card, from the tier the action names: pop_tier()).
__device__ __forceinline__ uint32_t deck_pop(uint32_t *sw, uint32_t top, int t) {
    const int len = (int)bget(sw[SW_DECK], t);
    if (len <= 0) return 0xFFu;
    sw[SW_DECK] = bset(sw[SW_DECK], t, (uint32_t)(len - 1));
    return top;
}

// legal_moves of every fresh deal (engine/rules.py:40-93 on state.py:181-211's table): every
// take-3 and take-2 (bank 4 of each colour), every visible and blind reserve, no purchase — as long as
// every card costs something.  A context whose card table has a free card (kTagFreeCard) never
// publishes the constant: its reset lanes evaluate legal_moves of the dealt state (fresh_deal_mask,
// or the deferred evaluation of step_ws).
constexpr uint64_t kFreshDealMask = ((1ull << 15) - 1ull) | (((1ull << 15) - 1ull) << 27);

// tier an action pops from: buy visible (:216-225) and reserve visible (:226-240) refill the
// slot's tier, reserve blind (:241-249) draws from its tier; -1 for every other action
__device__ __forceinline__ int pop_tier(int a) {
    return (a >= 15 && a < 27) ? (a - 15) >> 2 : ((a >= 27 && a < 39) ? (a - 27) >> 2 : ((a >= 39 && a < 42) ? a - 39 : -1));
}

// pick the r-th colour (ascending) among non-gold colours the player holds
__device__ __forceinline__ void return_one(Pl &p, int bank[6], int r) {
    int seen = 0;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const bool has = p.tok[c] > 0;
        const bool hit = has && seen == r;
        p.tok[c] -= hit ? 1 : 0;
        bank[c] += hit ? 1 : 0;
        seen += has ? 1 : 0;
    }
}

__device__ __forceinline__ int non_gold_kinds(const Pl &p) {
    int n = 0;
#pragma unroll
    for (int c = 0; c < 5; ++c) n += p.tok[c] > 0 ? 1 : 0;
    return n;
}

// engine/rules.py:150-185 auto_return_tokens on the full CPython MT stream (rare: seeds
// outside the precomputed table, or a table entry that ran out of draws).
__device__ __forceinline__ void token_return_mt(Pl &p, int bank[6], int remaining, uint64_t seed, uint32_t *mtx) {
    MTStream ms;
    ms.init(seed);
    bool done = false;
    auto draw = [&](uint32_t y) {  // rng.choice(choices) on output y
        const int nch = non_gold_kinds(p);
        const int kb = bit_length((uint32_t)nch);
        const int r = (int)(y >> (32 - kb));
        if (r < nch) {  // accepted
            return_one(p, bank, r);
            remaining -= 1;
        }
    };
    const int limit = min(g_stream_limit, MTStream::kMaxOut);
    for (int j = 0;; ++j) {
        done = done || remaining <= 0 || non_gold_kinds(p) == 0;
        if (!__any(!done)) break;
        if (j >= limit) break;  // lanes still returning continue below
        const uint32_t y = ms.next(j);
        if (!done) draw(y);
    }
    // Continuation past the streamed outputs (crafted states with hundreds of tokens to return):
    // one lane at a time, its full MT19937 state in the LDS region mtx, from output kMaxOut on.
    for (uint64_t slow = __ballot(!done); slow; slow &= slow - 1) {
        if (lane_id() == __ffsll((unsigned long long)slow) - 1) {
            LaneMT mt{mtx, 0};
            mt.init(seed);
            mt.start_at(limit);
            while (remaining > 0 && non_gold_kinds(p) > 0) draw(mt.next());
        }
    }
    if (remaining > 0 && p.tok[5] > 0) {
        const int give = min(remaining, p.tok[5]);
        p.tok[5] -= give;
        bank[5] += give;
    }
}

// token-return table index of (turn_count, to_play, sum(tokens), sum(bank)), -1 outside it
__device__ __forceinline__ int lut_key(int turn_count, int to_play, int total, int bank_total) {
    const bool in_lut = turn_count < kLutTc && to_play < kLutTp && total >= 11 && total <= 13 && bank_total < kLutSb;
    return in_lut ? ((turn_count * kLutTp + to_play) * kLutSt + (total - 11)) * kLutSb + bank_total : -1;
}

// The table entry action `a` will consult, predicted from the pre-action state so its load
// can start with the state loads: takes and reserves move tokens bank -> player exactly as
// apply_action does; buys only lower the mover's total (-1: no prediction).
__device__ __forceinline__ int predict_lut_key(const Pl &p, const int bank[6], int a, int turn_count, int to_play) {
    int total = 0, bank_total = 0, delta = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        total += p.tok[c];
        bank_total += bank[c];
    }
    if (a < 10) {
        const uint32_t cm = take3_mask(a);
#pragma unroll
        for (int c = 0; c < 5; ++c) delta += (((cm >> c) & 1u) && bank[c] >= 1) ? 1 : 0;
    } else if (a < 15) {
        delta = 2;
    } else if (a >= 27 && a < 42) {
        delta = bank[5] > 0 ? 1 : 0;
    } else {
        return -1;
    }
    return total + delta > 10 ? lut_key(turn_count, to_play, total + delta, bank_total - delta) : -1;
}

// engine/rules.py:150-185 auto_return_tokens on the table entry `e` (top 3 bits of the first
// 40 outputs of the seeded stream, 10 per word).  One draw per iteration for every lane still
// returning: rng.choice -> _randbelow(n) takes the top bit_length(n) bits of one output and
// rejects r >= n; an accepted r returns one token of the r-th held non-gold colour.  The loop
// exit is wave-uniform and the body predicated, so divergent rejection counts cost no nested
// control flow.  Returns false if the lane needs more than the table's 40 outputs.
__device__ __forceinline__ bool token_return_lut(Pl &p, int bank[6], int remaining, uint4 e) {
    // On this path the mover holds 11..13 tokens, so every count fits a nibble: `tk` holds the
    // five non-gold counts, `list` the held colours in ascending order (CPython's `choices`
    // list, rebuilt after every draw in the reference) and `n` its length.  A draw reads the
    // r-th entry of the list; a colour that runs out is cut out of it.  All 32-bit ops.
    uint32_t tk = 0, list = 0;
    int n = 0;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        tk |= (uint32_t)p.tok[c] << (4 * c);
        const bool has = p.tok[c] > 0;
        list |= has ? (uint32_t)c << (4 * n) : 0u;
        n += has ? 1 : 0;
    }
    bool active = remaining > 0 && n > 0;
    // every lane draws at the same position, so the output word and bit offset are uniform
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t w = q == 0 ? e.x : (q == 1 ? e.y : (q == 2 ? e.z : e.w));
#pragma unroll 1
        for (int j = 0; j < 10; ++j) {
            if (!__any(active)) goto drawn;
            // _randbelow(n): top bit_length(n) of the 3 stored bits; shift 3 - bit_length(n)
            // for n = 1..5 is 2, 1, 1, 0, 0 (nibbles of 0x1120)
            const uint32_t r = __builtin_amdgcn_ubfe(w, 3u * (uint32_t)j, 3u) >> ((0x1120u >> (4 * n)) & 15u);
            const bool acc = active && (int)r < n;
            const uint32_t c4 = 4u * __builtin_amdgcn_ubfe(list, 4u * r, 4u);  // nibble of the colour in tk
            tk -= acc ? (1u << c4) : 0u;
            const bool out = acc && ((tk >> c4) & 15u) == 0u;
            const uint32_t low = (1u << (4u * r)) - 1u;  // cut entry r out of the list
            list = out ? ((list & low) | ((list >> ((4u * r + 4u) & 31u)) << (4u * r))) : list;
            n -= out ? 1 : 0;
            remaining -= acc ? 1 : 0;
            active = active && remaining > 0 && n > 0;
        }
    }
drawn:
    if (remaining > 0 && n > 0) return false;  // table outputs exhausted
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const int now = (int)((tk >> (4 * c)) & 15u);
        bank[c] += p.tok[c] - now;
        p.tok[c] = now;
    }
    if (remaining > 0 && p.tok[5] > 0) {              // :179-184 then gold
        const int give = min(remaining, p.tok[5]);
        p.tok[5] -= give;
        bank[5] += give;
    }
    return true;
}

// engine/rules.py:188-193 _enforce_token_limit -> :150-185 auto_return_tokens.  `pre_key` /
// `pre_e` are the prefetched table entry (predict_lut_key); any other key is loaded here.
__device__ __forceinline__ void enforce_token_limit(Pl &p, int bank[6], int turn_count, int to_play,
                                                    const uint4 *lut, int pre_key, uint4 pre_e, uint32_t *mtx) {
    int total = 0, bank_total = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) total += p.tok[c];
    if (total <= 10) return;
#pragma unroll
    for (int c = 0; c < 6; ++c) bank_total += bank[c];
    const int key = lut_key(turn_count, to_play, total, bank_total);
    const bool in_lut = key >= 0;
    bool need_mt = !in_lut;
    if (in_lut) {
        SPL_CHECK(key < kLutEntries, BC_LUT);
        const uint4 e = key == pre_key ? pre_e : lut[key];
        Pl p2 = p;
        int bank2[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) bank2[c] = bank[c];
        if (token_return_lut(p2, bank2, total - 10, e)) {
            p = p2;
#pragma unroll
            for (int c = 0; c < 6; ++c) bank[c] = bank2[c];
        } else {
            need_mt = true;
        }
    }
    if (need_mt) {
        const uint64_t seed = ((uint64_t)turn_count * 1315423911ull) ^ ((uint64_t)to_play * 2654435761ull) ^
                              ((uint64_t)total * 97531ull) ^ ((uint64_t)bank_total * 31337ull);
        token_return_mt(p, bank, total - 10, seed, mtx);
    }
}

// engine/rules.py:132-147 _grant_noble_if_applicable (first visible noble in slot order)
__device__ __forceinline__ void grant_noble(uint32_t *sw, Pl &p, int to_play, const Consts &L) {
    const int nn = (int)bget(sw[SW_DECK], 3);
    uint32_t owners = (sw[SW_NOB1] >> 8) & 0x7FFFu;
    bool granted = false;
    const uint32_t bon_wb = (uint32_t)p.bon[0] | ((uint32_t)p.bon[1] << 16);
    const uint32_t bon_gr = (uint32_t)p.bon[2] | ((uint32_t)p.bon[3] << 16);
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int idx = s < 4 ? (int)bget(sw[SW_NOB0], s) : (int)bget(sw[SW_NOB1], 0);
        const bool visible = s < nn && ((owners >> (3 * s)) & 7u) == 0 && idx < 10;
        const uint2 rec = L.nobles[idx < 10 ? idx : 0];
        // requirement minus bonus, saturated, is zero in every colour
        const uint32_t req_wb = widen2(rec.x, 1, 2);
        const uint32_t req_gr = __builtin_amdgcn_perm(rec.y, rec.x, 0x0C040C03u);  // x.byte3 | y.byte0
        const bool meets = (sat_sub16(req_wb, bon_wb) | sat_sub16(req_gr, bon_gr)) == 0u &&
                           (int)bget(rec.y, 1) <= p.bon[4];
        const bool take = !granted && visible && meets;
        owners |= take ? ((uint32_t)(to_play + 1) << (3 * s)) : 0u;
        p.pres += take ? (int)bget(rec.y, 2) : 0;
        granted = granted || take;
    }
    sw[SW_NOB1] = (sw[SW_NOB1] & 0xFFu) | (owners << 8);
}

// engine/rules.py:290-303 compute_winner: key (prestige, -cards, -reserved); tie of the top
// two keys -> None
template <int P>
__device__ __forceinline__ int compute_winner(const Tab<P> &T) {
    // track the top two keys as values (a runtime-indexed key[] array would go to scratch)
    int best = -1;
    uint32_t kbest = 0, ksecond = 0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const Pl p = unpack_pl(T.pw[q]);
        const int nb = p.bon[0] + p.bon[1] + p.bon[2] + p.bon[3] + p.bon[4];
        const uint32_t key = ((uint32_t)p.pres << 16) | ((uint32_t)(1023 - nb) << 4) | (uint32_t)(15 - p.nres);
        if (q == 0) {
            best = 0;
            kbest = key;
        } else if (key >= kbest) {
            ksecond = kbest;
            kbest = key;
            best = q;
        } else if (q == 1 || key >= ksecond) {
            ksecond = key;
        }
    }
    return kbest == ksecond ? -1 : best;
}

__device__ __forceinline__ int get_to_play(const uint32_t *sw) { return (int)bget(sw[SW_BANK1], 2); }
__device__ __forceinline__ int get_turn(const uint32_t *sw) { return (int)bget(sw[SW_BANK1], 3); }
__device__ __forceinline__ int get_moves(const uint32_t *sw) { return (int)(sw[SW_MISC] & 0xFFFFu); }
__device__ __forceinline__ int get_winner(const uint32_t *sw) { return (int)(sw[SW_MISC] >> 24) - 1; }
__device__ __forceinline__ bool is_terminal(const uint32_t *sw) {
    return (sw[SW_MISC] & ST_GAME_OVER) && get_to_play(sw) == 0;
}

// engine/rules.py:196-287 apply_action on the current player (action known legal)
template <int P, class Stamp>
__device__ __forceinline__ void apply_action(Tab<P> &T, int a, uint32_t top, const Consts &L, const uint4 *lut,
                                             int pre_key, uint4 pre_e, uint32_t *mtx, Stamp stamp) {
    uint32_t *sw = T.sw;
    const int tp = get_to_play(sw);
    uint32_t w[4];
    get_player(T, tp, w);
    Pl p = unpack_pl(w);
    int bank[6];
    get_bank(sw, bank);
    if (a < 10) {  // :201-210 take-3 (only colours still in the bank)
        const uint32_t cm = take3_mask(a);
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const bool take = ((cm >> c) & 1u) && bank[c] >= 1;
            bank[c] -= take ? 1 : 0;
            p.tok[c] += take ? 1 : 0;
        }
    } else if (a < 15) {  // :211-215 take-2
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            bank[c] -= (a - 10) == c ? 2 : 0;
            p.tok[c] += (a - 10) == c ? 2 : 0;
        }
    } else if (a < 27) {  // :216-225 buy visible, refill
        const int k = a - 15;
        pay_for_card(p, bank, card_rec(L, board_get(sw, k)));
        board_set(sw, k, deck_pop(sw, top, k >> 2));
    } else if (a < 39) {  // :226-240 reserve visible, gold if any, refill
        const int k = a - 27;
        const int card = board_get(sw, k);
#pragma unroll
        for (int i = 0; i < 3; ++i) p.res[i] = p.nres == i ? card : p.res[i];
        p.rev |= 1 << p.nres;
        p.nres += 1;
        const bool gold = bank[5] > 0;
        bank[5] -= gold ? 1 : 0;
        p.tok[5] += gold ? 1 : 0;
        board_set(sw, k, deck_pop(sw, top, k >> 2));
    } else if (a < 42) {  // :241-249 reserve blind (hidden), gold if any
        const int card = (int)deck_pop(sw, top, a - 39);
#pragma unroll
        for (int i = 0; i < 3; ++i) p.res[i] = p.nres == i ? card : p.res[i];
        p.rev &= ~(1 << p.nres);
        p.nres += 1;
        const bool gold = bank[5] > 0;
        bank[5] -= gold ? 1 : 0;
        p.tok[5] += gold ? 1 : 0;
    } else {  // :250-255 buy reserved: list.pop(i) shifts later slots
        const int i = a - 42;
        const int r0 = opaque(p.res[0]), r1 = opaque(p.res[1]), r2 = opaque(p.res[2]);
        const int card = i == 0 ? r0 : (i == 1 ? r1 : r2);
        p.res[0] = i == 0 ? r1 : r0;
        p.res[1] = i <= 1 ? r2 : r1;
        p.res[2] = 0xFF;
        p.rev = (p.rev & ((1 << i) - 1)) | ((p.rev >> (i + 1)) << i);
        p.nres -= 1;
        pay_for_card(p, bank, card_rec(L, card));
    }
    stamp(8);
    if (!abl(ABL_NOBLE)) grant_noble(sw, p, tp, L);                         // :260
    stamp(9);
    if (!abl(ABL_TOKLIM)) enforce_token_limit(p, bank, get_turn(sw), tp, lut, pre_key, pre_e, mtx);  // :261
    stamp(10);
    uint32_t misc = sw[SW_MISC];
    if (p.pres >= 15) misc |= ST_GAME_OVER;                                 // :264-265
    pack_pl(p, w);
    put_player(T, tp, w);
    put_bank(sw, bank);
    const int moves = (int)(misc & 0xFFFFu) + 1;                            // :268-272
    const int ntp = (tp + 1) % P;
    const int turn = moves / 2 + 1;
    misc = (misc & 0xFFFF0000u) | (uint32_t)moves;
    sw[SW_BANK1] = (sw[SW_BANK1] & 0x0000FFFFu) | ((uint32_t)ntp << 16) | ((uint32_t)min(turn, 255) << 24);
    if (turn >= 100) {                                                      // :275-279
        misc |= ST_GAME_OVER | ST_TURN_LIMIT;
        misc &= 0x00FFFFFFu;  // winner None
    } else if ((misc & ST_GAME_OVER) && ntp == 0) {                         // :282-285
        sw[SW_MISC] = misc;
        const int wnr = compute_winner(T);
        misc = (misc & 0x00FFFFFFu) | ((uint32_t)(wnr + 1) << 24);
    }
    sw[SW_MISC] = misc;
}

}  // namespace spl
