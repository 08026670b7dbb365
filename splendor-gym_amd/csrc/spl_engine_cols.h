#pragma once
// spl_engine_cols.h — a terminal table's final_observation row encoded by the whole wave, column-parallel: the
// CK_* kinds, the per-lane recipes built once per launch (col_recipe, ColRecipes) and the row from a table's state
// words in LDS (row_columns, store_row_columns).  The same fields as spl_engine_obs.h's build_row.
#include "spl_engine_args.h"
#include "spl_engine_base.h"
#include "spl_layout.h"

namespace spl {

// ---- column-parallel rows (round 4) --------------------------------------------------------
// A terminal table's info["final_observation"] row encoded by the whole wave: lane l owns bytes
// e = l + 64 i (i < 5) of the ONE row and stores them as int32, coalesced (five 256-byte dword
// stores).  encode_row's lane-per-row form costs every lane a whole row even when one or two of the
// wave's 64 tables ended (random 4-player games end every ~30 steps: most steps), which made the
// 4-player output wave's encode 4.4 us against 2.6 us at 2 players.  Here a byte is one or two LDS
// reads plus a few VALU ops, driven by a per-lane recipe built once per launch (col_recipe): which
// state word holds it (absolute, or a word of the player to move / the next player), which byte of
// that word, and whether it names a card / noble whose record byte is the value
// (engine/encode.py:124-187; the same fields as build_row).
enum : uint32_t {
    CK_BYTE = 0,      // the byte itself
    CK_NRES = 1,      // & 3 (n_reserved of PW3)
    CK_BOARD = 2,     // board card id -> record byte f (0 when the slot is empty)
    CK_OWN_RES = 3,   // own reserved card slot s (PW3 byte s + 1) -> record byte f, f == 13: present
    CK_OPP_RES = 4,   // opponent's reserved slot s: as own, hidden (not revealed) -> zeros
    CK_NOBLE = 5,     // visible noble slot s (SW_NOB0 byte s) -> noble record byte f
    CK_MOVES = 6,     // move_count, the full value (no byte patch needed)
    CK_TERMINAL = 7,  // game_over and to_play == 0
    CK_NONE = 8       // past the row
};
// recipe: word (5 bits) | rel << 5 (0 absolute, 1 to_play's PW, 2 next player's PW) | byte << 7 |
//         kind << 9 | f << 13 | s << 17
__device__ __forceinline__ uint32_t col_recipe(int e) {
    auto R = [](int w, int rel, int b, uint32_t kind, int f = 0, int s = 0) {
        return (uint32_t)w | ((uint32_t)rel << 5) | ((uint32_t)b << 7) | (kind << 9) | ((uint32_t)f << 13) |
               ((uint32_t)s << 17);
    };
    if (e >= kObsDim) return R(0, 0, 0, CK_NONE);
    if (e < 4) return R(SW_BANK0, 0, e, CK_BYTE);                                   // bank :128
    if (e < 6) return R(SW_BANK1, 0, e - 4, CK_BYTE);
    if (e < 32) {                                                                    // players :131-142
        const int rel = e < 19 ? 1 : 2, q = e - (e < 19 ? 6 : 19);
        return q < 12 ? R(q >> 2, rel, q & 3, CK_BYTE) : R(3, rel, 0, CK_NRES);
    }
    if (e < 188) {                                                                   // board :144-147
        const int k = (e - 32) / 13;
        return R(SW_BOARD + k / 4, 0, k % 4, CK_BOARD, (e - 32) % 13);
    }
    if (e < 272) {                                                                   // reserved :151-168
        const bool own = e < 230;
        const int q = e - (own ? 188 : 230), s = q / 14;
        return R(3, own ? 1 : 2, s + 1, own ? CK_OWN_RES : CK_OPP_RES, q % 14, s);
    }
    if (e < 290) {                                                                   // nobles[:3] :171-178
        const int s = (e - 272) / 6;
        return R(SW_NOB0, 0, s, CK_NOBLE, (e - 272) % 6, s);
    }
    if (e < 293) return R(SW_DECK, 0, e - 290, CK_BYTE);                            // deck sizes :180-181
    if (e == 293) return R(SW_BANK1, 0, 3, CK_BYTE);                                // turn_count :183
    if (e == 294) return R(SW_BANK1, 0, 2, CK_BYTE);                                // to_play :184
    if (e == 295) return R(SW_MISC, 0, 0, CK_MOVES);                                // move_count :185
    return R(SW_MISC, 0, 0, CK_TERMINAL);                                           // terminal :186
}
struct ColRecipes {
    uint32_t r[5];
};
__device__ __forceinline__ ColRecipes col_recipes() {
    ColRecipes c;
#pragma unroll
    for (int i = 0; i < 5; ++i) c.r[i] = col_recipe(lane_id() + 64 * i);
    return c;
}

// One table's observation row, column-parallel (wave-uniform call): word w of the table's state is
// st[w * stride] in LDS (st and stride uniform); v[i] = column lane + 64 i of the row.
template <int P>
__device__ __forceinline__ void row_columns(const uint32_t *st, int stride, const Consts &L, const ColRecipes &C,
                                            uint32_t (&v)[5]) {
    const uint32_t bank1 = st[SW_BANK1 * stride], misc = st[SW_MISC * stride];
    const int tp = (int)bget(bank1, 2), np = (tp + 1) % P;
    const uint32_t deck = st[SW_DECK * stride], owners = (st[SW_NOB1 * stride] >> 8) & 0x7FFFu;
    const uint8_t *cb = reinterpret_cast<const uint8_t *>(L.cards);
    const uint8_t *nb = reinterpret_cast<const uint8_t *>(L.nobles);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint32_t r = C.r[i];
        const int w0 = (int)(r & 31u), rel = (int)((r >> 5) & 3u), b = (int)((r >> 7) & 3u);
        const uint32_t kind = (r >> 9) & 15u;
        const int f = (int)((r >> 13) & 15u), s = (int)((r >> 17) & 3u);
        const int widx = rel == 0 ? w0 : pw_index(rel == 1 ? tp : np, w0);
        const uint32_t w = st[widx * stride];
        const uint32_t byte = bget(w, b);
        // the record byte a card / noble kind reads (address clamped: read unconditionally)
        const bool is_noble = kind == CK_NOBLE;
        const uint32_t id = byte < (is_noble ? 10u : 90u) ? byte : 0u;
        const uint32_t rec = is_noble ? (uint32_t)nb[id * 8 + (f < 6 ? f : 0)] : (uint32_t)cb[id * 16 + (f < 13 ? f : 0)];
        const int nres = (int)(w & 3u), rev = (int)((w >> 2) & 7u);
        const bool res_pr = s < nres && (kind == CK_OWN_RES || ((rev >> s) & 1));
        const bool nob_pr = s < (int)bget(deck, 3) && ((owners >> (3 * s)) & 7u) == 0u && byte < 10u;
        uint32_t out = byte;
        out = kind == CK_NRES ? (w & 3u) : out;
        out = kind == CK_BOARD ? (byte != 0xFFu ? rec : 0u) : out;
        out = (kind == CK_OWN_RES || kind == CK_OPP_RES) ? (res_pr ? (f == 13 ? 1u : rec) : 0u) : out;
        out = is_noble ? (nob_pr ? rec : 0u) : out;
        out = kind == CK_MOVES ? (misc & 0xFFFFu) : out;
        out = kind == CK_TERMINAL ? (((misc & ST_GAME_OVER) && tp == 0) ? 1u : 0u) : out;
        v[i] = out;
    }
}
template <int P>
__device__ __forceinline__ void store_row_columns(const uint32_t *st, int stride, const Consts &L, const ColRecipes &C,
                                                  int32_t *dst) {
    uint32_t v[5];
    row_columns<P>(st, stride, L, C, v);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int e = lane_id() + 64 * i;
        if (e < kObsDim) dst[e] = (int32_t)v[i];
    }
}

}  // namespace spl
