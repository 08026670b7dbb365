/*
 * splendor_search.h — C-ABI of the one-ply search primitives (gfx950): every table's 45 successors in one
 * launch, read-only on the arena, and the pick over their values.
 *
 * The reference answers "what would each legal move lead to?" on the host: apply_action returns a new state
 * (engine/rules.py:196-287) and greedy_opponent_v2 (scripts/eval_suite.py:80-128) is a hand-written look at
 * it.  Here the same question is one launch:
 *
 *   spl_successors    for every table t and action a: SplendorEnv.step(a) on a copy of table t (autoreset
 *                     off), its observation row, reward, end flags and next legal mask.  The arena is only
 *                     read: no state word, pool record, PCG stream or legal-mask cache entry changes, so a
 *                     trajectory is the same with or without the call.  The token-limit return is a function
 *                     of the state alone (its MT seed is built from turn, seat and token sums), so a
 *                     successor is the step's exact result, not a sample.
 *   spl_search_pick   argmax_a q(t, a) over the legal pairs, q = the reward where the move ended the game,
 *                     else sign * value (sign = -1 for the value of the NEXT player in a two-player game).
 *
 * A one-ply value policy is spl_successors (compact rows), spl_policy_act in SPL_ACT_VALUE mode over the
 * 45 n rows (include/splendor_policy.h, obs_u8) and spl_search_pick: three launches, no host work.
 *
 * SPL_SUCC_DREW marks the pairs whose move popped a non-empty deck: the successor row then shows a board
 * card (or, for the mover's own blind reserve, a reserved card) that the mover could not have known.  The
 * rows are the engine's truth; a caller that wants an honest look-ahead treats DREW rows accordingly.
 *
 * Conventions as in splendor_eval.h: caller-owned device buffers as raw pointers, `stream` a hipStream_t
 * as void*, 0 / negative SPL_E_* returns (splendor_amd.h), spl_last_error() for the message.  Argument
 * errors are reported on the host before anything is launched.  Both calls are asynchronous and may be
 * captured into a hipGraph.  Zero-initialise every struct: a NULL optional member means skip.
 */
#ifndef SPLENDOR_SEARCH_H
#define SPLENDOR_SEARCH_H

#include <stdint.h>

#include "splendor_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPL_SEARCH_ABI 1

/* bits of spl_succ_args_t.flags (its own set, not SPL_F_*) */
#define SPL_SUCC_LEGAL 0x01      /* t is a live table and a is legal there: the pair's outputs are a step's */
#define SPL_SUCC_TERMINATED 0x02 /* the move ended the game                                                */
#define SPL_SUCC_TURN_LIMIT 0x04 /* ... by the turn limit                                                  */
#define SPL_SUCC_DREW 0x08       /* the move popped a non-empty deck (see above)                           */

#define SPL_SUCC_OBS_U8 300 /* bytes of a compact row (spl_step_args_t.obs_u8) */

/* spl_successors.  Every output is action-major, [45][n]...: pair (t, a) is element a * n + t.  Every
 * element of every given output is written on every call; for a pair without SPL_SUCC_LEGAL (a table that
 * is over, an illegal action) the rows are zero bytes, flags and mask_bits 0, reward 0 and winner -1, so a
 * buffer's content after the call depends on the arena alone. */
typedef struct {
    uint8_t *obs_u8;     /* [45][n][300], 16-byte aligned       } at least one of the two                  */
    int32_t *obs;        /* [45][n][297], 16-byte aligned       }                                          */
    uint8_t *flags;      /* [45][n] SPL_SUCC_*                                                             */
    float *reward;       /* [45][n], 4-byte aligned: SplendorEnv.step's reward of the mover                */
    uint64_t *mask_bits; /* [45][n], 8-byte aligned, or NULL: legal_moves of the successor, 0 when over    */
    int8_t *winner;      /* [45][n], or NULL: the successor's winner, -1 for none                          */
} spl_succ_args_t;

/* spl_search_pick over the [45][n] planes flags, reward and value: per table
 *   q(a)   = flags & SPL_SUCC_TERMINATED ? reward : sign * value
 *   action = the legal a of greatest q, compared with q > best from best = -inf: a NaN never wins and the
 *            lowest a wins a tie; the first legal a if no comparison succeeds; -1 if none is legal
 *   best_q = the greatest q, -inf if no comparison succeeded */
typedef struct {
    const uint8_t *flags; /* [45][n]                                  */
    const float *reward;  /* [45][n], 4-byte aligned                  */
    const float *value;   /* [45][n], 4-byte aligned                  */
    int32_t *action;      /* [n] out, 4-byte aligned                  */
    float *best_q;        /* [n] out, 4-byte aligned, or NULL         */
    float sign;
    int32_t reserved; /* 0 */
} spl_pick_args_t;

int spl_search_abi_version(void);
int spl_successors(spl_ctx_t *ctx, spl_arena_t *arena, const spl_succ_args_t *args, void *stream);
int spl_search_pick(int32_t n, const spl_pick_args_t *args, void *stream);

/* ---- the ragged form: legal pairs only ------------------------------------------------------------------
 * About one pair in six is legal, so the dense planes are mostly rows nobody reads.  spl_successors_pairs
 * writes the legal pairs alone, compacted, and spl_search_pick_pairs picks over them.  SPL_SEARCH_ABI did not
 * move: a library that has the two calls says so with SPL_SEARCH_PAIRS.
 *
 * The order of the pairs is a function of the arena alone.  With B = 64-table block t / 64:
 *   pairs are sorted by (t / 64, a, t): block b's pairs are [base[b], base[b + 1]), inside it action a's pairs
 *   come before action a + 1's, each in table order.  So with ballot_b(a) = the block's tables that allow a,
 *     index(t, a) = base[t / 64] + sum over a' < a of popcount(ballot_b(a')) + rank of t in ballot_b(a),
 *   computable from `legal` and `base` alone, and the rows of one (block, action) are contiguous.
 * m = base[ceil(n / 64)] is the number of legal pairs.  If m > capacity nothing at an index >= capacity is
 * written in any plane, and a (block, action) run that does not fit whole below capacity is not written at
 * all; `legal` and `base` are complete all the same, so the host learns of the overflow from m, grows its
 * buffers and calls again (the arena was only read).  No fault word is raised. */
#define SPL_SEARCH_PAIRS 1

typedef struct {
    uint8_t *obs_u8;     /* [capacity][300], 16-byte aligned: compact rows                                 */
    uint8_t *flags;      /* [capacity] SPL_SUCC_* (SPL_SUCC_LEGAL is set in every one)                     */
    float *reward;       /* [capacity], 4-byte aligned                                                     */
    int32_t *pair;       /* [capacity], 4-byte aligned: the dense index a * n + t of the pair              */
    uint64_t *mask_bits; /* [capacity], 8-byte aligned, or NULL: as in spl_succ_args_t                     */
    int8_t *winner;      /* [capacity], or NULL: as in spl_succ_args_t                                     */
    uint64_t *legal;     /* [n], 8-byte aligned: legal_moves of table t's state, 0 for a table that is over */
    int32_t *base;       /* [ceil(n / 64) + 1], 4-byte aligned: exclusive prefix of the blocks' pair counts */
    int32_t capacity;    /* rows the buffers hold, >= 1                                                    */
} spl_succ_pairs_args_t;

/* spl_search_pick_pairs: spl_search_pick's semantics over the compacted planes.  A pair whose index is
 * >= capacity takes no part: it is neither compared nor the first legal action. */
typedef struct {
    const uint64_t *legal; /* [n], 8-byte aligned                      */
    const int32_t *base;   /* [ceil(n / 64) + 1], 4-byte aligned       */
    const uint8_t *flags;  /* [m]                                      */
    const float *reward;   /* [m], 4-byte aligned                      */
    const float *value;    /* [m], 4-byte aligned                      */
    int32_t *action;       /* [n] out, 4-byte aligned                  */
    float *best_q;         /* [n] out, 4-byte aligned, or NULL         */
    float sign;
    int32_t capacity; /* pairs the planes hold, >= 1 */
    int32_t reserved; /* 0 */
} spl_pick_pairs_args_t;

int spl_successors_pairs(spl_ctx_t *ctx, spl_arena_t *arena, const spl_succ_pairs_args_t *args, void *stream);
int spl_search_pick_pairs(int32_t n, const spl_pick_pairs_args_t *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLENDOR_SEARCH_H */
