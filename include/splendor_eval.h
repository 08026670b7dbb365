/*
 * splendor_eval.h — C-ABI of the on-device evaluation league (gfx950): scripted opponents as a kernel
 * of their own, the per-table tally of an evaluation game and its reduction per opponent group.
 *
 * The reference evaluates through run_evaluation_suite (training_utils.py:237-260): --eval-games
 * games each against random, greedy_v1, basic_priority and the agent itself, one env step and one
 * batch-1 forward per ply.  These entry points let one batch of tables play every opponent kind at
 * once, each table against its own kind, with the statistics kept on the device:
 *
 *   spl_eval_scripted_act  the scripted opponents of scripts/eval_suite.py over a mask and an
 *                          observation: the three policies the step kernel fuses (same actions for the
 *                          same mask, state and (seed, table key, ply)) and greedy_v2 (:80-128), chosen
 *                          per table; tables of a network opponent are left alone
 *   spl_eval_check         before a dual step: the agent's choice against the mask it chose from
 *   spl_eval_tally         after a dual step: result, turns and prestige of the games that ended
 *   spl_eval_reduce        int64 [G][8] per opponent group
 *
 * Nothing here takes an engine context: the kernels read the step's outputs, not the table state, so
 * a turn of the league (agent act, spl_eval_check, spl_step, spl_eval_scripted_act, spl_step,
 * spl_dual_finish, spl_eval_tally) is a linear sequence of launches that a hipGraph can replay; the
 * ply of the scripted draws advances on the device (ply_base, e.g. spl_dual_io_t.step_counter).
 *
 * Conventions as in splendor_ppo.h: caller-owned device buffers as raw pointers, `stream` a
 * hipStream_t as void*, 0 / negative SPL_E_* returns (splendor_amd.h), spl_last_error() for the
 * message.  Argument errors are reported on the host before anything is launched.  Zero-initialise
 * every struct: a NULL optional member means skip.
 */
#ifndef SPLENDOR_EVAL_H
#define SPLENDOR_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPL_EVAL_ABI 1

/* policy ids of spl_eval_scripted_act beyond SPL_POLICY_UNIFORM / GREEDY_V1 / BASIC_PRIORITY (0, 1, 2:
 * splendor_amd.h; spl_step takes only those) */
#define SPL_POLICY_GREEDY_V2 3 /* eval_suite.py:80-128 with the bank read from the observation */
#define SPL_EVAL_KEEP (-1)     /* leave action[t] as it is (a network's choice)                   */

#define SPL_EVAL_OBS_U8 300 /* bytes of a compact observation row (spl_step_args_t.obs_u8) */
#define SPL_EVAL_COLS 8     /* columns of spl_eval_reduce's rows                            */

/* spl_eval_scripted_act.  The policies read the mask and the observation only: the bank is obs[0:5],
 * the points of visible card k obs[32 + 13k + 2].
 *   UNIFORM         a uniform legal action: the Philox word of (seed; key, ply) scaled to the legal count
 *   GREEDY_V1       lowest legal buy (15..26, 42..44), else take-2 (10..14), take-3 (0..9), reserve
 *                   (27..41), else the lowest legal action
 *   BASIC_PRIORITY  a uniform choice among the legal visible buys with the most points, else among the
 *                   reserved buys, take-3s, take-2s, reserves; else the lowest legal action
 *   GREEDY_V2       lowest legal buy, visible before reserved; else the legal take-2 whose colour has the
 *                   smallest bank count (first minimum); else the legal take-3 with the smallest bank sum
 *                   over its three colours (first minimum); else the highest legal reserve (27..41); else
 *                   the lowest legal action; deterministic
 * Every policy answers 0 on an empty mask.  key = table_key[t] if given, else table0 + t;
 * ply = ply + *ply_base (if given).  An id outside -1..3 writes nothing for its row and adds one to
 * *errors. */
typedef struct {
    const int8_t *mask;       /* [n][45], nonzero = legal, any alignment                             */
    const int32_t *obs;       /* [n][297], 4-byte aligned        } exactly one of the two            */
    const uint8_t *obs_u8;    /* [n][300], 4-byte aligned        }                                   */
    const int32_t *policy_of; /* [n], or NULL: `policy` for every row                                */
    const int64_t *table_key; /* [n], 8-byte aligned, or NULL: table0 + t                            */
    const int64_t *ply_base;  /* device scalar, 8-byte aligned, or NULL: 0                           */
    int32_t *action;          /* [n] out                                                             */
    uint64_t *errors;         /* device counter, 8-byte aligned, or NULL (bad ids are then only skipped) */
    uint64_t seed, ply;
    int64_t table0;
    int32_t policy;
    int32_t reserved; /* 0 */
} spl_eval_act_t;

/* spl_eval_check: where playing[t], checks[t] += 1 and, if action[t] is outside 0..44 or mask[t][action[t]]
 * is zero, illegal[t] += 1 (scripts/eval_suite.py:94-97: the choice against the mask it was made from). */
typedef struct {
    const int32_t *action;  /* [n]                                   */
    const int8_t *mask;     /* [n][45]                               */
    const uint8_t *playing; /* [n]                                   */
    int32_t *checks;        /* [n]                                   */
    int32_t *illegal;       /* [n]                                   */
} spl_eval_check_t;

/* spl_eval_tally: where playing[t] and done[t]
 *   result[t]   = sign(game_ended_on[t] == 1 ? agent_step_reward[t] : -opp_reward[t])   (-1, 0, 1)
 *   turns[t]    = final_obs[t][293], prestige[t] = final_obs[t][30]
 *   playing[t]  = 0
 * (the conventions of splendor_gym.evaluation.eval_vs_opponent).  The legality counters are
 * spl_eval_check's: the mask the agent chose from is overwritten by the step, and the step's flags do
 * not tell a choice outside an empty mask from the draw that follows it. */
typedef struct {
    const uint8_t *done;            /* [n] spl_dual_io_t.done                      */
    const int8_t *game_ended_on;    /* [n]                                         */
    const float *agent_step_reward; /* [n] the agent's step reward (phase A)       */
    const float *opp_reward;        /* [n]                                         */
    const int32_t *final_obs;       /* [n][297]                                    */
    uint8_t *playing;               /* [n] in / out                                */
    int8_t *result;                 /* [n]                                         */
    int32_t *turns, *prestige;      /* [n]                                         */
} spl_eval_tally_t;

/* spl_eval_reduce: out[g] = { wins, losses, draws, unfinished, sum turns, sum prestige, checks, illegal }
 * over the tables with group_of[t] == g (group_of NULL: every table is group 0).  wins / losses / draws
 * count finished tables (playing == 0) by result; unfinished counts playing != 0; the sums run over every
 * table of the group.  A table whose group is outside 0..G-1 is counted nowhere.  Integer sums: the same
 * bytes whatever the order.  One workgroup per group scans the n tables (G is a handful). */
typedef struct {
    const int32_t *group_of; /* [n] or NULL                       */
    const uint8_t *playing;  /* [n]                               */
    const int8_t *result;    /* [n]                               */
    const int32_t *turns, *prestige, *checks, *illegal; /* [n]    */
    int64_t *out;            /* [G][8], 8-byte aligned            */
} spl_eval_reduce_t;

int spl_eval_abi_version(void);
int spl_eval_scripted_act(int32_t n, const spl_eval_act_t *args, void *stream);
int spl_eval_check(int32_t n, const spl_eval_check_t *args, void *stream);
int spl_eval_tally(int32_t n, const spl_eval_tally_t *args, void *stream);
int spl_eval_reduce(int32_t n, int32_t G, const spl_eval_reduce_t *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLENDOR_EVAL_H */
