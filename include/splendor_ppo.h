/*
 * splendor_ppo.h — C-ABI of the PPO rollout store (gfx950): record, GAE, minibatch gather, loss head
 * and optimiser step.
 *
 * The reference's learner (ppo_splendor.py:287-325) appends per-step numpy copies to Python lists,
 * runs GAE as a numpy loop on the host and re-uploads everything for the update.  These entry points
 * keep the agent's trajectory on the device in the engine's compact formats and reproduce the
 * reference's arithmetic:
 *
 *   spl_ppo_record   one step's rows into a step-major store (compact observation rows copied, the
 *                    int8 mask packed into 45-bit words, reward / done rows copied)
 *   spl_ppo_gae      the reverse scan of ppo_splendor.py:304-314, bit-equal to numpy, plus the
 *                    statistics ppo_splendor.py:325 normalises the advantages with
 *   spl_ppo_gather   one minibatch of flat positions, expanded into what
 *                    ActorCritic.get_action_and_value takes
 *   spl_ppo_loss     the loss head of the update (ppo_splendor.py:337-352) for one minibatch of flat
 *                    positions: the loss, its statistics and its gradients with respect to the actor's
 *                    logits and the critic's value, the recorded quantities read from the planes
 *   spl_ppo_adam     the optimiser step behind the backward pass (ppo_splendor.py:354-361): the
 *                    global-norm clip, torch.optim.Adam's step and the target-KL early stop, decided
 *                    on the device so that the host never waits for a minibatch's KL
 *   spl_ppo_net_forward / spl_ppo_net_backward   the actor's and the critic's passes around the loss
 *                    head, reading the observations from the store by position and writing the parameter
 *                    gradients where spl_ppo_adam reads them
 *
 * The store is step-major [K][T] (K steps, T tables), every plane caller-owned device memory:
 *   obs_u8     uint8  [K][T][300]  the compact rows of spl_step_args_t.obs_u8 (bytes 0..296 the values
 *                                  mod 256, byte 297 = move_count >> 8, bytes 298-299 zero)
 *   mask_bits  uint64 [K][T]       bit a set <=> action a legal (bits 0..44, the rest zero)
 *   action     int32  [K][T]
 *   logprob, value, reward  float32 [K][T]
 *   done       uint8  [K][T]       the dual step's `done`
 *   adv, ret   float32 [K][T]      written by spl_ppo_gae
 * action / logprob / value need no copy: spl_policy_act writes wherever it is pointed, so the
 * collector points it at row k of the store.
 *
 * Conventions as in splendor_policy.h: caller-owned device buffers as raw pointers, `stream` a
 * hipStream_t as void*, 0 / negative SPL_E_* returns, spl_last_error() for the message.  Argument
 * errors are reported on the host before anything is launched.
 */
#ifndef SPLENDOR_PPO_H
#define SPLENDOR_PPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPL_PPO_ABI 1

#define SPL_PPO_OBS_U8 300 /* bytes of a compact observation row */

/* spl_ppo_record: four source -> destination groups, each nullable as a pair (both NULL: the group
 * is skipped; one NULL: SPL_E_ARG; all four skipped: SPL_E_ARG).  Destinations are row k of the
 * store's planes. */
typedef struct {
    const uint8_t *obs_u8;   /* [n][300], 4-byte aligned                                            */
    uint8_t *dst_obs_u8;     /* [n][300], 4-byte aligned (16-byte aligned pairs move 16 bytes a lane) */
    const int8_t *mask;      /* [n][45] int8, nonzero = legal (spl_act_args_t.mask), any alignment   */
    uint64_t *dst_mask_bits; /* [n], 8-byte aligned                                                  */
    const float *reward;     /* [n], 4-byte aligned                                                  */
    float *dst_reward;       /* [n], 4-byte aligned                                                  */
    const uint8_t *done;     /* [n]                                                                  */
    uint8_t *dst_done;       /* [n]                                                                  */
} spl_ppo_record_t;

/* Statistics of the float32 advantages x (as the adv plane holds them), accumulated in float64 in a
 * fixed order (bit-identical from run to run):
 *   count = K * T, sum = SUM x, sumsq = SUM x*x
 *   mean  = sum / count
 *   var   = (sumsq - sum * mean) / (count - 1)      the n-1 denominator of torch.std; a negative var
 *   std   = sqrt(var < 0 ? 0 : var)                 (cancellation) counts as 0; count = 1 gives NaN
 *   mean32 = (float)mean, std32 = (float)std
 * every operation one IEEE float64 operation, left to right as written, none fused.  count, sum and
 * sumsq are what sharded stores all-reduce. */
typedef struct {
    uint64_t count;
    double sum, sumsq;
    double mean, std;
    float mean32, std32;
} spl_ppo_stats_t;

/* spl_ppo_gae: with r, v, v_next float32 and nnt = 1 - done[t] (v_next = last_value[table] at
 * t = K-1, value[t+1] otherwise; `last` starts at 0 and is carried unrounded):
 *   gv     = fp32( fp32(gamma) * v_next )
 *   delta  = (f64)r + (f64)gv * nnt - (f64)v        float64, left to right
 *   last   = delta + ((gamma * lambda) * nnt) * last      gamma * lambda multiplied once, in double
 *   adv[t] = fp32(last);  ret[t] = fp32(last + (f64)v) */
typedef struct {
    const float *reward;     /* [K][T]                                                               */
    const float *value;      /* [K][T]                                                               */
    const uint8_t *done;     /* [K][T], nonzero = the episode ended on this step                     */
    const float *last_value; /* [T]: the critic's value of the observation after step K-1            */
    float *adv, *ret;        /* [K][T] out                                                           */
    double gamma, lambda;    /* each in [0, 1]                                                       */
    spl_ppo_stats_t *stats;  /* out, device, 8-byte aligned                                          */
    void *scratch;           /* spl_ppo_gae_scratch_bytes(T) bytes, device, 8-byte aligned; no need to
                                clear it: every word read was written by the same call               */
} spl_ppo_gae_t;

/* spl_ppo_gather: row b of every output is the store's flat position idx[b] = k * T + t (duplicates
 * allowed).  A position outside [0, K*T) writes nothing for its row and adds one to *errors; its
 * address is never formed. */
typedef struct {
    int32_t K, T;
    int32_t normalize;            /* nonzero: adv = (adv - mean32) / (std32 + 1e-8f), each a correctly
                                     rounded float32 operation, mean32 / std32 read from *stats on the
                                     device; 0: the raw adv (stats may be NULL)                       */
    int32_t reserved;             /* 0                                                               */
    const int64_t *idx;           /* [B]                                                             */
    const uint8_t *obs_u8;        /* the store's planes: [K][T][300], 4-byte aligned                 */
    const uint64_t *mask_bits;    /* [K][T]                                                          */
    const int32_t *action;        /* [K][T]                                                          */
    const float *logprob, *value, *adv, *ret; /* [K][T]                                              */
    const spl_ppo_stats_t *stats;
    float *out_obs;               /* [B][297]: column 295 = byte 295 + 256 * byte 297, else its byte */
    float *out_mask;              /* [B][45]: 0.0 / 1.0                                              */
    int64_t *out_action;          /* [B]                                                             */
    float *out_logprob, *out_value, *out_adv, *out_ret; /* [B]                                       */
    uint64_t *errors;             /* device counter, incremented per bad position (never reset here) */
} spl_ppo_gather_t;

/* What spl_ppo_loss reports, on the device (56 bytes).  Every mean divides by B, bad rows included in
 * the divisor and left out of the sums:
 *   policy_loss = mean(-min(r A, clamp(r, 1-c, 1+c) A))     value_loss = mean(0.5 max((v-ret)^2, (v_c-ret)^2))
 *   entropy     = mean(H)                                   approx_kl  = mean(lp_old - lp)
 *   clipfrac    = mean(|r - 1| > c)                         loss = policy_loss + vf_coef value_loss + ent_coef entropy
 * loss32 = (float)loss; bad = the bad rows of this call. */
typedef struct {
    double loss, policy_loss, value_loss, entropy, approx_kl, clipfrac;
    float loss32;
    uint32_t bad;
} spl_ppo_loss_out_t;

/* spl_ppo_loss: the loss head of ppo_splendor.py:337-352 for one minibatch, forward and backward.  Row b
 * stands for the store's flat position idx[b] = k * T + t (duplicates allowed) and for row b of `logits`
 * and `new_value`, which the caller's actor and critic computed from that position's observation.
 * float32 per row, float64 sums over rows.  With L the set bits of the row's mask word (all 45 actions
 * when no bit is set, ppo_splendor.py:37), a the recorded action, A the advantage (normalised as
 * spl_ppo_gather does when `normalize`), c = clip_coef:
 *   p = softmax(logits over L)    lp = log p[a]    H = -SUM_L p log p    r = exp(lp - logprob)
 *   v_c = value + clamp(v - value, -vclip, vclip)
 * and the gradients of `loss` are those torch's autograd gives for that expression (min / max split a
 * tie evenly, clamp passes the gradient on its closed interval):
 *   g_lp       = -A r / B   when r in [1-c, 1+c] or r A < clamp(r) A, else 0
 *   dlogits[j] = g_lp (1[j = a] - p_j) - (ent_coef / B) p_j (log p_j + H)   for j in L, exactly 0 otherwise
 *   dvalue     = (vf_coef / B) (w1 (v - ret) + w2 (v_c - ret) 1[|v - value| <= vclip])
 *                (w1, w2) = (1, 0) / (0, 1) / (1/2, 1/2) as (v-ret)^2 is above / below / equal to (v_c-ret)^2
 * A bad row (a position outside [0, K*T), whose address is never formed, or a recorded action outside
 * L) gets zero gradients, adds nothing to the sums and counts once in *errors and in out->bad.
 * No floating-point atomics: workgroup partial sums go to `scratch` and are combined in a fixed order,
 * so two calls on the same inputs give the same bits. */
typedef struct {
    int32_t K, T;
    int32_t normalize;            /* as spl_ppo_gather_t.normalize (0: stats may be NULL)             */
    int32_t reserved;             /* 0                                                               */
    const int64_t *idx;           /* [B], 8-byte aligned                                             */
    const uint64_t *mask_bits;    /* the store's planes: [K][T], 8-byte aligned                      */
    const int32_t *action;        /* [K][T]                                                          */
    const float *logprob, *value, *adv, *ret; /* [K][T]                                              */
    const spl_ppo_stats_t *stats;
    const float *logits;          /* [B][45] raw actor logits                                        */
    const float *new_value;       /* [B] the critic's value                                          */
    float clip_coef, vclip, vf_coef; /* each >= 0                                                    */
    float ent_coef;               /* signed: positive adds the entropy to the loss (the reference),
                                     negative subtracts it (the usual bonus)                         */
    float *dlogits;               /* [B][45] out: d loss / d logits                                  */
    float *dvalue;                /* [B] out: d loss / d new_value                                   */
    spl_ppo_loss_out_t *out;      /* out, device, 8-byte aligned                                     */
    uint64_t *errors;             /* device counter, incremented per bad row (never reset here)      */
    void *scratch;                /* spl_ppo_loss_scratch_bytes(B) bytes, device, 8-byte aligned; no
                                     need to clear it                                                */
} spl_ppo_loss_t;

/* ---------------------------------------------------------------------------------------------
 * spl_ppo_adam: clip_grad_norm_, torch.optim.Adam.step and the target-KL `break` of one minibatch as
 * one call (SPL_PPO_ADAM advertises it; SPL_PPO_ABI is unchanged, nothing above moved).
 *
 * The device state block (232 bytes, 8-byte aligned).  The host writes the hyper-parameters with small
 * asynchronous copies; nothing of them is a kernel argument, so a captured call follows them. */
#define SPL_PPO_ADAM 1
#define SPL_PPO_ADAM_MAX_TENSORS 16
#define SPL_PPO_ADAM_CHUNK 2048 /* floats of one partial sum's chunk; a segment starts a new chunk */
#define SPL_PPO_ADAM_PARTS 512  /* partial sums at the most: chunk c belongs to partial c % 512     */
#define SPL_PPO_ADAM_EPOCH 0    /* spl_ppo_adam_begin: a new epoch                                  */
#define SPL_PPO_ADAM_UPDATE 1   /* spl_ppo_adam_begin: a new update                                 */

typedef struct {
    double lr, beta1, beta2, eps;
    double max_norm;             /* negative: no clipping                                            */
    double target_kl;            /* <= 0: the gate is off                                            */
    int64_t step;                /* applied steps since creation: drives the bias corrections        */
    int64_t applied, gated, nonfinite; /* calls since the last begin(UPDATE): applied, skipped by the
                                    latch, skipped for a non-finite norm                             */
    int32_t stopped;             /* the gate's latch                                                 */
    int32_t active;              /* the latest call: 1 applied, 0 skipped                            */
    double grad_norm, clip_coef; /* of the latest call (clip_coef as the float32 the elements saw)   */
    spl_ppo_loss_out_t first;    /* loss_out of the update's first applied call                      */
    spl_ppo_loss_out_t last;     /* loss_out of the latest applied call                              */
    int64_t step_in;             /* hand-off words of a call's two launches (below); not for callers */
    int32_t armed, reserved;
} spl_ppo_adam_state_t;

/* One call, with g the gradients as stored, in this order:
 *  1. norm = sqrt(SUM g*g) over all segments: each square one float32 multiply, the sum float64 in a
 *     fixed order that depends on the segments' sizes alone (never on the device), so two calls on the
 *     same bytes give the same bytes.  With cn = max_norm / (norm + 1e-6) in float64:
 *       clip_coef = fp32(max_norm < 0 ? 1 : cn < 1 ? cn : 1)
 *  2. The call is active when `stopped` was clear on entry and norm is finite.  A set latch skips the
 *     call and counts in `gated` (whatever the norm); else a non-finite norm skips it and counts in
 *     `nonfinite`.  A skipped call leaves every parameter, moment and `step` bit for bit as it was.
 *  3. Active: step += 1, applied += 1; *loss_out (if given) is copied to `last`, and to `first` when
 *     this is the first applied call since begin(UPDATE).
 *  4. Whether active or not: if target_kl > 0 and a KL is given (*approx_kl, else loss_out->approx_kl)
 *     and KL > target_kl, `stopped` is set.  The call whose KL crossed the line is itself applied, as
 *     the reference steps before its `break`; the calls after it are gated until begin().
 *  5. Active, per element, g' = g * clip_coef, every operation one float32 operation, none fused:
 *       m = m + (g' - m) * fp32(1 - beta1)
 *       v = v * fp32(beta2) + fp32(1 - beta2) * (g' * g')
 *       p = p - fp32(lr / (1 - beta1^step)) * (m / (sqrt(v) / fp32(sqrt(1 - beta2^step)) + fp32(eps)))
 *     the scalars computed in float64 from the state block and rounded once.  This is torch.optim.Adam
 *     (_single_tensor_adam: no weight decay, no amsgrad, not maximising) behind clip_grad_norm_.
 * Two launches.  The first writes each partial sum of squares, and its workgroup 0 alone reads the
 * latch, leaves `armed` and `step_in` for the second and applies rule 4.  In the second every workgroup
 * adds the partial sums in the same order, decides alike and applies the step; its workgroup 0 writes
 * active, the counters, grad_norm, clip_coef and the latches, none of which that launch reads.  No
 * launch writes a word that all its workgroups read, and there are no floating-point atomics. */
typedef struct {
    int32_t n;                   /* segments, 1..SPL_PPO_ADAM_MAX_TENSORS                            */
    int32_t reserved;            /* 0                                                               */
    float *param[SPL_PPO_ADAM_MAX_TENSORS];      /* [numel[i]] each, wherever it lies; 4-byte aligned */
    const float *grad[SPL_PPO_ADAM_MAX_TENSORS]; /* [numel[i]]                                       */
    int64_t numel[SPL_PPO_ADAM_MAX_TENSORS];     /* >= 1 each, at most 2^31 together                 */
    float *exp_avg, *exp_avg_sq; /* the moment arenas: segment i at the sum over j < i of numel[j]
                                    rounded up to a multiple of 4 floats.  A segment whose parameter,
                                    gradient and two moment pointers are all 16-byte aligned moves 16
                                    bytes a lane; any other gives the same bits, a dword at a time  */
    spl_ppo_adam_state_t *state; /* device, 8-byte aligned                                           */
    const double *approx_kl;     /* device, 8-byte aligned, or NULL                                  */
    const spl_ppo_loss_out_t *loss_out; /* device, 8-byte aligned, or NULL                           */
    void *scratch;               /* spl_ppo_adam_scratch_bytes(total) bytes, device, 8-byte aligned; no
                                    need to clear it                                                 */
} spl_ppo_adam_t;

/* ---------------------------------------------------------------------------------------------
 * spl_ppo_net_forward / spl_ppo_net_backward: the two networks of the update (297 -> 256 -> 256 -> 45 and
 * 297 -> 256 -> 256 -> 1, tanh; ppo_splendor.py:40-59) around spl_ppo_loss, so that a minibatch is four
 * calls on one stream: forward -> spl_ppo_loss -> backward -> spl_ppo_adam (SPL_PPO_NET advertises them;
 * SPL_PPO_ABI is unchanged, nothing above moved).
 *
 * Row b stands for the store's flat position idx[b] (duplicates allowed), as in spl_ppo_gather and
 * spl_ppo_loss.  Its 297 inputs are rebuilt from the obs_u8 plane as spl_ppo_gather does (column 295 =
 * byte 295 + 256 * byte 297, every other column its byte); no [B][297] float copy exists.  A position
 * outside [0, K*T) is a bad row: its address is never formed, its logits and value are exact zeros, it
 * adds nothing to any gradient, and the forward call counts it once in *errors.
 *
 * float32 operands, float32 accumulation: every sum is one chain of fused multiply-adds in a fixed order
 * (the forward sums in input order from the bias; the backward sums over rows in row order), tanh to about
 * 2 ulp.  No floating-point atomics; the split of the sum over rows is by the constants below, never by the
 * device, and the partial sums are combined in one fixed order: two calls on the same bytes give the same
 * bytes.  1 <= B <= SPL_PPO_NET_MAX_ROWS, above it SPL_E_RANGE.  EVERY pointer of both argument blocks
 * must be 16-byte aligned (SPL_E_ARG otherwise); torch's allocations are.  Argument errors are reported
 * on the host before anything is launched; nothing is allocated; everything is asynchronous on `stream`. */
#define SPL_PPO_NET 1
#define SPL_PPO_NET_MAX_ROWS 65536
#define SPL_PPO_NET_HIDDEN 256
#define SPL_PPO_NET_FWD_ROWS 8    /* rows of one forward workgroup (and of one workgroup of the backward's
                                     first launch)                                                       */
#define SPL_PPO_NET_BWD_ROWS 128  /* rows of one chunk of the sums over rows                              */
#define SPL_PPO_NET_BWD_PARTS 32  /* partial sums at the most: chunk c belongs to partial c % 32          */

typedef struct {            /* torch's nn.Linear layout: weight [out][in] row-major, bias [out]; float32 */
    const float *w1, *b1;   /* [256][297], [256] */
    const float *w2, *b2;   /* [256][256], [256] */
    const float *w3, *b3;   /* [n3][256],  [n3]   n3 = 45 (actor) or 1 (critic) */
} spl_ppo_mlp_t;
typedef struct { float *w1, *b1, *w2, *b2, *w3, *b3; } spl_ppo_mlp_grad_t;   /* same shapes, out */

/* One launch: a workgroup takes SPL_PPO_NET_FWD_ROWS rows through the three layers of one network. */
typedef struct {
    int32_t K, T;
    int64_t reserved;             /* 0                                                               */
    const int64_t *idx;           /* [B]                                                             */
    const uint8_t *obs_u8;        /* the store's plane: [K][T][300]                                  */
    spl_ppo_mlp_t actor, critic;
    float *logits;                /* [B][45] out: what spl_ppo_loss_t.logits takes                   */
    float *new_value;             /* [B] out: what spl_ppo_loss_t.new_value takes                    */
    void *act;                    /* spl_ppo_net_act_bytes(B) bytes out: both networks' activations
                                     behind each tanh, in a layout of the implementation's own, for
                                     the backward call with the same B, idx and weights               */
    uint64_t *errors;             /* device counter, incremented per bad row (never reset here)      */
} spl_ppo_net_fwd_t;

/* Three dependent launches.  With dOut = dlogits (actor) or dvalue (critic), H1 / H2 the saved activations
 * and X the rebuilt inputs, per network, as torch's autograd does for Sequential(Linear, Tanh, Linear,
 * Tanh, Linear):
 *   dW3 = dOut^T H2, db3 = SUM_b dOut;  dZ2 = (dOut W3) (1 - H2^2);  dW2 = dZ2^T H1, db2 = SUM_b dZ2;
 *   dZ1 = (dZ2 W2) (1 - H1^2);  dW1 = dZ1^T X, db1 = SUM_b dZ1.
 * Launch 1 writes dZ2 and dZ1 to `scratch` (SPL_PPO_NET_FWD_ROWS rows a workgroup).  Launch 2 sums every
 * 32 x 32 tile of every dW (a bias gradient is one more column, against ones) over the chunks of
 * SPL_PPO_NET_BWD_ROWS rows of its partial, in row order, into `scratch`.  Launch 3 adds the partials in
 * order and OVERWRITES the twelve gradients: nothing is accumulated into, there is no zero_grad. */
typedef struct {
    int32_t K, T;
    int64_t reserved;             /* 0                                                               */
    const int64_t *idx;           /* [B]: the forward call's                                         */
    const uint8_t *obs_u8;        /* [K][T][300]                                                     */
    spl_ppo_mlp_t actor, critic;  /* the forward call's (b1, b2, b3 are not read)                    */
    const float *dlogits;         /* [B][45] as spl_ppo_loss writes them                             */
    const float *dvalue;          /* [B]                                                             */
    const void *act;              /* the forward call's                                              */
    spl_ppo_mlp_grad_t actor_grad, critic_grad; /* out                                               */
    void *scratch;                /* spl_ppo_net_scratch_bytes(B) bytes; no need to clear it          */
} spl_ppo_net_bwd_t;

/* n rows of one step into the store */
int spl_ppo_record(int32_t n, const spl_ppo_record_t *args, void *stream);
/* bytes of spl_ppo_gae_t.scratch for T tables (SPL_E_ARG for T < 1) */
int64_t spl_ppo_gae_scratch_bytes(int32_t T);
/* advantages, returns and their statistics for a [K][T] store: two launches (the scan with each
 * workgroup's partial sums, then a one-workgroup finish that combines them in a fixed order) */
int spl_ppo_gae(int32_t K, int32_t T, const spl_ppo_gae_t *args, void *stream);
/* one minibatch of B positions, expanded */
int spl_ppo_gather(int32_t B, const spl_ppo_gather_t *args, void *stream);
/* bytes of spl_ppo_loss_t.scratch for B rows (SPL_E_ARG for B < 1) */
int64_t spl_ppo_loss_scratch_bytes(int32_t B);
/* loss, statistics and gradients of one minibatch of B rows: two launches (the rows with each
 * workgroup's partial sums, then a one-workgroup finish), asynchronous on `stream`, nothing allocated */
int spl_ppo_loss(int32_t B, const spl_ppo_loss_t *args, void *stream);
/* bytes of spl_ppo_adam_t.scratch for segments of total_numel floats together (SPL_E_ARG below 1 or
 * above 2^31): room for a partial sum per chunk had every segment but one a single element */
int64_t spl_ppo_adam_scratch_bytes(int64_t total_numel);
/* SPL_PPO_ADAM_EPOCH clears `stopped`; SPL_PPO_ADAM_UPDATE clears `stopped`, `applied`, `gated`,
 * `nonfinite` and `first`.  One launch, asynchronous on `stream` */
int spl_ppo_adam_begin(spl_ppo_adam_state_t *state, int32_t what, void *stream);
/* norm clip, Adam step and KL gate of one minibatch: two launches, asynchronous on `stream`, nothing
 * allocated */
int spl_ppo_adam(const spl_ppo_adam_t *args, void *stream);
/* bytes of spl_ppo_net_fwd_t.act / spl_ppo_net_bwd_t.scratch for B rows (SPL_E_ARG for B < 1, SPL_E_RANGE
 * above SPL_PPO_NET_MAX_ROWS) */
int64_t spl_ppo_net_act_bytes(int32_t B);
int64_t spl_ppo_net_scratch_bytes(int32_t B);
/* both networks' outputs for B positions: one launch */
int spl_ppo_net_forward(int32_t B, const spl_ppo_net_fwd_t *args, void *stream);
/* both networks' twelve parameter gradients, overwritten: three launches */
int spl_ppo_net_backward(int32_t B, const spl_ppo_net_bwd_t *args, void *stream);

/* ---------------------------------------------------------------------------------------------
 * spl_ppo_net_forward_tiled / spl_ppo_net_backward_tiled: the same two passes for large minibatches
 * (SPL_PPO_NET_TILED advertises them; SPL_PPO_ABI is unchanged, nothing above moved).  Rows are blocked as
 * well as units: a workgroup takes SPL_PPO_NET_TILE_ROWS rows through one layer as an LDS-tiled product on
 * the f32-input matrix instruction, so a weight element fetched once serves that many rows.
 *
 * Same argument blocks, same buffers of the same sizes, same refusals, same treatment of bad rows, and THE
 * SAME BYTES in every output: the matrix instruction is a k-ordered chain of fused multiply-adds from its
 * accumulator's start value, which is what the calls above compute, and the sums over rows keep the split
 * by SPL_PPO_NET_BWD_ROWS and SPL_PPO_NET_BWD_PARTS.  `act` is [network][layer][B][256] and the head of
 * `scratch` [network][dZ2, dZ1][B][256] for both pairs, so either forward goes with either backward, and a
 * caller may choose by B without the training run changing.  Forward: three launches (layer 1, layer 2,
 * the output layers); backward: four (dZ2, dZ1, the sums over rows, the ordered combination). */
#define SPL_PPO_NET_TILED 1
#define SPL_PPO_NET_TILE_ROWS 64  /* rows of one workgroup of the tiled forward and dZ launches          */
int spl_ppo_net_forward_tiled(int32_t B, const spl_ppo_net_fwd_t *args, void *stream);
int spl_ppo_net_backward_tiled(int32_t B, const spl_ppo_net_bwd_t *args, void *stream);

/* ---------------------------------------------------------------------------------------------
 * spl_ppo_net_forward_bf16 / spl_ppo_net_backward_bf16: the tiled passes with bf16 operands on the bf16
 * matrix instruction, float32 accumulation, float32 master weights (SPL_PPO_NET_BF16 advertises them;
 * SPL_PPO_ABI is unchanged, nothing above moved).  Opt-in: the numbers DIFFER from the two pairs above, so
 * a training run that switches them on is another run.
 *
 * Same argument blocks, same spl_ppo_net_act_bytes / spl_ppo_net_scratch_bytes, same refusals before any
 * launch, same float32 buffer layouts (`act` [network][layer][B][256], the head of `scratch`
 * [network][dZ2, dZ1][B][256], then the partials), same treatment of a bad row, same launches as the tiled
 * pair (forward three, backward four), asynchronous on `stream`, nothing allocated, no floating-point
 * atomics.  The sums over rows are split by SPL_PPO_NET_BWD_ROWS / SPL_PPO_NET_BWD_PARTS, never by the
 * device: two calls on the same bytes give the same bytes.  The twelve gradients are overwritten.
 *
 * The arithmetic:
 *   - Matrix-instruction products.  Every product issued on the matrix instruction takes BOTH operands
 *     rounded from float32 to bf16, round-to-nearest-even, as they are staged: the weights W1, W2, W3
 *     (actor) and their transposed uses in dZ2 / dZ1; the hidden activations H1, H2; dlogits, dvalue, dZ2
 *     and dZ1 in the sums over rows.  A bf16 x bf16 product is exact in float32; the sum is accumulated in
 *     float32 by the instruction, from the bias in the forward layers and from zero elsewhere.  The order
 *     inside an instruction is the hardware's and no part of this contract.
 *   - The inputs X enter exactly.  Every column is a byte (exact in bf16) except column 295 = byte 295 +
 *     256 * byte 297, which is fed as two k-positions, byte 295 at k = 295 and 256 * byte 297 at the pad
 *     position k = 297, both against W1[:, 295]; in dW1 the two positions' sums are added into column 295.
 *     No input value is ever rounded.
 *   - Everything elementwise stays float32: the bias add (the accumulator's start), tanh (4 ulp), fma(-h, h,
 *     1), the zeros of a bad row, the saved activations and dZ planes as stored.
 *   - VALU products take unrounded float32 operands: the critic's single output unit, the critic's
 *     elementwise dZ2, and the bias gradients (plain float32 sums down the rows).
 *   - Master weights, moments and spl_ppo_adam stay float32; nothing outside these two calls changes.
 *   - Denormal operands: whether the bf16 instruction flushes them is unspecified. */
#define SPL_PPO_NET_BF16 1
int spl_ppo_net_forward_bf16(int32_t B, const spl_ppo_net_fwd_t *args, void *stream);
int spl_ppo_net_backward_bf16(int32_t B, const spl_ppo_net_bwd_t *args, void *stream);

/* ---------------------------------------------------------------------------------------------
 * spl_ppo_permute and spl_ppo_loss_dev: what a whole update captured as ONE graph needs from the device
 * (SPL_PPO_PERMUTE advertises both; SPL_PPO_ABI is unchanged, nothing above moved).  A replayed graph repeats
 * its kernel arguments, so whatever changes from update to update has to live in device memory: the epoch's
 * permutation is drawn from a device state block that the call itself advances, and the loss head reads its
 * four coefficients from a device block that the host rewrites between replays.
 *
 * spl_ppo_permute: a keyed permutation of 0 .. n-1, every element computed on its own (no sort, no
 * atomics) by a keyed bijection with cycle walking:
 *   n == 1: {0}.  Otherwise bits = max(2, bit_length(n - 1)), a = bits / 2, b = bits - a, and one PASS is
 *   eight rounds r = 0..7 on x in [0, 2^bits):
 *     (wl, wr) = (b, a) when r is even, else (a, b)
 *     L = x >> wr,  R = x & (2^wr - 1)
 *     f = the .x word of Philox4x32-10(counter = (R, r, draw_lo, draw_hi), key = (seed_lo, seed_hi))
 *     x = (R << wl) | ((L ^ f) & (2^wl - 1))
 *   perm[i]: x = i, one pass, and another pass while x >= n.
 * A pass is a bijection of [0, 2^bits), so the walk from i < n comes back below n, and since 2^bits < 2n
 * (n >= 3) it takes fewer than two passes on average.  (seed, draw) select the permutation; the call leaves
 * draw + 1 behind it, so the next call, or the next replay of a captured call, draws the next one.
 *
 * Output: element i goes to out[(i / B) * stride + i % B] with stride = B rounded up to even, so minibatch
 * m = the first min(B, n - m B) words of row m, and every row starts on a 16-byte boundary whatever B is.
 * The pad word of a row (B odd) and the last row's words past n are written as -1: a consumer that takes
 * them for positions counts bad rows.  Exactly ceil(n / B) * stride words are written.
 *
 * Two launches: the permutation, whose threads all read *state, then one thread that advances state->draw
 * behind it; no launch writes a word that its other threads read. */
#define SPL_PPO_PERMUTE 1
typedef struct { uint64_t seed, draw; } spl_ppo_perm_state_t;   /* device, 16 bytes, 8-byte aligned */
typedef struct {
    int64_t n;                      /* positions: 1 .. 2^31 - 1 (SPL_E_RANGE otherwise)                 */
    int32_t B;                      /* minibatch size: 1 .. n (SPL_E_RANGE otherwise)                   */
    int32_t reserved;               /* 0                                                               */
    spl_ppo_perm_state_t *state;    /* read; draw is advanced by 1 behind the permutation              */
    int64_t *out;                   /* [ceil(n/B)][stride], stride = B rounded up to even; 16-byte
                                       aligned                                                         */
} spl_ppo_permute_t;
/* SPL_E_RANGE for n or B out of range, SPL_E_ARG for a null or misaligned pointer or reserved != 0;
 * nothing is launched on an error.  Asynchronous on `stream`, nothing allocated */
int spl_ppo_permute(const spl_ppo_permute_t *args, void *stream);

/* spl_ppo_loss with {clip_coef, vclip, vf_coef, ent_coef} read on the device from coef[0..3] (device,
 * 16-byte aligned) instead of from the argument block, whose own four fields are ignored.  Everything else
 * is spl_ppo_loss (the same kernels, the same fixed-order sums): the same inputs give the same bits as
 * spl_ppo_loss with those four values as arguments.  The host cannot check device values, so what
 * spl_ppo_loss refuses is handled per call on the device: with a negative or NaN clip_coef, vclip or
 * vf_coef, or a NaN ent_coef, EVERY row of the call is a bad row: zero gradients, nothing in the sums,
 * *errors and out->bad rise by B. */
int spl_ppo_loss_dev(int32_t B, const spl_ppo_loss_t *args, const float *coef, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLENDOR_PPO_H */
