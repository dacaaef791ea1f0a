/*
 * mtfjsp.h — C ABI of libmtfjsp.so: MI355X-native batched MT-FJSP disjunctive-graph
 * environment (reset / step / observe / masks), the rollout forward passes of
 * the GIN + GAT actors, and the planner of the dispatch-rule baselines ("pdrs:" =
 * tester/pdrs.py).  This is the drop-in boundary for the hot path of
 * RKWin93/E2E-MAPPO-for-MT-FJSP; every entry point cites the reference interface
 * it replaces ("pe:" = trainer/parallel_env.py, "env:" = graph-jsp-env/src/
 * graph_jsp_env/disjunctive_graph_jsp_env_singlestep.py, "ppo:" =
 * algorithm/ppo_algorithm.py, "ac:" = model/actor_critic.py, "agent:" =
 * algorithm/agent_func.py, "run:" = Run.py).  The reference-side ctypes binding
 * is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; every function returns 0 (MTFJSP_OK) or a negative
 *    mtfjsp_status; mtfjsp_last_error(h) describes the last failure on h.
 *  - One handle per GPU.  A handle is not thread-safe; distinct handles are.
 *  - All array arguments are DEVICE pointers unless the name ends in _host.
 *    Work is enqueued on the handle's stream (mtfjsp_set_stream; default: the
 *    NULL stream) and is asynchronous; *_host variants synchronise that stream.
 *  - Task index a in [0,T), T = n_job*n_machine, job = a / n_machine,
 *    op = a % n_machine (square instances: ops per job == n_machine, as in the
 *    reference generator).  Machine index m in [0,M).
 *  - Scheduling state and all times/rewards are IEEE binary64, evaluated in the
 *    reference's operation order without FMA contraction.
 */
#ifndef MTFJSP_H
#define MTFJSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mtfjsp_env *mtfjsp_handle_t;
typedef struct mtfjsp_encoder *mtfjsp_encoder_t;

typedef enum {
    MTFJSP_OK = 0,
    MTFJSP_ERR_ARG = -1,      /* bad argument / configuration */
    MTFJSP_ERR_STATE = -2,    /* call order (e.g. step before load_instances/reset) */
    MTFJSP_ERR_HIP = -3,      /* HIP runtime error (no device, launch failure, OOM) */
    MTFJSP_ERR_ACTION = -4,   /* *_host step: at least one action was invalid */
    MTFJSP_ERR_RETRY = -5     /* encoder: an earlier forward on the single-launch GIN kernel failed asynchronously (time-out of a grid-wide statistics exchange);
                               * everything enqueued on the handle since then is invalid, the handle has switched to the streaming
                               * launches — repeat the work (see mtfjsp_encoder_check) */
} mtfjsp_status;

enum { MTFJSP_OBS_F64 = 0, MTFJSP_OBS_F32 = 1 };

/* per-instance status word written by mtfjsp_step (bound obs.status) */
enum {
    MTFJSP_PATH_MASK = 0x7,          /* scheduling path taken (env:1531-1685): */
    MTFJSP_PATH_EMPTY = 0,           /*   machine route was empty */
    MTFJSP_PATH_FRONT = 1,           /*   left-shifted to the front of the route */
    MTFJSP_PATH_BETWEEN = 2,         /*   left-shifted into a gap */
    MTFJSP_PATH_APPEND = 3,          /*   appended */
    MTFJSP_ST_INVALID = 0x100,       /* already scheduled / job predecessor unscheduled / index out of range:
                                        the instance is left untouched (the reference silently corrupts node
                                        attributes here, env:1496-1528; never reached under the masks).
                                        A REJECTED step moves nothing of the instance — scheduling state, the 17
                                        RewardScaling words, tasks_fea, ELL rows, m_fea2, candidate, job_mask — and
                                        writes only its per-step outputs:
                                          status  = MTFJSP_ST_INVALID exactly (no path bits, no ST_INFEASIBLE)
                                          info    = [0, done, 0, 0, 0, 0]
                                          raw     = [0, 0, 0, 0, 0]
                                          r4_out  = [0, 0, 0, 0], done_out = done   (mtfjsp_step_record)
                                        with done = 1 iff all T tasks of the instance are scheduled already (a finished
                                        instance that keeps receiving actions keeps reporting done), else 0.  The
                                        other instances of the batch, of the same workgroup included, step as usual */
    MTFJSP_ST_INFEASIBLE = 0x200     /* t[a,m] < 0 chosen (pe:246-248 prints a warning and carries on; so do we) */
};

typedef struct {
    int32_t n_job, n_machine, n_edge;   /* pe:22-25 */
    int32_t batch;                      /* env_batch, pe:26 */
    int32_t left_shift;                 /* perform_left_shift_if_possible (pe:116; tester/pdrs.py:669 uses 0) */
    int32_t obs_dtype;                  /* MTFJSP_OBS_F64: observations as the reference returns them (f64)
                                           MTFJSP_OBS_F32: the same values rounded once to f32 — what ac:143,377
                                           `.float()` would produce — for the device-resident rollout */
    int32_t device_id;
    int32_t reserved;
    double gamma;                       /* GAMMA for RewardScaling, pe:81 */
    double w_mk, w_ec, w_tt;            /* config weights in the scalar reward, env:1119-1132 */
    double scaling_divisor;             /* reward_function_parameters['scaling_divisor'], env:1164 */
} mtfjsp_config_t;

/* Observation / step outputs, all DEVICE pointers, caller- or library-allocated.
 * Shapes use B = batch, T, M, J.                                                                  replaces        */
typedef struct {
    void *tasks_fea;      /* [B*T,12] obs_dtype: st_est, ft_est, pt_est, scheduled, in_degree,      env:2245-2277   */
                          /*          machine+1|0, t|0, p|0, job+1, w3[0..2]                                         */
    int32_t *ell_col;     /* [B*T,2]  in-edge sources of node v (task index inside the instance,   env:2019-2073   */
                          /*          -1 = none): slot 0 job edge, slot 1 machine edge                               */
    float *ell_val;       /* [B*T,2]  adj_wrk values of those edges (small integers); the self      (dense: see     */
                          /*          loop (value 1) is implicit                                     export below)   */
    void *m_fea2;         /* [B,M,8]  obs_dtype                                                     env:2315-2354   */
    double *info;         /* [B,6]    reward, done, mk_s, idle_s, pt_s, tt_s (scaled components)    pe:255-262      */
    double *raw;          /* [B,5]    reward, r_mk, r_idle, r_pt, r_tt (unscaled); may be NULL      env:1051-1171   */
    int32_t *candidate;   /* [B,J]    next selectable task of each job                              ppo:306-309     */
    uint8_t *job_mask;    /* [B,J]    1 = job not selectable                                        ppo:238-297     */
    int32_t *status;      /* [B]      see MTFJSP_PATH_* / MTFJSP_ST_*                                               */
} mtfjsp_obs_t;

/* ------------------------------------------------------------------ lifecycle */
/* = Parallel_env.__init__ (pe:20-37). Allocates all device state for `batch` instances. */
int mtfjsp_create(const mtfjsp_config_t *cfg, mtfjsp_handle_t *out);
int mtfjsp_destroy(mtfjsp_handle_t h);
const char *mtfjsp_last_error(mtfjsp_handle_t h);      /* h may be NULL: last create() error */
int mtfjsp_set_stream(mtfjsp_handle_t h, void *hip_stream);
int mtfjsp_synchronize(mtfjsp_handle_t h);

/* Library-owned observation buffers (freed by destroy) / caller-owned ones. */
int mtfjsp_alloc_obs(mtfjsp_handle_t h, mtfjsp_obs_t *out);
int mtfjsp_bind_obs(mtfjsp_handle_t h, const mtfjsp_obs_t *obs);
/* = the observation copies of ReplayBuffer.store_operation (trainer/replaybuffer.py:82-139): snapshot of the
 * CURRENT bound observation into caller buffers of the same layout (a trajectory slot), one launch on the handle's stream.
 * Fields of dst left NULL are skipped (status is never copied).  The adjacency stays ELL: the reference's dense
 * [steps,B,T,T] f64 buffer is 7.6 GB per copy at B=4096 J6M6. */
int mtfjsp_snapshot_obs(mtfjsp_handle_t h, const mtfjsp_obs_t *dst);
/* The same launch with a second destination and the scalar reward: the reference's buffer stores s' of step k (adj_, fea_, ...:
 * replaybuffer.py:108-118) and s of step k+1 (replaybuffer.py:97-104) separately although they are the same observation inside an
 * episode, and the reward as f32 [B] (replaybuffer.py:106 <- info[:,0], pe:255-262).  dst2 (may be NULL) receives a second copy of
 * every field it has; reward_out (may be NULL) receives (float)info[b][0]. */
int mtfjsp_snapshot_obs2(mtfjsp_handle_t h, const mtfjsp_obs_t *dst, const mtfjsp_obs_t *dst2, float *reward_out);

/* ------------------------------------------------------------------ instances */
/* = Parallel_env.get_batch (pe:39-66): t,p [B,T,M] (negative = machine infeasible), tt [B,M,M],
 * shop_of_machine [B,M] (0-based shop id; the reference's edge[E,M/E] table inverted).
 * Precomputes min_dur/min_pt (env:1932-1950) and the per-task means used by m_fea1 (pe:176-183). */
int mtfjsp_load_instances(mtfjsp_handle_t h, const double *t, const double *p, const double *tt,
                          const int32_t *shop_of_machine);
int mtfjsp_load_instances_host(mtfjsp_handle_t h, const double *t_host, const double *p_host,
                               const double *tt_host, const int32_t *shop_host);
/* = Instance_Dataset generation (instance/generate_allsize_mofjsp_dataset.py:133-296) ON the device, straight into the
 * handle's instance arrays: same distributions (scope9 = t_low, t_high, p_low, p_high, weight_low,
 * weight_high, transT_in_low, transT_in_high, transT_out_high of instance/config_ins.json), Philox stream keyed by
 * (seed, first_instance + b) — distributional parity only, the legacy MT19937 stream stays in the host generator. */
int mtfjsp_generate_instances(mtfjsp_handle_t h, uint64_t seed, uint64_t first_instance, const double *scope9);
/* t, p [B,T,M] f64, tt [B,M,M] f64, shop [B,M] i32 of the loaded / generated instances, to host memory. */
int mtfjsp_read_instances_host(mtfjsp_handle_t h, double *t, double *p, double *tt, int32_t *shop);

/* = init_RewardScaling_sameBATCH (pe:70-85) and RewardScaling.reset() per episode (run:283-284). */
int mtfjsp_scaler_init(mtfjsp_handle_t h);
int mtfjsp_scaler_reset_returns(mtfjsp_handle_t h);
/* same, only for instances with mask_host[b] != 0 (run:283-284 resets them one by one) */
int mtfjsp_scaler_reset_returns_masked_host(mtfjsp_handle_t h, const uint8_t *mask_host);

/* ------------------------------------------------------------------ reset / step */
/* = init_DGFJSPEnv_state0 (pe:87-149) = env.reset() on every instance (env:1183-1245).
 * w3 [B,3]: normalised reward weights; the host draws them (env:1253-1259 uses python `random`). */
int mtfjsp_reset(mtfjsp_handle_t h, const double *w3);
/* = env.generate_random_weights("01") (env:1253-1259) for every instance ON the device: w3_out [B,3] f64 (device), three
 * uniforms normalised by their sum, Philox stream keyed by (seed, episode, instance) — distributional parity, for rollouts
 * that must not wait for the host; parity runs draw the weights with python `random` and pass them to mtfjsp_reset. */
int mtfjsp_draw_reward_weights(mtfjsp_handle_t h, uint64_t seed, uint64_t episode, double *w3_out);
/* One episode's start in ONE launch (the accelerated rollout issued three per episode): mtfjsp_draw_reward_weights(seed, episode) into
 * w3_out [B,3] (kept: the trajectory record and the next episode's observations carry the weights), mtfjsp_reset with them, and — with
 * reset_returns != 0 — mtfjsp_scaler_reset_returns (run:283-284: RewardScaling.reset() of every instance, pt:123).  Bit-identical to
 * the three calls. */
int mtfjsp_reset_episode(mtfjsp_handle_t h, uint64_t seed, uint64_t episode, double *w3_out, int32_t reset_returns);
int mtfjsp_reset_host(mtfjsp_handle_t h, const double *w3_host);

/* = DGFJSPEnv_paral_step (pe:217-268): env.step (env:716-974) + RewardScaling (pe:255-260), fused with
 * the candidate / job-mask update of ppo:202-316.  One launch; writes every bound obs field.
 * Actions are judged per instance: an instance with a bad action (MTFJSP_ST_INVALID above) is skipped — state and observation
 * untouched, info = [0, done, 0, 0, 0, 0], raw = 0, status = MTFJSP_ST_INVALID, done = 1 once the instance is finished — while
 * the others step; the device entry points return MTFJSP_OK either way (the caller reads status). */
int mtfjsp_step(mtfjsp_handle_t h, const int32_t *task_idx, const int32_t *mach_idx);
/* same launch, additionally recording this step's trajectory entries as f32 for the advantage computation
 * (SURVEY Appendix A rows 11,17-20): r4_out [4,B] = scaled mk, idle, pt, tt (pe:255-262 order) ; done_out [B]:
 * the float32 of info[b][2..5] and of info[b][1].  A rejected instance gets r4_out[:, b] = 0 and done_out[b] = done as above. */
int mtfjsp_step_record(mtfjsp_handle_t h, const int32_t *task_idx, const int32_t *mach_idx, float *r4_out, float *done_out);
/* The step as the TAIL of the launch that selects the machines (Run.py:363-427: machine actor forward, then env.step, nothing in
 * between): mtfjsp_step_params fills an opaque parameter block (mtfjsp_step_params_bytes() bytes) for exactly the step that
 * mtfjsp_step / mtfjsp_step_record (r4_out, done_out both given or both NULL) with these arguments would run, and returns 1; or
 * returns 0 when this handle's step cannot ride in another launch (shapes beyond the 16-instance register kernel, kernel-time
 * recording on, a diagnostic kernel override) and the caller must call mtfjsp_step itself; < 0 on errors.  The block is handed to
 * mtfjsp_encoder_arm_env_step before the mtfjsp_machine_actor_forward whose armed selection writes `mach_idx`. */
int32_t mtfjsp_step_params_bytes(void);
int mtfjsp_step_params(mtfjsp_handle_t h, const int32_t *task_idx, const int32_t *mach_idx, float *r4_out, float *done_out,
                       void *params_out, int32_t params_bytes);
/* The step kernel the next mtfjsp_step on this handle launches ("k_env_grp16", ...: the launch selection itself, on the handle's shape,
 * its device's LDS capacity and the diagnostic switches MTFJSP_ENV_KERNEL / MTFJSP_ENV_LDS / MTFJSP_ENV_STEP_G as they are NOW — they are
 * read on every call).  mtfjsp_step_kernel_name_for: the same for a shape without a handle, where a workgroup may use lds_max bytes of
 * LDS (gfx950: 160 KiB); no device is touched.  Optional outputs: instances per workgroup, bytes of one instance's LDS region (0: register
 * kernels), whether a switch is set.  NULL for a shape mtfjsp_create rejects, one that needs more than lds_max bytes for a single instance
 * included.  mtfjsp_step_launch_info: of that same launch on a live handle, the instances per workgroup, the dynamic LDS bytes of the
 * launch (0: register kernels) and the LDS a workgroup may use on the handle's device; every output is optional. */
const char *mtfjsp_step_kernel_name(mtfjsp_handle_t h);
int mtfjsp_step_launch_info(mtfjsp_handle_t h, int32_t *group_out, int64_t *lds_launch_out, int64_t *lds_max_out);
const char *mtfjsp_step_kernel_name_for(int32_t n_job, int32_t n_machine, int32_t batch, int32_t obs_f32, int64_t lds_max,
                                        int32_t *group_out, int64_t *lds_bytes_out, int32_t *overridden_out);
/* host variant: returns MTFJSP_ERR_ACTION if any status word carries MTFJSP_ST_INVALID — AFTER the launch: the valid instances of
 * the batch have been stepped, the rejected ones hold the outputs above; mtfjsp_last_error names the first rejected instance */
int mtfjsp_step_host(mtfjsp_handle_t h, const int32_t *task_idx_host, const int32_t *mach_idx_host);

/* = cal_cur_task_machine_feature (pe:152-214): out [B,M,6] obs_dtype, mmask_out [B,M] (1 = infeasible; may be
 * NULL).  mmask_in [B,M] may be NULL (then feasibility t>=0 is used, which is what run:335 passes). */
int mtfjsp_observe_mfea1(mtfjsp_handle_t h, const int32_t *task_idx, const uint8_t *mmask_in,
                         void *out, uint8_t *mmask_out);

/* Uniform random valid actions on device (benchmark / property-test policy, SURVEY §8d "on-device Philox allowed
 * for perf runs"): job uniform over unmasked jobs of the bound job_mask, machine uniform over feasible ones. */
int mtfjsp_random_actions(mtfjsp_handle_t h, uint64_t seed, uint64_t counter, int32_t *task_idx,
                          int32_t *mach_idx, int32_t *job_idx);

/* ------------------------------------------------------------------ fork */
/* Device-side copy of environment state between handles: destination instance i becomes a copy of source instance src_index[i]
 * (device, int32 [dst.batch]; duplicates and any order allowed) — the primitive of every search-style use: continue one partial
 * schedule in several directions, try an action and take it back (keep the original, step the copy).  The reference has no
 * counterpart: its one-step look-ahead rule re-runs env.reset() and replays the whole prefix for every candidate (pdrs:465-540).
 *   MTFJSP_FORK_INSTANCE  the instance constants: t, p, tt and what load_instances derives from them (transposed tt, {min_dur,
 *                         min_pt}, per-task means), shop_of_machine
 *   MTFJSP_FORK_STATE     the scheduling state: per-task, per-job and per-machine records, the f64 machine features, and every
 *                         per-instance scalar (previous costs, transport, reward weights, the 17 RewardScaling words, the merged-edge
 *                         words), plus the reset weights mtfjsp_reset_host staged.  The step kernels read no bound observation field
 *                         back — candidate and job_mask are derived from the job records and only written — so a copy forked with
 *                         STATE alone steps correctly: info, raw and status of its later steps are right, while its observation
 *                         (tasks_fea, ELL rows, m_fea2, candidate, job_mask: a step rewrites only the rows it changes) is undefined
 *                         until its next reset
 *   MTFJSP_FORK_OBS       the bound observation: tasks_fea, ell_col, ell_val, m_fea2, info, raw (where both have it), candidate,
 *                         job_mask, status
 * ONE launch (k_env_fork) on dst's stream, 16-byte words wherever an array's bytes per instance allow; nothing is read back and
 * nothing synchronises.  ORDERING AGAINST src's STREAM IS THE CALLER'S DUTY (same stream, or an event): the launch reads src's
 * arrays as they are when it runs.
 * dst and src must agree in n_job, n_machine, n_edge, obs_dtype, left_shift and device (batches may differ) and must be distinct
 * handles (an in-place gather races between instances): otherwise MTFJSP_ERR_ARG.  MTFJSP_ERR_STATE: src not loaded; STATE or OBS
 * from a src that was never reset; OBS without bound observations on either side; no INSTANCE flag and a dst without instances.
 * Nothing is written on an error return.  After success dst counts as loaded if INSTANCE was set and as reset if STATE was set.
 * An index outside [0, src.batch) leaves that destination instance untouched and sets MTFJSP_ST_INVALID in its status word (where
 * dst has observations bound); all other instances are copied. */
enum { MTFJSP_FORK_INSTANCE = 1, MTFJSP_FORK_STATE = 2, MTFJSP_FORK_OBS = 4 };
int mtfjsp_fork(mtfjsp_handle_t dst, mtfjsp_handle_t src, const int32_t *src_index, int32_t flags);

/* ------------------------------------------------------------------ one-step look-ahead dispatch rules */
/* = the look-ahead of LWKR_IT_o_jointActor (pdrs:465-540: for every candidate env.reset(), replay of the prefix, the candidate's
 * step, pdrs:486-510; then the choice, pdrs:512-520), as one copy and one ordinary step per candidate.  src holds B instances,
 * scratch B*T (T = n_job*n_machine) whose constants were forked once (mtfjsp_fork, MTFJSP_FORK_INSTANCE, index i -> i / T): copy
 * (b, j, m) = scratch instance (b*n_job + j)*n_machine + m tries "job j's next task on machine m" for source instance b.
 * mtfjsp_lookahead_expand: forks src's STATE into scratch (k_env_fork with the implicit index i / T) and writes the candidate
 * actions task_c, mach_c [B*T]; two launches on scratch's stream.  The caller then runs mtfjsp_step(scratch, task_c, mach_c):
 * the copies of a finished job come back with MTFJSP_ST_INVALID, an infeasible machine with MTFJSP_ST_INFEASIBLE — throw-away
 * copies either way.  Errors as mtfjsp_fork; scratch.batch != src.batch * T: MTFJSP_ERR_ARG.
 * mtfjsp_lookahead_select: per source instance, the copy without those two flags whose raw[column] is LARGEST (rewards are
 * previous minus current cost: the least added cost; column 0..4 = scalar reward, makespan, idle, energy, transport, env:1051-1171),
 * compared as binary64, no arithmetic; a NaN is never selected (-inf is a value like any other); ties go to the lowest (j, m) (pdrs:520 draws among tied jobs with random.choice, and the
 * reference fixes each task's machine beforehand by a machine rule: here the look-ahead ranges over (job, machine) jointly).
 * task_out, mach_out [B] (device; the action for mtfjsp_step(src, ...)), job_out [B] and best_out [B] f64 (the winning value:
 * the picked copy's own raw[column], bit for bit — -0.0 where that copy holds -0.0, whatever equal zero another copy holds)
 * may be NULL.  An instance without a copy to pick (finished, or NaN in every copy that counts) gets task, machine, job -1 and best NaN.  One launch, one wavefront per
 * source instance, on src's stream; it reads scratch's bound status and raw and src's job records: ordering between the two
 * handles' streams is the caller's duty here too. */
int mtfjsp_lookahead_expand(mtfjsp_handle_t scratch, mtfjsp_handle_t src, int32_t *task_c, int32_t *mach_c);
int mtfjsp_lookahead_select(mtfjsp_handle_t scratch, mtfjsp_handle_t src, int32_t column, int32_t *task_out, int32_t *mach_out,
                            int32_t *job_out, double *best_out);

/* ------------------------------------------------------------------ beam search on the fork */
/* Beam search over (job, machine) decisions: keep the W best partial schedules ("slots") of each of N source instances, expand
 * each into its T children, keep the best W again.  beam holds N*W instances (slot w of source n = instance n*W + w), scratch
 * N*W*T with its constants forked once (index i -> i / (W*T) of the source set).  One decision is mtfjsp_lookahead_expand(scratch,
 * beam, ...), mtfjsp_step(scratch, ...), optionally mtfjsp_state_signature(scratch, sig), mtfjsp_beam_select and
 * mtfjsp_fork(beam, scratch, parent_out, MTFJSP_FORK_STATE); after the last one mtfjsp_beam_backtrack reads the plans out.
 * The reference has no search (its only look-ahead is the greedy pdrs:465-540).
 *
 * mtfjsp_state_signature: sig_out [batch] (device, u64) = a 64-bit signature of every instance's PARTIAL SCHEDULE that does not
 * depend on the order in which its decisions were taken: the sum mod 2^64 over the scheduled tasks k of
 *     mix(mix(bits64(start_k)) + ((uint64)k << 32 | (uint64)machine_k << 16 | (uint64)position_k in its machine's route)),
 * mix = the splitmix64 finaliser (z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31);
 * an unscheduled task contributes 0, so a freshly reset instance has signature 0.  Equal partial schedules (the same tasks on the
 * same machines at the same positions and start times) have equal signatures; distinct ones collide with probability about 2^-64.
 * With left shift off any two decisions on different machines commute, so every order in which one partial schedule can be reached gives one signature.
 * NOT covered, deliberately: the words that remember the previous step (the merged-edge node and its transport time), the 17
 * RewardScaling words and the previous-step costs — two states that agree in the schedule but differ there count as equal.
 * Merging by signature is therefore a search heuristic: a false merge costs one beam slot and never corrupts a state.
 * One launch on h's stream (one wavefront per instance, lanes over tasks), nothing read back.  MTFJSP_ERR_STATE: h never reset
 * (a handle replayed with MTFJSP_REPLAY_STATE holds schedules and is accepted).
 *
 * mtfjsp_beam_select: candidate c = w*T + r of source n (r = j*n_machine + m: slot w tries job j's next task on machine m) is
 * scratch instance g = (n*W + w)*T + r.  It is eligible iff score_in[n*W + w] != -inf (-inf marks an empty slot) and status[g]
 * carries neither MTFJSP_ST_INVALID nor MTFJSP_ST_INFEASIBLE; its value is score_in[n*W + w] + raw[g][column] — one binary64
 * addition, so a slot's score is the running sum of its one-step rewards in step order; a NaN value is never selected.  Ranks
 * k = 0..W-1 in turn take the eligible candidate of the largest value, the lowest c among equals, and remove it; where sig
 * (device u64 [N*W*T], what mtfjsp_state_signature(scratch) wrote; may be NULL) is given, every candidate with the pick's
 * signature is removed with it (duplicates are merged into their best, lowest-c representative).  Outputs, device [N*W], at
 * n*W + k: parent_out = g (the index of the following mtfjsp_fork), from_slot_out = w, task_out / mach_out = the child's action
 * (formed from beam's job records as mtfjsp_lookahead_select forms it), score_out = the value — the picked candidate's own
 * sum, bit for bit (of -0.0 and +0.0, which tie, each rank reports the zero its candidate holds).  A rank left without a candidate
 * writes -1, -1, -1, -1, -inf: the fork leaves that slot untouched and the score marks it empty.  An instance without any
 * candidate to pick (finished) keeps its beam: parent -1, from_slot = k, task = mach = -1, score_out = score_in.
 * 1 <= W <= 64, beam.batch % W == 0, W*T <= 8192 (the candidates live in one workgroup's LDS), column 0..4, scratch.batch ==
 * beam.batch*T, score_out != score_in (every rank reads all parent scores): otherwise MTFJSP_ERR_ARG and nothing is written.
 * One launch, one workgroup per source instance, on beam's stream; it reads scratch's bound status and raw: ordering between the
 * handles' streams is the caller's duty, as for the look-ahead.
 *
 * mtfjsp_beam_backtrack: h = the beam handle (N = batch / W).  hist_from_slot, hist_task, hist_mach: device int32 [S, N*W], row s
 * = what decision s's mtfjsp_beam_select wrote (hand it pointers into these arrays).  start_slot: device int32 [N], or NULL for
 * slot 0 — the best, since ranks come out in order.  task_plan, mach_plan: device int32 [N, S]; with k = start_slot[n], for
 * s = S-1 .. 0: plan[n][s] = hist[s][n*W + k], k = hist_from_slot[s][n*W + k].  A slot outside [0, W) met on the way (an empty
 * rank) writes -1 for that and every earlier step.  One launch, one thread per source instance, on h's stream. */
int mtfjsp_state_signature(mtfjsp_handle_t h, uint64_t *sig_out);
int mtfjsp_beam_select(mtfjsp_handle_t scratch, mtfjsp_handle_t beam, int32_t W, int32_t column, const double *score_in, const uint64_t *sig,
                       int32_t *parent_out, int32_t *from_slot_out, int32_t *task_out, int32_t *mach_out, double *score_out);
int mtfjsp_beam_backtrack(mtfjsp_handle_t h, int32_t W, int32_t S, const int32_t *hist_from_slot, const int32_t *hist_task,
                          const int32_t *hist_mach, const int32_t *start_slot, int32_t *task_plan, int32_t *mach_plan);

/* ------------------------------------------------------------------ policy-guided beam search on the fork */
/* Beam decoding of the trained actors: a slot's score is the running sum of log p(job) + log p(machine | job) along its decisions,
 * and only the W children that are kept are stepped.  Two beam handles of N*W instances take turns (mtfjsp_fork needs distinct
 * handles).  One decision on the current one: mtfjsp_job_actor_forward (batch N*W), mtfjsp_observe_mfea1_jobs, ONE
 * mtfjsp_machine_actor_forward over all N*W*n_job (slot, job) rows, the two logarithms, mtfjsp_beam_select_policy,
 * mtfjsp_fork(next, current, parent_out, STATE | OBS), mtfjsp_step(next, task_out, mach_out), optionally
 * mtfjsp_state_signature(next) + mtfjsp_beam_merge_slots; mtfjsp_beam_backtrack reads the plans out as for the cost beam.
 * The reference decodes greedily or by sampling only (validate.py:60-297).
 *
 * mtfjsp_observe_mfea1_jobs: out [B, n_job, n_machine, 6] in the handle's observation dtype, mmask_out [B, n_job, n_machine] bytes
 * (may be NULL).  Row (b, j) is, bit for bit, what mtfjsp_observe_mfea1 writes for task_idx[b] = candidate[b][j] (the handle's bound
 * observation field) with mmask_in = NULL — for every job, masked or not; an index outside [0, T) is treated as there (task 0).
 * One launch on the handle's stream, nothing read back.  MTFJSP_ERR_STATE: no reset, or no bound observations.  MTFJSP_ERR_ARG,
 * nothing written: out NULL, or the two outputs overlap.
 *
 * mtfjsp_beam_select_policy: beam holds N*W slots (slot w of source n = instance n*W + w) with bound candidate and job_mask.
 * score_in [N*W] f64, logp_job [N*W, n_job] f64, logp_mach [N*W*n_job, n_machine] f64, mmask [N*W*n_job, n_machine] bytes (device).
 * Candidate c = w*T + j*n_machine + m of source n is "slot w schedules job j's next task on machine m"; with slot = n*W + w it is
 * eligible iff score_in[slot] != -inf, job_mask[slot][j] == 0, mmask[slot*n_job + j][m] == 0 and its value is neither NaN nor -inf;
 * value = (score_in[slot] + logp_job[slot][j]) + logp_mach[slot*n_job + j][m] — two binary64 additions in exactly this order.  The
 * kernel takes logarithms, not probabilities, on purpose: it holds comparisons and these two additions only, so a host model
 * reproduces it exactly.  Ranks k = 0..W-1 in turn take the eligible candidate of the largest value, the lowest c among equals, and
 * remove it.  Outputs, device [N*W], at n*W + k: parent_out = slot (the index of the following mtfjsp_fork), from_slot_out = w,
 * job_out = j, task_out = the child's task (formed from beam's job records as mtfjsp_beam_select forms it), mach_out = m,
 * child_out = slot*n_job + j (the machine forward's row: its pooled embedding is the child's), score_out = the picked candidate's own
 * sum, bit for bit.  A rank left without a candidate writes -1 in the six integer outputs and -inf in score_out: the fork leaves that
 * slot untouched, the step rejects task -1, and the score marks it empty.  1 <= W <= 64, beam.batch % W == 0, W*T <= 8192,
 * score_out != score_in: otherwise MTFJSP_ERR_ARG and nothing is written.  One launch, one workgroup per source instance, on beam's
 * stream.
 *
 * mtfjsp_beam_merge_slots: sig [N*W] (device u64, what mtfjsp_state_signature(h) wrote), score_inout [N*W] f64.  Slot k's score
 * becomes -inf iff a slot k' < k of the same source has the same signature and had a score other than -inf ON ENTRY (the entry
 * scores are staged before anything is written).  Ranks come out in score order, so the more probable representative survives; the
 * emptied slot is refilled by the next selection.  The signature ignores what is not schedule (above) — here also the embedding a
 * slot carries — so merging is a heuristic, as for the cost beam.  1 <= W <= 64, batch % W == 0, else MTFJSP_ERR_ARG.  One launch. */
int mtfjsp_observe_mfea1_jobs(mtfjsp_handle_t h, void *out, uint8_t *mmask_out);
int mtfjsp_beam_select_policy(mtfjsp_handle_t beam, int32_t W, const double *score_in, const double *logp_job, const double *logp_mach,
                              const uint8_t *mmask, int32_t *parent_out, int32_t *from_slot_out, int32_t *job_out, int32_t *task_out,
                              int32_t *mach_out, int32_t *child_out, double *score_out);
int mtfjsp_beam_merge_slots(mtfjsp_handle_t h, int32_t W, const uint64_t *sig, double *score_inout);

/* ------------------------------------------------------------------ groups of copies: final costs, best copy, Pareto front */
/* Best-of-K evaluation keeps K copies of each of N instances in one handle of N*K (copy c of instance n = element n*K + c, made
 * with mtfjsp_fork and the index i / K) and lets every copy play its own episode.  These two calls reduce the copies on the
 * device; nothing per copy has to be read back.  The reference evaluates one schedule per instance (validate.py:60-297).
 *
 * mtfjsp_final_costs: cost4_out [batch,4] (device) = {makespan, processing energy / T, transport time, idle time} of every
 * instance's schedule as it stands, from the previous-step costs (MTFJSP_STATE_PREV_COSTS) — what validate.py:277-287 forms on the
 * host: one binary64 division, no other arithmetic.  done_out [batch] (device bytes, or NULL) = 1 where all T operations are
 * scheduled, else 0.  One launch on h's stream.  A handle that was never reset: MTFJSP_ERR_STATE.
 *
 * mtfjsp_group_reduce: h gives the device and the stream only.  cost4 [N*K,4] and done [N*K] are device arrays (any source);
 * w3cfg_host = three HOST doubles (w_mk, w_ec, w_tt), passed by value.  Per copy: mk = cost4[0], ec = cost4[1] + cost4[3],
 * tt = cost4[2], obj = (w_mk*mk + w_ec*ec) + w_tt*tt in exactly this order, uncontracted (test_all.py:536-538).  A copy is ELIGIBLE
 * iff done != 0 and none of mk, ec, tt is NaN.  Outputs (device; each may be NULL):
 *   obj_out [N*K]       obj, NaN for an ineligible copy
 *   best_out [N]        n*K + c of the eligible copy with the smallest obj, the lowest c among equal ones (comparisons only; an
 *                       eligible copy whose obj is NaN — possible only with infinite costs — is never chosen); -1 if there is none
 *   best_obj_out [N]    that copy's obj; NaN if there is none
 *   front_out [N*K]     1 iff the copy is eligible and no eligible c' of its group dominates it: mk' <= mk && ec' <= ec && tt' <= tt
 *                       and (one of the three strictly smaller, or all three equal and c' < c) — of exact duplicates the lowest
 *                       index stays on the front; else 0
 * 1 <= K <= 4096 (the copies of a group live in one workgroup's LDS, 32 bytes each), N >= 1, N*K < 2^31: otherwise
 * MTFJSP_ERR_ARG and nothing is written.  One launch, one workgroup per group, on h's stream. */
int mtfjsp_final_costs(mtfjsp_handle_t h, double *cost4_out, uint8_t *done_out);
int mtfjsp_group_reduce(mtfjsp_handle_t h, int32_t N, int32_t K, const double *cost4, const uint8_t *done, const double *w3cfg_host,
                        double *obj_out, int32_t *best_out, double *best_obj_out, uint8_t *front_out);

/* ------------------------------------------------------------------ plans evaluated in one launch */
/* mtfjsp_replay_plans: what mtfjsp_reset, T x mtfjsp_step and mtfjsp_final_costs give for known plans — the replay every search on
 * plans below pays per round or generation — in ONE launch, bit for bit: cost4_out [batch,4] and done_out [batch] (device) as
 * mtfjsp_final_costs writes them after the T steps.  The reference replays a plan step by step on the host (pdrs:465-540).
 * task, mach: device int32 [T, stride] in history layout, row s = the actions of step s, copy b = column b (stride >= batch: the
 * buffers of mtfjsp_plan_neighbours and mtfjsp_plan_offspring, or a column-offset view of larger ones).  The handle needs loaded
 * instances and no prior reset; left_shift and the shape are its configuration's.
 * Per step only the scheduling part of the step (env:1476-1685): the validity tests (index range, already scheduled, job
 * predecessor unscheduled), the empty route, the front of the route, the gap search, the append, and the route links; a rejected
 * action changes nothing and the following actions are still tried, exactly as mtfjsp_step does; t[a][m] < 0 is scheduled like any
 * duration (MTFJSP_ST_INFEASIBLE today).  Of the cost part only what the final costs depend on: the transport time accumulated in
 * step order (env:872-876), and after the last step the per-job chain of estimated finishes (env:1920-1999; an operation whose finish
 * is 0.0 counts as having no real finish) for the makespan, numpy's pairwise sum of the processing energies (env:896), the idle
 * terms in (machine, position) order summed left to right (dg:144-170), and the one binary64 division of mtfjsp_final_costs.
 * done = all T operations scheduled; a copy that is not done gets four NaNs in cost4_out (mtfjsp_step leaves estimates of a partial
 * schedule there): mtfjsp_group_reduce, mtfjsp_walk_accept and mtfjsp_front_rank make such a copy ineligible from done alone.
 * No observation, reward, RewardScaling word, mask or machine feature is read or written.
 * flags: 0, or MTFJSP_REPLAY_STATE: every copy's per-task records (machine, start, duration, energy, route links) are written as the T
 * step launches would leave them, copies with rejected actions included.
 * After the call the handle is REPLAYED until the next mtfjsp_reset / mtfjsp_reset_episode (or a fork of a state into it) clears it:
 *   with MTFJSP_REPLAY_STATE   mtfjsp_critical_path, mtfjsp_state_signature and mtfjsp_read_state_host of MTFJSP_STATE_MACHINE, _START,
 *                              _FINISH, _ROUTES work on the replayed schedules; without it they return MTFJSP_ERR_STATE
 *   either way                 everything that reads other dynamic state or the observation returns MTFJSP_ERR_STATE with a message:
 *                              mtfjsp_step*, mtfjsp_final_costs, mtfjsp_fork from it with MTFJSP_FORK_STATE or _OBS, the masks, the
 *                              snapshots, the other selectors of mtfjsp_read_state_host
 * MTFJSP_ERR_ARG, nothing written: a null pointer, stride < batch, flags with another bit, an output that overlaps the plans or
 * the other output, a shape whose single copy does not fit a workgroup's LDS.  MTFJSP_ERR_STATE: no instances loaded.
 * One launch (k_replay_plans) on h's stream, nothing read back: one wavefront per copy, G copies per workgroup, each copy's
 * schedule and its per-step operands (duration, power, transport time from the job predecessor's planned machine, gathered from
 * the plan before the first step) in its own LDS region, 62 bytes per task plus 8 n_machine^2 for the transport times.
 *
 * mtfjsp_replay_launch_info_for: that launch's G and dynamic LDS bytes for a shape where a workgroup may use lds_max bytes (gfx950:
 * 160 KiB), no GPU needed: G = the largest of 4, 2, 1 whose regions stay within min(64 KiB, lds_max) and with G < 2 * batch; a
 * single region may take up to lds_max.  MTFJSP_ERR_ARG: a shape mtfjsp_create refuses, or one copy does not fit. */
enum { MTFJSP_REPLAY_STATE = 1 };
int mtfjsp_replay_plans(mtfjsp_handle_t h, const int32_t *task, const int32_t *mach, int64_t stride, double *cost4_out, uint8_t *done_out,
                        int32_t flags);
int mtfjsp_replay_launch_info_for(int32_t n_job, int32_t n_machine, int32_t batch, int64_t lds_max, int32_t *group_out, int64_t *lds_bytes_out);

/* ------------------------------------------------------------------ local search on plans: neighbourhood moves */
/* Improvement of a schedule the library already has, over the best-of-K machinery above: every group's incumbent plan becomes K
 * neighbouring plans in one launch, the K copies replay them (mtfjsp_reset, T x mtfjsp_step), mtfjsp_final_costs and
 * mtfjsp_group_reduce keep the best, and its best_out is the next round's src_col: T + 4 launches a round, nothing read back.
 * Copy 0 is the incumbent itself and the reduction keeps the lowest copy among equal objectives, so the incumbent survives ties and
 * the best objective never rises: hill climbing by construction.  The reference has no improvement step.
 *
 * A plan is the flexible-job-shop encoding: step s dispatches the next operation of job q[s] = task[s] / n_machine, and every task
 * a = j*n_machine + o has a machine mu[a] (= mach[s] where task[s] == a).  Any permutation of q is a plan: a move needs no repair.
 *
 * mtfjsp_plan_neighbours: h = the handle of the copies (batch = N*K, copy c of group n = element g = n*K + c); it gives t (the
 * feasible machines), the device and the stream, and must hold instances (MTFJSP_ERR_STATE otherwise).  src_task, src_mach: device
 * int32 [T, src_stride] in history layout, row s = the action of step s; the incumbent of group n is column src_col[n] (device
 * int32 [N]) or, with src_col == NULL, column n.  task_out, mach_out: device int32 [T, N*K], row s ready for mtfjsp_step.
 * kind_out: device int8 [N*K] or NULL: -1 for copy 0, else the move drawn (1 SWAP, 2 INSERT, 4 REASSIGN), whether or not it
 * changed the plan.
 *   copy 0      the incumbent, unchanged; no draw
 *   copy c >= 1 w0..w3 = Philox4x32-10 of counter ((uint32)(first_instance + n), c, (uint32)round, 0x6d6f7665 "move") under the key
 *               ((uint32)seed, (uint32)(seed >> 32)).  ONLY THE LOW 32 BITS of the instance number and of the round enter the
 *               counter: first_instance and first_instance + 2^32 give one stream.  The instance number is global (first_instance
 *               = the group's offset in the caller's set), so results do not depend on how the set is cut into passes.  Every
 *               uniform integer below n is (w * n) >> 32.  moves = the allowed kinds as a bit mask; the kind drawn is the
 *               ((w0 * popcount(moves)) >> 32)-th set bit of it; x = (w1 * T) >> 32.
 *     SWAP      y = (w2 * (T-1)) >> 32, y += (y >= x): q[x] and q[y] change places (equal jobs: the plan stays as it is)
 *     INSERT    the same x, y: the element at x is taken out and put in at position y, those between move by one
 *     REASSIGN  a = task[x]; F = the machines m != mu[a] with t[a][m] >= 0 in ascending order; mu[a] = F[(w2 * |F|) >> 32], and
 *               nothing where F is empty
 *   decode      task'[s] = q'[s]*n_machine + (number of s' < s with q'[s'] == q'[s]), mach'[s] = mu'[task'[s]]: the machine
 *               travels with the operation, not with the position
 * Every input is device data that is never read back: a src_col[n] outside [0, src_stride), or an incumbent with a task outside
 * [0, T) or a machine outside [0, n_machine), writes -1 to all rows of all K copies of that group — mtfjsp_step rejects them and
 * done stays 0, which makes them ineligible for mtfjsp_group_reduce.  An incumbent that is in range but no plan (wrong operation
 * counts) gives in-range or -1 entries.  No access leaves the arrays either way.
 * MTFJSP_ERR_ARG, nothing written: K < 1, batch % K != 0, moves == 0 or > 7, a null src_task / src_mach / task_out / mach_out,
 * src_stride < 1, an output array that overlaps a source array or another output; n_job*n_machine too large for 16 plans in a
 * workgroup's LDS (beyond about 1900).
 * One launch (k_plan_neighbours) on h's stream, no read-back, no synchronisation: a workgroup builds 64 (32, 16 for larger T)
 * consecutive copies in LDS and stores every row as one contiguous run. */
enum { MTFJSP_MOVE_SWAP = 1, MTFJSP_MOVE_INSERT = 2, MTFJSP_MOVE_REASSIGN = 4 };
int mtfjsp_plan_neighbours(mtfjsp_handle_t h, int32_t K, const int32_t *src_task, const int32_t *src_mach, int64_t src_stride,
                           const int32_t *src_col, uint64_t seed, uint64_t round, uint64_t first_instance, uint32_t moves,
                           int32_t *task_out, int32_t *mach_out, int8_t *kind_out);

/* mtfjsp_critical_path: one critical path per row out of the scheduling state of h as it stands — which operations and which
 * machine hand-overs make the schedule as long as it is.  h: any handle that has been reset, or replayed with MTFJSP_REPLAY_STATE (MTFJSP_ERR_STATE otherwise).  col:
 * device int32 [n], row i describes instance col[i] of h (any order, repeats allowed); NULL = the identity, and n must then be the
 * batch.  Outputs (device): path_task int32 [n,T], path_arc int8 [n,T], path_len int32 [n].  The rule uses only what
 * mtfjsp_read_state_host exports (machine, start, finish = start + duration: the addition the step performs, routes) and tt:
 *   tasks     only the scheduled tasks (machine >= 0) of instance col[i].  col[i] outside [0, batch), or nothing scheduled:
 *             path_len = 0 and the row is all -1
 *   first     path_task[0] = the scheduled task with the largest finish time, the lowest task index among equal ones
 *   arcs      of a task a on machine m: mp = its route predecessor (none for the first of a route), jp = a - 1 (none for
 *             operation 0 of a job).  a is MACHINE-TIGHT iff st[a] == ft[mp] + xm, xm = tt[m][m] if mp is of a's job, else 0.0
 *             (the step's own rule for a route neighbour); JOB-TIGHT iff st[a] == ft[jp] + tt[machine of jp][m].  Both are binary64 equalities of the very sums
 *             the step formed when it placed a (appending, in front of the route, in a gap): exact, not approximate
 *   walk      from a to mp if machine-tight (arc kind 1), else to jp if job-tight (arc kind 0), else the path ends at a
 *   encoding  path_arc[k] = the kind of the arc from path_task[k] to path_task[k+1]; -1 for the last element; path_task and
 *             path_arc are -1 at and after path_len; path_len <= T
 * Without left shift every task of a complete schedule is tight on one side until a start at 0.0 is reached; with left shift a task
 * put in front of a route or into a gap can leave its successor tight on neither side, and the path ends there.
 * MTFJSP_ERR_ARG, nothing written: a null output, n < 1, col == NULL with n != batch.
 * One launch (k_critical_path) on h's stream, nothing read back: one wave per row, lanes over tasks; the walk is pointer doubling
 * in LDS (position k applies the table of 2^b steps where bit b of k is set), comparisons and the two sums above only.
 *
 * mtfjsp_plan_neighbours_critical: mtfjsp_plan_neighbours with two more kinds of move, directed by a critical path per group:
 * path_task, path_arc [N,T] and path_len [N] (device; row n belongs to group n) as mtfjsp_critical_path writes them for the
 * incumbents' schedules.  moves is a mask in 1..31; Philox draw, tag, w0..w3 and the choice of the kind — the
 * ((w0 * popcount(moves)) >> 32)-th set bit in ascending order 1, 2, 4, 8, 16 — are mtfjsp_plan_neighbours'.  With moves <= 7 the
 * path arrays are not read (they may be NULL) and the output is mtfjsp_plan_neighbours' word for word.  pos[a] = the position of
 * task a in the incumbent, L = path_len[n]:
 *     CRIT_SWAP      A = the ascending k in [0, L-1) with path_arc[k] == 1 and path_task[k], path_task[k+1] of different jobs.  A
 *                    empty: the identity.  Else k = A[(w1 * |A|) >> 32], v = path_task[k], u = path_task[k+1], and INSERT with
 *                    x = pos[v], y = pos[u] (the element at x taken out and put in at y, whichever is larger); decode as always
 *     CRIT_REASSIGN  L == 0: the identity.  Else a = path_task[(w1 * L) >> 32], then as REASSIGN with this a: F = the other
 *                    feasible machines in ascending order, mu[a] = F[(w2 * |F|) >> 32], nothing where F is empty
 * kind_out names the kind drawn (8, 16) whether or not it changed the plan.  With a crit bit in moves, a path_len[n] outside [0, T]
 * or a path_task[n][k], k < path_len[n], outside [0, T) writes -1 to all K copies of group n, as a bad incumbent does.
 * MTFJSP_ERR_ARG, nothing written: as mtfjsp_plan_neighbours with moves > 31; a crit bit with a null path array; an output that
 * overlaps one of the three path arrays.  mtfjsp_plan_neighbours itself keeps refusing moves > 7. */
enum { MTFJSP_MOVE_CRIT_SWAP = 8, MTFJSP_MOVE_CRIT_REASSIGN = 16 };
int mtfjsp_critical_path(mtfjsp_handle_t h, int32_t n, const int32_t *col, int32_t *path_task, int8_t *path_arc, int32_t *path_len);
int mtfjsp_plan_neighbours_critical(mtfjsp_handle_t h, int32_t K, const int32_t *src_task, const int32_t *src_mach, int64_t src_stride,
                                    const int32_t *src_col, uint64_t seed, uint64_t round, uint64_t first_instance, uint32_t moves,
                                    int32_t *task_out, int32_t *mach_out, int8_t *kind_out, const int32_t *path_task, const int8_t *path_arc,
                                    const int32_t *path_len);

/* ------------------------------------------------------------------ a walk on plans: tabu ring, threshold and late acceptance */
/* The local search above never takes a step that is not strictly better, and ends in the first local optimum of its neighbourhood.
 * mtfjsp_walk_accept takes mtfjsp_group_reduce's place in its round and may step sideways or uphill; the incumbent is then no longer
 * the best plan met, so the best is kept beside it.  A round: mtfjsp_plan_neighbours, mtfjsp_reset, T x mtfjsp_step,
 * mtfjsp_final_costs, mtfjsp_state_signature, mtfjsp_walk_accept — T + 5 launches, nothing read back; next_col is the next round's
 * src_col.  The reference has no improvement step.
 *
 * mtfjsp_walk_accept: h gives T, the device and the stream only.  N groups of K copies, copy c of group n = element g = n*K + c; copy 0
 * is the incumbent.  cost4 [N*K,4], done [N*K], w3cfg_host: as for mtfjsp_group_reduce.  sig: device u64 [N*K], what
 * mtfjsp_state_signature wrote for the copies after their replay, or NULL.  task, mach: device int32 [T, N*K], the plans this round
 * replayed (history layout).  STATE, device arrays the caller keeps from call to call and never has to look into: late binary64
 * [N, late_len], tabu u64 [N, tabu_len], tabu_n int32 [N], best_obj binary64 [N], best_task, best_mach int32 [T, N] (history layout,
 * column n = group n).  With late_len == 0 late, with tabu_len == 0 tabu and tabu_n are neither read nor written and may be NULL.
 * The rule for group n:
 *   1 objectives   obj[c] and eligibility exactly as mtfjsp_group_reduce forms them — mk = cost4[0], ec = cost4[1] + cost4[3], tt =
 *                  cost4[2], obj = (w_mk*mk + w_ec*ec) + w_tt*tt, uncontracted; eligible iff done != 0 and none of mk, ec, tt is NaN;
 *                  obj[c] = NaN for an ineligible copy.  cur = obj[0]
 *   2 first call   first != 0: late[n][0 .. late_len) = cur, tabu_n[n] = 0, best_obj[n] = cur, and column n of best_task / best_mach =
 *                  column n*K of task / mach, word for word, whatever it holds; nothing of the state is read
 *   3 candidates   c = 1 .. K-1 with obj[c] not NaN; where sig is given also sig[g] != sig[n*K] (the incumbent's own schedule again is
 *                  no move) and sig[g] none of the valid ring entries tabu[n][0 .. min(tabu_n[n], tabu_len)).  barred = the number of
 *                  copies c >= 1 with a non-NaN obj that these two tests removed.  The ring holds signatures of SCHEDULES the walk has
 *                  left: a plan that decodes to one of them is barred however its job string looks.  No aspiration rule: a barred
 *                  schedule was an incumbent, so best_obj is not above its objective
 *   4 pick         the candidate with the smallest obj, the lowest c among equal ones (comparisons only); -1 if there is none
 *   5 why          0 if there is no pick; else 2 if cur is NaN or obj[pick] < cur; else 3 if slack >= 0 and obj[pick] <= cur + slack
 *                  (one binary64 addition; a negative or NaN slack switches this off, 0.0 admits sideways steps, +inf always moves to
 *                  the best candidate); else 4 if late_len > 0 and obj[pick] <= late[n][round % late_len] (its value before this call
 *                  writes it, after a first call's fill); else 1: refused
 *   6 move         iff why >= 2: with tabu_len > 0, tabu[n][tabu_n[n] mod tabu_len] = sig[n*K] — the schedule being left — and
 *                  tabu_n[n] += 1 (mod: the non-negative remainder); next_col[n] = n*K + pick, new cur = obj[pick].  Otherwise
 *                  next_col[n] = n*K where cur is not NaN, else -1 (what best_out of mtfjsp_group_reduce gives: a group without a
 *                  plan stays without one), new cur = cur
 *   7 late ring    late_len > 0: late[n][round % late_len] = new cur (late-acceptance hill climbing in Burke and Bykov's form: the
 *                  entry is overwritten every round, moved or not)
 *   8 best so far  on a move with best_obj[n] NaN or new cur < best_obj[n]: best_obj[n] = new cur, column n of best_task / best_mach
 *                  = column n*K + pick of task / mach, and 8 is added to why
 *   9 outputs      device, [N] each, all but next_col may be NULL: next_col int32; cur_obj_out = new cur; best_obj_out = best_obj[n]
 *                  after the call; pick_out int32 = pick (the local index c); why_out int8; barred_out int32; obj_out [N*K] = obj as
 *                  mtfjsp_group_reduce writes it.  Every value reported is the copy's own word: of -0.0 and +0.0, which are equal,
 *                  the one the copy holds
 * Signatures are compared, never computed with: two different schedules share one with probability about 2^-64, and the copy is
 * then barred without cause for as long as the entry stays in the ring — a lost candidate, never a wrong plan.
 * MTFJSP_ERR_ARG, nothing written: N < 1, K < 1 or K > 4096, N*K >= 2^31; late_len outside 0..4096; tabu_len outside 0..1024; a null
 * cost4, done, w3cfg_host, task, mach, best_obj, best_task, best_mach or next_col; late_len > 0 without late; tabu_len > 0 without tabu,
 * tabu_n or sig; a state or output array that overlaps an input array or another state or output array.
 * One launch (k_walk_accept), one workgroup per group, on h's stream, no read-back, no synchronisation: every thread keeps its own
 * copies in registers as k_group_reduce does, the ring's valid entries sit in LDS and are read by broadcast, one thread decides and
 * the workgroup copies the plan, rows over threads, only where there is a new best; every write of the state comes after every read
 * of it. */
int mtfjsp_walk_accept(mtfjsp_handle_t h, int32_t N, int32_t K, const double *cost4, const uint8_t *done, const double *w3cfg_host,
                       const uint64_t *sig, const int32_t *task, const int32_t *mach, uint64_t round, int32_t first, double slack,
                       int32_t late_len, int32_t tabu_len, double *late, uint64_t *tabu, int32_t *tabu_n, double *best_obj,
                       int32_t *best_task, int32_t *best_mach, int32_t *next_col, double *cur_obj_out, double *best_obj_out,
                       int32_t *pick_out, int8_t *why_out, int32_t *barred_out, double *obj_out);

/* ------------------------------------------------------------------ evolutionary search on plans: offspring of a population */
/* Recombination over the same machinery: a population of P plans per instance lives in one handle of N*P (member c of group n =
 * element g = n*P + c), one launch turns it into its offspring, the P copies replay them (mtfjsp_reset, T x mtfjsp_step), and
 * mtfjsp_final_costs and mtfjsp_group_reduce write what the next generation selects by: obj_out and best_out.  T + 4 launches a
 * generation, nothing read back.  Replacement is generational with one elite, so the best objective never rises.  The reference has
 * no counterpart.
 *
 * mtfjsp_plan_offspring: h = the handle of the copies (batch = N*P); it gives t, the device and the stream, and must hold instances
 * (MTFJSP_ERR_STATE otherwise).  All inputs are device data that is never read back.  src_task, src_mach: int32 [T, N*P] in history
 * layout, column g = member g: the current population.  src_obj: binary64 [N*P], what mtfjsp_group_reduce wrote as obj_out (NaN = not
 * eligible).  src_best: int32 [N], its best_out, or NULL.  cross_thr, mut_thr in [0, 2^32]: an event happens iff its Philox word is
 * below the threshold (2^32: always, 0: never).  moves: the mutation's mask, 1..7, as for mtfjsp_plan_neighbours.  task_out, mach_out:
 * int32 [T, N*P], row s ready for mtfjsp_step.  parent_out: int32 [N*P, 2] or NULL: the columns of parents A and B; B = -1 where no
 * crossover was drawn; -1, -1 for the elite.  kind_out: int8 [N*P] or NULL: -1 for the elite, 0 where no mutation was drawn, else
 * the move drawn (1, 2, 4), whether or not it changed the plan.
 * Every draw is Philox4x32-10 of counter ((uint32)(first_instance + n), c, (uint32)generation, tag) under the key ((uint32)seed,
 * (uint32)(seed >> 32)) — ONLY THE LOW 32 BITS of the instance number and of the generation enter, as in the move stream; every
 * uniform integer below n is (w * n) >> 32.  Bit i of a stream of tag X is bit i % 32 of word (i / 32) % 4 of the block of tag
 * X + i / 128.
 *   child 0     with src_best: column src_best[n] word for word (column n*P where src_best[n] is outside [n*P, (n+1)*P)); no draw.
 *               With src_best == NULL child 0 is a child like the others
 *   parents     tag 0x70617265 "pare": i_k = (w_k * P) >> 32, k = 0..3.  A = the better of members i0 and i1, B = the better of i2
 *               and i3: the smaller src_obj; a NaN loses to any number; equal values, or two NaNs, go to the lower member index
 *   crossover   tag 0x63726f73 "cros": iff w0 < cross_thr.  Precedence-preserving order crossover of the job strings q_A, q_B
 *               (q[s] = task[s] / n_machine): job j is in S iff bit j of the stream of tag 0x6a736574 "jset" is set; q'[s] = q_A[s]
 *               where q_A[s] is in S; the other positions, ascending, take the entries of q_B that are not in S in q_B's order.  The
 *               machine of task a is mu_A[a] if bit a of the stream of tag 0x6d616368 "mach" is set, else mu_B[a].  Without
 *               crossover q' = q_A, mu' = mu_A
 *   mutation    the same "cros" block: iff w1 < mut_thr.  One move exactly as mtfjsp_plan_neighbours defines SWAP, INSERT and
 *               REASSIGN, from the words of tag "move" with round = generation, applied to q' and mu' (REASSIGN's a = the task at
 *               position x of q' decoded)
 *   decode      as mtfjsp_plan_neighbours: task'[s] = q'[s]*n_machine + (number of s' < s with q'[s'] == q'[s]), mach'[s] = mu'[task'[s]]
 * A child of a parent that is no plan is -1 in every row (mtfjsp_step rejects it, it stays ineligible): a parent (A, and B where a
 * crossover was drawn) with a task outside [0, T) or a machine outside [0, n_machine), or one that does not hold every task exactly
 * once (wrong operation counts: the fill would run short or long, a task would have no machine).  The order of a job's operations in
 * a parent does not matter: only its job string is read.  The elite is -1 in every row iff an entry of its column is out of range.
 * parent_out and kind_out are written all the same.  No access leaves the arrays.
 * MTFJSP_ERR_ARG, nothing written: P < 1, batch % P != 0, moves == 0 or > 7, a threshold above 2^32, a null src_task / src_mach /
 * src_obj / task_out / mach_out, an output array that overlaps a source array or another output; n_job*n_machine too large for 16
 * plans in a workgroup's LDS (beyond about 1400).
 * One launch (k_plan_offspring) on h's stream, no read-back, no synchronisation: mtfjsp_plan_neighbours' tile of children in LDS;
 * a wave keeps both parents of its child in LDS and compacts the fill with ballots. */
int mtfjsp_plan_offspring(mtfjsp_handle_t h, int32_t P, const int32_t *src_task, const int32_t *src_mach, const double *src_obj,
                          const int32_t *src_best, uint64_t seed, uint64_t generation, uint64_t first_instance, uint64_t cross_thr,
                          uint64_t mut_thr, uint32_t moves, int32_t *task_out, int32_t *mach_out, int32_t *parent_out, int8_t *kind_out);

/* ------------------------------------------------------------------ Pareto-front evolutionary search: front ranks, survivors */
/* Multi-front (NSGA-II style) selection over the same machinery: the three objectives are not collapsed before selecting.  Parents
 * and children of an instance are ranked together into fronts, a crowding distance orders the members of one front, and the first P
 * of that order are the next population ((mu + lambda) survival).  The survivors are stored in selection order, so the position of
 * a member IS its fitness: mtfjsp_plan_offspring with src_obj = fit_out and src_best = NULL runs NSGA-II's crowded tournaments as
 * it stands.  A generation: mtfjsp_plan_offspring, mtfjsp_reset, T x mtfjsp_step, mtfjsp_final_costs, mtfjsp_front_rank,
 * mtfjsp_plan_survivors — T + 5 launches, nothing read back.  The reference has no counterpart.
 *
 * Both calls see N groups of K = Ka + Kb candidates in two array sets, so that parents (a) and children (b) need no concatenation:
 * candidate c < Ka of group n is element n*Ka + c of the a arrays, candidate c >= Ka element n*Kb + (c - Ka) of the b arrays.
 * Kb = 0: the b arrays are not read and may be NULL; with Kb > 0 they are required.
 *
 * mtfjsp_front_rank: h gives the device and the stream only.  cost4_a [N*Ka,4], done_a [N*Ka], cost4_b [N*Kb,4], done_b [N*Kb]:
 * device arrays as mtfjsp_final_costs writes them; w3cfg_host as for mtfjsp_group_reduce.  Per candidate, exactly as
 * mtfjsp_group_reduce forms them: mk = cost4[0], ec = cost4[1] + cost4[3], tt = cost4[2], obj = (w_mk*mk + w_ec*ec) + w_tt*tt,
 * uncontracted; ELIGIBLE iff done != 0 and none of mk, ec, tt is NaN; c' DOMINATES c iff both are eligible, mk' <= mk && ec' <= ec
 * && tt' <= tt and (one of the three strictly smaller, or all three equal and c' < c).  Outputs (device; each may be NULL):
 *   rank_out [N*K] int32      the front index by peeling: rank r holds the eligible candidates not yet ranked that no eligible
 *                             unranked candidate dominates; then r + 1, and so on.  -1 for an ineligible candidate.  Rank 0 is
 *                             front_out of mtfjsp_group_reduce on the same data; of exact duplicates the lowest index has the
 *                             lowest rank and every further one falls one rank
 *   crowd_out [N*K] binary64  the crowding distance among the members of the candidate's own rank.  Per axis x in the order mk, ec,
 *                             tt, the members ordered by (x, index): pred = the largest x_q among the members q with (x_q, q) <
 *                             (x_c, c) lexicographically, succ = the smallest among those with >, lo and hi = the rank's extremes
 *                             on the axis; d_x = +inf where pred or succ does not exist, else 0.0 where hi == lo, else
 *                             (succ - pred) / (hi - lo).  crowd = (d_mk + d_ec) + d_tt, taken literally in binary64 (an infinite
 *                             cost can make it NaN).  THEN the member of the rank with the smallest non-NaN obj, the lowest
 *                             index among equal ones, gets crowd = +inf — the one addition to the textbook rule: at most seven
 *                             members of a rank carry +inf (two per axis and this one), so where P >= 8 of a group survive and the
 *                             weights are not negative, the candidate with the smallest obj is among them.  NaN for an ineligible
 *                             candidate
 *   order_out [N*K] int32     the group's candidates in selection order, order_out[n*K + i] = the local index c of the i-th:
 *                             eligible before ineligible; then ascending rank; then descending crowd, a NaN crowd after every
 *                             number; then ascending index
 *   front_size_out [N] int32  the members of rank 0
 *   best_obj_out [N] binary64 the smallest non-NaN obj of the eligible candidates (the lowest candidate's own word among equal
 *                             ones), NaN if there is none
 * All but front_size_out's count, obj and the division and sums of crowd are comparisons.
 * Ka >= 1, Kb >= 0, 1 <= K <= 2048 (a group lives in one workgroup's LDS, 44 bytes per candidate), N >= 1, N*K < 2^31, the a
 * arrays, w3cfg_host and with Kb > 0 the b arrays not NULL: otherwise MTFJSP_ERR_ARG and nothing is written.
 * One launch (k_front_rank), one workgroup per group (one wave for K <= 64, else four), on h's stream: the peeling counts every
 * candidate's dominators once and takes every ranked candidate off the counts once — 2 K dominance tests per candidate whatever the
 * number of fronts — and per front pays one barrier and one scan of the K ranks; it stops as soon as nothing is left.  A totally
 * ordered group (every candidate a front of its own) is the slow extreme: K such rounds.
 *
 * mtfjsp_plan_survivors: h = the handle of the N*P copies; it gives T, the device and the stream.  order, rank: int32 [N*K] as
 * mtfjsp_front_rank wrote them; 1 <= P <= K.  task_a, mach_a: int32 [T, N*Ka], task_b, mach_b: int32 [T, N*Kb] in history layout;
 * cost4_a / done_a, cost4_b / done_b as above.  Output column n*P + i takes candidate c = order[n*K + i]:
 *   task_out, mach_out [T, N*P] int32   its plan, row s ready for mtfjsp_step
 *   cost4_out [N*P,4], done_out [N*P]   its costs and done byte (or NULL)
 *   rank_out [N*P] int32                rank[n*K + c] (or NULL)
 *   src_out [N*P] int32                 c, as read (or NULL)
 *   fit_out [N*P] binary64              (double)i where rank[n*K + c] >= 0, NaN otherwise (or NULL): smaller is better, NaN loses
 * An order entry outside [0, K) gives a column of -1, done_out = 0, rank_out = -1, cost4_out and fit_out NaN (src_out still holds
 * the entry).  No access leaves the arrays.
 * MTFJSP_ERR_ARG, nothing written: a null order / rank / a array / task_out / mach_out, a null b array with Kb > 0; Ka < 1, Kb < 0,
 * N < 1, N*K >= 2^31, P < 1 or P > K, batch != N*P; an output array that overlaps an input array or another output.
 * One launch (k_plan_survivors) on h's stream: row s is written as contiguous runs, the reads stay inside one group's columns. */
int mtfjsp_front_rank(mtfjsp_handle_t h, int32_t N, int32_t Ka, int32_t Kb, const double *cost4_a, const uint8_t *done_a,
                      const double *cost4_b, const uint8_t *done_b, const double *w3cfg_host, int32_t *rank_out, double *crowd_out,
                      int32_t *order_out, int32_t *front_size_out, double *best_obj_out);
int mtfjsp_plan_survivors(mtfjsp_handle_t h, int32_t N, int32_t Ka, int32_t Kb, int32_t P, const int32_t *order, const int32_t *rank,
                          const int32_t *task_a, const int32_t *mach_a, const double *cost4_a, const uint8_t *done_a,
                          const int32_t *task_b, const int32_t *mach_b, const double *cost4_b, const uint8_t *done_b,
                          int32_t *task_out, int32_t *mach_out, double *cost4_out, uint8_t *done_out, int32_t *rank_out,
                          int32_t *src_out, double *fit_out);

/* ------------------------------------------------------------------ dispatch-rule baselines */
/* = the two lists run_Rules_jointActions_withMinus_1217 fixes before its first step (tester/pdrs.py:680-753) for every instance:
 * o_rule[b] in 0..5 = FIFO (pdrs:123-125), MOR (pdrs:128-137), LWKR_T, LWKR_PT, MWKR_T, MWKR_PT (pdrs:162-286 with the "mean"
 * data type that pdrs:690-702 hard-codes); m_rule[b] in 0..1 = SPT (pdrs:46-52), SEC (pdrs:55-66); both device, [B] — rules are
 * per instance, so one handle holding N instances 12 times carries all 12 pairs of test_all.py:484-540 through one rollout.
 * mor_order device [B,M,J] (row = the job order of one column: MOR's random.shuffle, replayed) or NULL: drawn on the device, one
 * Fisher-Yates per (instance, column) from the Philox stream keyed by (seed, instance, column).  task_out, mach_out device [B,T]:
 * the (task, machine) of step s (pdrs:751-754), to be replayed through mtfjsp_step on a handle with left_shift = 0 (pdrs:669).
 * Reads t, p from the handle's device instance arrays (loaded or generated).  The rule ids are read back and checked first (one
 * small copy that synchronises the handle's stream): an id out of range returns MTFJSP_ERR_ARG and nothing is written.  The
 * plan itself is one launch on the handle's stream. */
int mtfjsp_pdr_plan(mtfjsp_handle_t h, const int32_t *o_rule, const int32_t *m_rule, const int32_t *mor_order, uint64_t seed,
                    int32_t *task_out, int32_t *mach_out);

/* ------------------------------------------------------------------ exports (compat / tests) */
/* dense adj_wrk [B,T,T] f64, row = destination, diagonal 1 (env:2066-2073) — what pe:136 returns. */
int mtfjsp_export_dense_adj(mtfjsp_handle_t h, double *out);
/* same, into HOST memory (the reference returns adj as a host numpy array, pe:136,263); the [B,T,T] device scratch is
 * allocated inside the handle on first use — compatibility path for small batches */
int mtfjsp_export_dense_adj_host(mtfjsp_handle_t h, double *out_host);
/* gym-style valid_action_mask (env:2535-2575): [B,T] 1 = selectable */
int mtfjsp_valid_action_mask(mtfjsp_handle_t h, uint8_t *out);
enum {
    MTFJSP_STATE_MACHINE = 0,   /* int32 [B,T]   machine of task, -1 unscheduled       (G.nodes[k]['machine'])      */
    MTFJSP_STATE_START = 1,     /* f64   [B,T]   start time, NaN unscheduled           (…['start_time'])            */
    MTFJSP_STATE_FINISH = 2,    /* f64   [B,T]   finish time, NaN unscheduled          (…['finish_time'], ppo:271)  */
    MTFJSP_STATE_ROUTES = 3,    /* int32 [B,M,T] task indices in processing order, -1 padded (env.machine_routes)   */
    MTFJSP_STATE_PREV_COSTS = 4,/* f64   [B,4]   makespan/e1/trans/idle _previous_step  (run:632-633)               */
    MTFJSP_STATE_SCALER = 5,    /* f64   [B,17]  R[4], n, mean[4], S[4], std[4]         (pt:54-124)                 */
    MTFJSP_STATE_W3 = 6         /* f64   [B,3]   reward_random_weight                   (run:478)                   */
};
int mtfjsp_read_state_host(mtfjsp_handle_t h, int which, void *out_host);
/* writes back the RewardScaling state (MTFJSP_STATE_SCALER layout, [count,17]) of instances [first, first+count): lets a caller
 * drive ONE instance through mtfjsp_step the way the reference's gym-style env.step does (env:716-974 — no reward scaling;
 * only the batched step applies it, pe:255-260) by restoring that instance's scaler afterwards */
int mtfjsp_set_scaler_state_host(mtfjsp_handle_t h, int32_t first, int32_t count, const double *state17);
/* copy `nbytes` from a device buffer of this handle's context to host (synchronises the stream) */
int mtfjsp_copy_to_host(mtfjsp_handle_t h, void *dst_host, const void *src_dev, size_t nbytes);

/* GAE reverse scan of ppo:438-536 for one reward channel: for every instance b, s = S-1..0:
 *   delta = r[s,b] + gamma*v_next[s,b] - v[s,b] ; gae = delta + gamma*lambda*gae*(1-done[s,b]) ; adv[s,b] = gae
 * r, v, v_next are f32 with element strides (stride_s, stride_b) so packed trajectory buffers can be passed as views;
 * done and adv are [S,B] contiguous.  The result is NOT normalised (that needs the all-gather across GPUs). */
int mtfjsp_gae(mtfjsp_handle_t h, int32_t S, const float *r, int64_t r_ss, int64_t r_sb, const float *v, int64_t v_ss, int64_t v_sb,
               const float *v_next, int64_t n_ss, int64_t n_sb, const float *done, float gamma, float lambda, float *adv);
/* Global advantage normalisation of the hand-off (ppo:485,532): `(adv - adv.mean()) / (adv.std() + 1e-5)` with torch's unbiased
 * std, per tensor over ALL shards' columns.  gathered = [world][K_total][S][B] f32 — what ONE all-gather of the packed
 * [K_total,S,B] buffer leaves on every rank (world = 1: the packed buffer itself); the first K <= K_total <= 16 tensors are
 * advantages to normalise, the others (the value tensors of the whole hand-off, ppo:628-703) only ride along.  norm_out [K][S][B]
 * receives this rank's normalised advantages; targets_out (may be NULL) [K][S][B] = normalised advantage + value at act time
 * (ppo:668-671,689) with values[k] an f32 [S,B] view given by element strides (NULL entries are skipped); full_out (may be NULL)
 * [K_total][S][world*B] receives every gathered tensor in the reference's single-process layout (rank-major column blocks).
 * Two launches on the handle's stream; f64 statistics from per-block partial sums in a fixed order: bit-reproducible. */
int mtfjsp_normalize_advantages(mtfjsp_handle_t h, int32_t K, int32_t K_total, int32_t world, int32_t rank, int32_t S, const float *gathered, float eps,
                                const float *const *values, const int64_t *value_stride_s, const int64_t *value_stride_b,
                                float *norm_out, float *targets_out, float *full_out);
/* K strided f32 [S,B] views -> one packed [K][S][B] buffer in one launch (the value tensors that ride in the hand-off's all-gather
 * beside the advantages; the reference stacks them with torch.cat, ppo:657-703) */
int mtfjsp_pack_views(mtfjsp_handle_t h, int32_t K, int32_t S, const float *const *src, const int64_t *stride_s, const int64_t *stride_b, float *out);

/* kernel timing hook for bench.py: HIP events recorded on the handle's stream around every step launch
 * between begin/end; returns accumulated milliseconds and launch count. */
int mtfjsp_timing_begin(mtfjsp_handle_t h);
int mtfjsp_timing_end(mtfjsp_handle_t h, double *step_ms_total, int64_t *step_launches);

/* measurement only (the step kernel's achieved bytes/s are to be compared with "the measured copy bandwidth of a
 * same-footprint streaming kernel on the same GPU"): `reps` launches of a kernel that reads read_bytes and writes write_bytes
 * with access_bytes-wide (4, 8 or 16), fully coalesced accesses on `grid` workgroups of 256 threads, HIP events around every
 * launch on the handle's stream; returns the average and the minimum launch duration in microseconds.  Scratch buffers are
 * allocated and freed inside the call.  Replaces nothing in the reference (no reference counterpart). */
int mtfjsp_footprint_copy(mtfjsp_handle_t h, size_t read_bytes, size_t write_bytes, int32_t access_bytes, int32_t grid, int32_t reps,
                          double *avg_us_out, double *min_us_out);

/* ------------------------------------------------------------------ encoder (rollout forward passes) */
typedef struct {
    int32_t n_job, n_machine, batch;
    int32_t hidden;            /* gcn_hidden_dim == machine_hidden_dim == 128 (parameters.py:106,109) */
    int32_t obs_dtype;         /* dtype of tasks_fea / m_fea1 / m_fea2 handed to the forwards */
    int32_t device_id;
} mtfjsp_encoder_config_t;

int mtfjsp_encoder_create(const mtfjsp_encoder_config_t *cfg, mtfjsp_encoder_t *out);
int mtfjsp_encoder_destroy(mtfjsp_encoder_t e);
const char *mtfjsp_encoder_last_error(mtfjsp_encoder_t e);
int mtfjsp_encoder_set_stream(mtfjsp_encoder_t e, void *hip_stream);
/* Weights by the reference's state_dict key, prefixed "job_actor." or "machine_actor."
 * (e.g. "job_actor.encoder.feature_extract.mlps.0.linears.0.weight"); f32, row-major as in torch.
 * Loading a tensor again on a used handle (rollout, update on the host, load, rollout) writes over the same device buffers — the plain
 * copy and every image derived from it; nothing is allocated after the first load and the first forward of each kind.
 * Ordering: the call first waits for everything enqueued on the handle's stream (mtfjsp_encoder_set_stream), so a forward enqueued
 * BEFORE it computes with the weights it was enqueued under, and returns when its copies have landed, so a forward enqueued AFTER
 * it computes with the new tensor (the fused GAT projections, which depend on three tensors, are formed by the next forward that
 * needs them, after the same wait).  data_host may be freed on return.  Work on OTHER streams that reads this handle's outputs is
 * not waited for; loading between the two forwards of one decision mixes two policies, as it would anywhere. */
int mtfjsp_encoder_load_weight_host(mtfjsp_encoder_t e, const char *name, const float *data_host, int64_t numel);
int mtfjsp_encoder_weights_ready(mtfjsp_encoder_t e);     /* 0 when every required tensor has been loaded */

/* = Operation_Actor_JointAction_selfCritic.forward (ac:104-296) without the sampling:
 * GIN encoder (gcn:109-197, training-mode BatchNorm over all B*T rows), candidate scorer, masked softmax,
 * local critic.  h_m_prev may be NULL (first step: learned `_input`, ac:229-233).
 * Outputs (f32): prob [B,J], h_pooled [B,H], job_v [B,2]; h_nodes [B*T,H] optional (NULL = keep internal).
 * candidate [B,J]: any task row in [0, T) per job (ac:197-207 gathers by index).  The environment's candidates lie in their job's
 * own block of rows, candidate[b][j] in [j M, (j+1) M) (ppo:306-309), which the streaming pool/gather kernel of the large shapes
 * exploits (it picks them out of the row stream); a candidate outside its block takes a dependent gather there — same result. */
int mtfjsp_job_actor_forward(mtfjsp_encoder_t e, const void *tasks_fea, const int32_t *ell_col,
                             const float *ell_val, const int32_t *candidate, const uint8_t *job_mask,
                             const float *h_m_prev, float *prob, float *h_pooled, float *job_v, float *h_nodes);
/* = Machine_Actor_JointAction_selfGAT_selfCritic.forward (ac:359-498; GATLayer gat:82-159).
 * Outputs (f32): prob [B,M], h_pooled [B,H], machine_v [B,2]. */
int mtfjsp_machine_actor_forward(mtfjsp_encoder_t e, const void *m_fea1, const void *m_fea2,
                                 const float *h_pooled_o, const uint8_t *mmask, float *prob, float *h_pooled,
                                 float *machine_v);
/* = Global_Critic_JointAction_GAT.forward (ac:587-750; SURVEY §8f N1, used under no_grad by ppo:628-703 to sample the
 * global values for GAE): weights under the prefix "global_critic." (loaded with mtfjsp_encoder_load_weight_host);
 * value4 [B,4] f32 = (mk, pt, tt, it). */
int mtfjsp_global_critic_forward(mtfjsp_encoder_t e, const void *tasks_fea, const int32_t *ell_col, const float *ell_val,
                                 const void *m_fea1, const void *m_fea2, float *value4);
/* = select_operation_action / greedy_select_action / select_machine_action (agent:22-72):
 * categorical sample (Philox, (seed,counter)) or argmax from prob [B,N]; idx_out [B], logp_out [B];
 * gather_from (optional, [B,N] int32, e.g. candidate) -> gathered_out [B] (task index). */
int mtfjsp_sample_categorical(mtfjsp_encoder_t e, const float *prob, int32_t n, int32_t greedy, uint64_t seed,
                              uint64_t counter, int32_t *idx_out, float *logp_out, const int32_t *gather_from,
                              int32_t *gathered_out);
/* Device-side recipe of Parallel_env.cal_cur_task_machine_feature (pe:152-214) for ONE decision: everything
 * mtfjsp_observe_mfea1 reads and writes, as plain device pointers, so that the job actor's heads kernel can produce
 * m_fea1 / the machine mask for the task it has just selected (one launch less between the two actor forwards).
 * Filled by mtfjsp_get_mfea1_context (environment side), consumed by mtfjsp_encoder_arm_mfea1 (encoder side). */
typedef struct {
    const double *t, *p, *tt, *mean3;   /* [B,T,M], [B,T,M], [B,M,M], [B,T,3] */
    const int32_t *shop;                /* [B,M] */
    const void *link;                   /* [B,T] 16-byte task records {f64 energy estimate; i16 machine, prev, pos, next}: the machine of task v is the i16 at byte 16 v + 8 */
    void *m_fea1_out;                   /* [B,M,6] obs dtype */
    uint8_t *mmask_out;                 /* [B,M] */
    int32_t T, M, obs_f32;
    const void *m_fea2;                 /* [B,M,8] obs dtype: the environment's bound machine features (may be NULL).  With it the
                                         * job actor's heads launch can also run the machine actor's GAT passes on (m_fea1_out, m_fea2)
                                         * — the mtfjsp_machine_actor_forward that follows with exactly these two pointers skips them */
} mtfjsp_mfea1_ctx_t;
int mtfjsp_get_mfea1_context(mtfjsp_handle_t h, void *m_fea1_out, uint8_t *mmask_out, mtfjsp_mfea1_ctx_t *ctx);
/* ---- One-shot arms: mtfjsp_encoder_arm_selection (which = 0, 1), _arm_mfea1, _arm_machine_heads, _arm_env_step, _arm_values_only.
 * AN ARM BELONGS TO THE NEXT CALL OF THE FORWARD IT NAMES, AND TO NO LATER CALL.  A forward that returns MTFJSP_OK takes what is its
 * own: a job forward that does not run the machine heads itself leaves the machine selection and the environment step to the machine
 * forward that follows, and a values-only pair is one job forward and one machine forward.  A forward that returns an error — any
 * error, from any of its checks: MTFJSP_ERR_RETRY at its entry, MTFJSP_ERR_ARG, MTFJSP_ERR_STATE, MTFJSP_ERR_HIP — leaves
 * NOTHING armed on the handle: the pair the arms were made for is void (and so is work a launch did ahead for it).  mtfjsp_encoder_check does the same when it returns MTFJSP_ERR_RETRY.  The caller arms again for the
 * forwards it repeats; no later forward ever selects, writes m_fea1, runs the machine heads or steps the environment through
 * pointers armed for an earlier one.  mtfjsp_encoder_env_step_fused() speaks of the last forward pair only: 0 after any pair that
 * had no armed step, whichever launch served it. */
/* The WHOLE machine actor forward (ac:359-498) inside the job actor's heads launch: three launches per rollout step.  With these
 * outputs armed (prob [B,M], h_pooled [B,H], machine_v [B,2]; one-shot), a machine selection armed (mtfjsp_encoder_arm_selection,
 * which = 1) and an mfea1 context with m_fea2 (above), the NEXT mtfjsp_job_actor_forward — where the shape allows it: one workgroup
 * of 16 instances per CU, all co-resident (the single-launch GIN kernel's census), split products — also runs the machine path's
 * GAT passes, exchanges the BatchNorm sums of the B*M machine nodes (ac:434) between its workgroups inside the launch
 * (count-carrying integer atomics as in the single-launch GIN kernel; the wait is bounded, a time-out surfaces as
 * MTFJSP_ERR_RETRY) and the machine heads with their selection.  The mtfjsp_machine_actor_forward that follows with exactly the
 * pointers involved (m_fea1_out, m_fea2, that job forward's h_pooled, mmask_out, these outputs) finds itself done and returns at
 * once; with any other argument it recomputes (and selects again with the machine selection the launch consumed).  The match is by
 * POINTER IDENTITY, as for m_fea2: a caller that rewrites m_fea1 / the machine mask IN PLACE between the two forwards (a forced task
 * through mtfjsp_observe_mfea1 into the same buffers) must not arm the machine heads for that step.  The mode setters
 * (set_bn_mode, set_stats_reduce, set_product_mode) and mtfjsp_global_critic_forward discard a forward done ahead.
 * Where the shape does not allow it nothing changes.  MTFJSP_NO_FUSED_MHEADS=1: off.
 * mtfjsp_encoder_fused_launches: how many forwards took the three-in-one launch so far (tests, bench). */
int mtfjsp_encoder_arm_machine_heads(mtfjsp_encoder_t e, float *prob, float *h_pooled, float *machine_v);
int mtfjsp_encoder_fused_launches(mtfjsp_encoder_t e, int64_t *three_in_one_out);
/* The post-terminal forward pair of an episode (Run.py:455-475: job actor on the terminal observation, machine actor on the last
 * decision's m_fea1) keeps only the two local critics' values (replaybuffer.py:131-139).  Armed with this call, the NEXT
 * mtfjsp_job_actor_forward and the NEXT mtfjsp_machine_actor_forward write job_v / machine_v and the pooled embeddings as always —
 * bit-identical — and skip the scorer: prob (and any selection output) is left untouched.  One-shot; ignored (full forward) for a
 * forward with an armed selection / m_fea1 context, with per-instance BatchNorm or with the f32-instruction heads. */
int mtfjsp_encoder_arm_values_only(mtfjsp_encoder_t e);
/* BatchNorm statistics of the two actor forwards (every BatchNorm in the reference is in training mode):
 * per_instance = 0 (default): over all rows of the device batch = one reference run with env_batch = B (training rollout);
 * per_instance = 1: over the rows of ONE instance = B independent reference runs with env_batch = 1, i.e. the greedy
 * evaluation of validate.py:60-297 batched over the evaluation set.  Not applied to the global critic. */
int mtfjsp_encoder_set_bn_mode(mtfjsp_encoder_t e, int32_t per_instance);
/* Exact big-batch BatchNorm over several shards (optional): with a reduction callback set, every BatchNorm of the
 * forwards normalises over the rows of ALL shards.  After the launch that completes a BatchNorm's column sums the library
 * synchronises its stream and calls fn(user, sums, count): `sums` is DEVICE memory holding `count` doubles, which the callback
 * replaces by their element-wise sum over the shards (e.g. one all-reduce) and returns 0 once that is in place.
 * global_batch = instances of all shards together (>= this handle's batch).  7 calls per actor pair forward; the GIN encoder
 * then runs as its streaming launches (the single-launch kernel cannot exchange data mid-launch).  fn = NULL: off.  Per-shard
 * statistics (the default) are what DESIGN.md §7 describes: each GPU behaves like a reference run with env_batch = its shard. */
typedef int (*mtfjsp_stats_reduce_fn)(void *user, double *sums, int32_t count);
int mtfjsp_encoder_set_stats_reduce(mtfjsp_encoder_t e, mtfjsp_stats_reduce_fn fn, void *user, int64_t global_batch);
/* deferred = 1: the forward entries stop polling the asynchronous failure words (see mtfjsp_encoder_check); a failure then
 * surfaces only at mtfjsp_encoder_check.  For callers whose forwards contain collectives (the reduction callback above): every
 * shard must issue the same sequence of forwards, so a shard-local MTFJSP_ERR_RETRY may only be acted upon at a point all shards
 * agree on — rollout.py checks once per step and lets the shards agree through one MAX all-reduce (the reference has no
 * counterpart: its update samples the critics in one process, ppo:422-435).  Default 0.
 * Diagnostic: MTFJSP_RANGE_FAIL_AT=n raises the range word at the n-th job-actor forward of a handle (tests). */
int mtfjsp_encoder_set_deferred_poll(mtfjsp_encoder_t e, int32_t deferred);
/* How the [rows,128]x[128,128] products of the actor forwards (Linear layers of gcn:95-153 / ac:205-293, the GAT weight of
 * gat:82) are formed.  0 (default): on the 16-bit matrix cores with f32 accumulation, from f32 operands split into two f16
 * pieces (relative representation error <= 2^-22; weights pre-scaled by a power of two) and the three significant piece
 * products — measured as accurate as an f32 FMA chain of the same length (tests/test_encoder_hip.py states
 * the bounds); the 12 -> 128 first Linear, whose inputs are raw features, uses an exact three-piece bf16 split instead.
 * Bits select the f32 matrix instruction instead, as the A/B reference: 1 = GIN products, 2 = GAT passes, 4 = actor/critic
 * heads, 8 = first GIN Linear (12 -> 128) on the vector ALU.  Bit 16 is not a numerics choice: it runs the GIN encoder as six
 * streaming launches (k_gemm_x6) even where the single-launch register-resident kernel (k_gin_res; in-kernel grid-wide statistics exchanges for
 * the batch statistics) is eligible (16 <= T <= 65, <= 576 node rows per CU, census launch passed in mtfjsp_encoder_create);
 * MTFJSP_NO_RESIDENT_GIN=1 in the environment does the same for every handle. */
int mtfjsp_encoder_set_product_mode(mtfjsp_encoder_t e, int32_t f32_instruction_mask);
/* Fuse the action selection of the NEXT mtfjsp_job_actor_forward (which = 0) / mtfjsp_machine_actor_forward (which = 1) call into
 * its heads kernel: same arguments and the same Philox stream as mtfjsp_sample_categorical on that forward's `prob`
 * (agent:22-72), one launch less per decision.  One-shot: applies to one forward call. */
int mtfjsp_encoder_arm_selection(mtfjsp_encoder_t e, int32_t which, int32_t greedy, uint64_t seed, uint64_t counter,
                                 int32_t *idx_out, float *logp_out, const int32_t *gather_from, int32_t *gathered_out);
/* One-shot like mtfjsp_encoder_arm_selection (and only together with it, which = 0): the next job actor forward also
 * writes m_fea1 / the machine mask of every instance's selected task (== mtfjsp_observe_mfea1 on gathered_out). */
int mtfjsp_encoder_arm_mfea1(mtfjsp_encoder_t e, const mtfjsp_mfea1_ctx_t *ctx);
/* One-shot: the NEXT mtfjsp_machine_actor_forward also runs the environment step described by `params` (mtfjsp_step_params) in its
 * heads launch — one launch and one launch boundary less per rollout step — provided its armed selection (which = 1) writes the
 * `mach_idx` the block names and the shapes agree.  mtfjsp_encoder_env_step_fused() tells afterwards whether it did (1) or the
 * caller still has to call mtfjsp_step / mtfjsp_step_record (0: the default — the combined launch is enabled with the environment
 * variable MTFJSP_FUSED_ENV when the handle is created, because it measured slower than two launches at the headline shape —, also
 * per-instance BatchNorm mode, f32-instruction heads, kernel-time recording).  Results are those of mtfjsp_step, bit for bit (the
 * same device code). */
int mtfjsp_encoder_arm_env_step(mtfjsp_encoder_t e, const void *params, int32_t params_bytes);
int mtfjsp_encoder_env_step_fused(mtfjsp_encoder_t e);
/* ---- host-side helpers of the instance generator (instance/generate_allsize_mofjsp_dataset.py:204-216, 241-272).
 * The reference draws "k machines infeasible per task" and the transport times from numpy's legacy RandomState one python call at
 * a time; these take the same draws from the same MT19937 state (key[624] + *pos as RandomState.get_state() returns them; updated
 * in place for set_state()) at native speed, bit for bit, and keep only samples [first, first+count): t [count,T,M] gets the sign
 * flips, tt [count,M,M] is written.  No GPU involved. */
int mtfjsp_hostgen_infeasible(uint32_t *key, int32_t *pos, int64_t samples, int32_t T, int32_t M, int64_t first, int64_t count, double *t);
int mtfjsp_hostgen_transport(uint32_t *key, int32_t *pos, int64_t samples, int32_t M, const int64_t *shop_of_machine,
                             double in_lo, double in_hi, double out_hi, int64_t first, int64_t count, double *tt);
/* Synchronises the encoder's stream and reports asynchronous failures of the forwards enqueued so far.  The single-launch GIN
 * kernel exchanges its BatchNorm statistics between its workgroups inside the launch (count-carrying integer atomics; the waits
 * for the other workgroups' contributions are bounded at 4 ms); it needs all of its workgroups
 * resident at once (one per CU), which another process or another stream using the same GPU can prevent — not a hang but a
 * time-out.  The kernel then sets a host-mapped word that EVERY job-actor / global-critic forward polls on entry (a plain host
 * read, no synchronisation) and that this call reads after synchronising: the first call to see it returns MTFJSP_ERR_RETRY,
 * switches the handle to the streaming launches (slower, no co-residency requirement) and leaves the caller to recompute what
 * it enqueued since the failed launch (the Python rollout restarts the episode and discards the trajectory buffer).  A later
 * mtfjsp_encoder_check re-runs the residency census on the idle stream and re-enables the single launch when it passes.
 * *gin_resident_out (may be NULL) = 1 when the single-launch kernel is in use for this handle (shape eligible, census passed in
 * mtfjsp_encoder_create or here, product-mode bits 1, 8, 16 clear), 0 when the streaming launches are.  Only one process / stream
 * per GPU should use the single-launch path at a time (use one stream, or order handles with events).
 * Diagnostic: MTFJSP_GIN_RES_FAIL_AT=n makes the n-th single-launch forward of a handle time out (tests). */
int mtfjsp_encoder_check(mtfjsp_encoder_t e, int32_t *gin_resident_out);
/* Range of the split products.  The default kernels run every 128-deep product on the f16 matrix cores from operands split into
 * two f16 pieces: f32-accurate, but an activation beyond 65 504 (a BatchNorm gamma of several hundred, an edge weight of several
 * thousand — nothing a trained reference checkpoint produces, nothing the reference's f32/f64 arithmetic forbids) cannot be
 * represented.  It is never clamped and never silent: its pieces are (inf | -inf), their products NaN, the NaN reaches every output
 * of that forward, the heads kernel sets a host-mapped word, and the next forward entry (or mtfjsp_encoder_check) returns
 * MTFJSP_ERR_RETRY after switching the handle to the f32-instruction kernels (product mode 15, no range limit, slower): repeat
 * the forward.  mtfjsp_encoder_set_product_mode(0) returns to the split products.  *count_out = number of such switches,
 * *product_mode_out (may be NULL) = the product mode now in force. */
int mtfjsp_encoder_range_fallbacks(mtfjsp_encoder_t e, int64_t *count_out, int32_t *product_mode_out);
/* diagnostic (tools/first_launch): the first `count` floats of the machine path's node buffer [B*M,128] — the output of the three
 * GAT passes of ac:409-420 before the BatchNorm of ac:434 — copied to host memory after synchronising the stream.  The buffer is
 * written by the separate GAT launches (k_gat3x, k_headsx_gat3x) and by the global critic; the three-in-one launch keeps its node
 * rows in LDS (round 6) and leaves the buffer alone unless MTFJSP_FUSED3_NODES_HBM=1. */
int mtfjsp_encoder_peek_nodes_host(mtfjsp_encoder_t e, float *out_host, int64_t count);
/* diagnostic (tests/test_weight_reload_gpu.py): the device buffers this handle has allocated so far and their total size in bytes
 * (either pointer may be NULL).  Workspaces are allocated by mtfjsp_encoder_create, weight buffers and their derived images the first
 * time a tensor is loaded or a forward needs them; loading a tensor again reuses them, so both figures stay constant once every
 * tensor has been loaded and every kind of forward has run once.  Nothing is freed before mtfjsp_encoder_destroy.  No GPU work. */
int mtfjsp_encoder_device_allocations(mtfjsp_encoder_t e, int64_t *buffers_out, int64_t *bytes_out);
/* Which instantiation of the single-launch GIN kernel serves a forward — the library's one statement of the rule (csrc/mtfjsp_gin_res_select.h; every
 * launch goes through it).  No GPU involved.  batch instances of rows_per_instance (= n_job * n_machine) node rows on num_cu compute units; n_job bounds
 * the candidate table; candidates = candidates per instance of the forward (n_job for the job actor, 0 for the global critic); node_output != 0 when
 * the node embeddings are requested.  "k_gin_res_t36j6x16" — the body compiled for T = 36, J = 6, 16 instances in every workgroup, no node output —
 * serves exactly that shape (batch a multiple of 16 with ceil(batch / num_cu) == 16); "k_gin_res", the same body with the shape read at run time, everything
 * else that is eligible; NULL where the shape is not eligible for the single launch (the streaming launches run).  MTFJSP_GIN_RES_GENERIC=1 in the
 * environment (read per call, by the launches too) forces "k_gin_res": A/B runs and the parity test.  *ipc_out / *grid_out (may be NULL): instances per
 * workgroup and workgroups.  mtfjsp_encoder_gin_res_kernel_name: the instantiation the handle's last single-launch forward ran (NULL: none yet). */
const char *mtfjsp_gin_res_kernel_name_for(int32_t batch, int32_t rows_per_instance, int32_t n_job, int32_t candidates, int32_t num_cu,
                                           int32_t node_output, int32_t *ipc_out, int32_t *grid_out);
const char *mtfjsp_encoder_gin_res_kernel_name(mtfjsp_encoder_t e);
/* Which path a GIN forward takes, who pools, and every launch it makes, in order — the library's one statement of the rule (csrc/mtfjsp_gin_select.h; both
 * forwards plan with it and the streaming launches are that plan's steps).  No handle, no GPU.  batch instances of rows_per_instance node rows on num_cu
 * compute units; n_job bounds the candidate table; candidates = candidates per instance of the forward (0: none); product_mode as
 * mtfjsp_encoder_set_product_mode takes it.  flags: who asks, and the handle's answers that are not the shape's —
 *   MTFJSP_GIN_CRITIC        the global critic asks (otherwise the job actor, whose heads launch can pool)
 *   MTFJSP_GIN_NODE_OUTPUT   the node embeddings are requested
 *   MTFJSP_GIN_PER_INSTANCE  per-instance BatchNorm mode (mtfjsp_encoder_set_bn_mode)
 *   MTFJSP_GIN_OBS_F64       f64 observations
 *   MTFJSP_GIN_NO_SINGLE     the handle's census of co-resident workgroups has not passed (or a launch has timed out since)
 *   MTFJSP_GIN_REDUCE        a statistics reduction is installed (mtfjsp_encoder_set_stats_reduce)
 * The weights are taken as loaded.  MTFJSP_FUSE_PAIR, MTFJSP_FUSE_GIN0, MTFJSP_FUSE_POOL, MTFJSP_NO_STREAM_ORDER, MTFJSP_STREAM_NT, MTFJSP_POOL_S,
 * MTFJSP_FUSE_POOL_MAXT, MTFJSP_NO_RESIDENT_GIN and MTFJSP_GIN_RES_GENERIC are read per call, through the reader a handle uses (their defaults, and
 * when a handle reads each — MTFJSP_FUSE_POOL_MAXT only once per process —: csrc/mtfjsp_enc_switches.h and the table "Encoder switches" of DESIGN.md).
 * buf receives "path;pooling form;family:kernel,family:kernel,...": path = "per_instance" | "single_launch" | "streaming"; pooling form = "gin_kernel"
 * (the per-instance / single-launch kernel itself) | "heads" (the job actor's heads launch) | "epilogue" (the epilogue of a second pass of the last
 * product, + k_cand_fixup) | "pool_gather" (k_job_pool_gather); then each launch's timing family (mtfjsp_encoder_timing_query) and kernel.
 * order_out (may be NULL; 12 entries): per launch, GemmArgs::rev (the rows walked backwards) + 2 * GemmArgs::nt (non-temporal input reads) + 4 where
 * a statistics reduction follows the launch (the mtfjsp_encoder_set_stats_reduce callback, when one is installed).  pool_out (may be NULL; 2 entries): k_job_pool_gather's rows per
 * range (0: plain instance order) and workgroups, 0 where it does not run.  Returns the number of launches, or MTFJSP_ERR_ARG (a size out of range, buf
 * too small).
 * mtfjsp_encoder_gin_launches: the same for the handle's last GIN forward, job actor's or global critic's (MTFJSP_ERR_STATE: none yet). */
#define MTFJSP_GIN_CRITIC 1u
#define MTFJSP_GIN_NODE_OUTPUT 2u
#define MTFJSP_GIN_PER_INSTANCE 4u
#define MTFJSP_GIN_OBS_F64 8u
#define MTFJSP_GIN_NO_SINGLE 16u
#define MTFJSP_GIN_REDUCE 32u
int32_t mtfjsp_gin_launches_for(int32_t batch, int32_t rows_per_instance, int32_t n_job, int32_t candidates, int32_t num_cu, int32_t product_mode,
                                uint32_t flags, char *buf, int32_t buf_len, int32_t *order_out, int32_t *pool_out);
int32_t mtfjsp_encoder_gin_launches(mtfjsp_encoder_t e, char *buf, int32_t buf_len, int32_t *order_out, int32_t *pool_out);
/* diagnostic (tests): what the handle's last single-launch GIN forward left, copied to host memory after synchronising the stream — the first `count`
 * floats of the candidate rows [B*J,128]; the 6 x 8 x 128 x 2 count-carrying statistics words of its six boundaries (csrc/mtfjsp_gin_resident.h,
 * gr_fix_encode); the (time-out, range) words.  Any of the three pointers may be NULL. */
int mtfjsp_encoder_peek_gin_res_host(mtfjsp_encoder_t e, float *cand_feat_host, int64_t count, uint64_t *stats_host, uint32_t *flags_host);
/* Which instantiation of the three-in-one heads launch (job heads + the machine path's GAT passes + machine heads: k_headsx_gat3x_headsx) serves a job
 * forward of the rollout — the library's one statement of the rule (csrc/mtfjsp_fused3_select.h; the heads launch's plan, csrc/mtfjsp_heads_select.h, goes through it).  No GPU involved.
 * batch instances of n_job candidates and n_machine machines (n_job * n_machine task rows) on num_cu compute units; obs_f64 != 0: f64 observations;
 * env_tail != 0: an armed environment step rides in the launch.  "k_headsx_gat3x_headsx<0, true, H3ShapeFixed<6, 6, 16>>" — the kernel text compiled for
 * J = 6, M = 6, 16 full instances per workgroup, f32 observations, node rows in LDS, no environment tail — serves exactly batch = 4096 of that shape;
 * "k_headsx_gat3x_headsx", the same text with the shape read at run time, everything else the launch is eligible for; NULL where it is not (the
 * separate launches run).  MTFJSP_FUSED3_GENERIC=1 (read per call, by the launches too) forces the run-time kernel; MTFJSP_FUSED3_NODES_HBM is
 * honoured as the handle honours it.  The handle's half of the eligibility (its switches, the census of co-resident workgroups) is not part of
 * the answer, and a forward whose arguments are not the rollout step's (no armed selection, no m_fea1 context ...) runs the run-time kernel.
 * *grid_out (may be NULL): workgroups.  mtfjsp_encoder_fused3_kernel_name: what the handle's last three-in-one launch ran (NULL: none yet). */
const char *mtfjsp_fused3_kernel_name_for(int32_t batch, int32_t n_job, int32_t n_machine, int32_t num_cu, int32_t obs_f64, int32_t env_tail, int32_t *grid_out);
const char *mtfjsp_encoder_fused3_kernel_name(mtfjsp_encoder_t e);
/* Which heads kernel serves an actor forward, with how many instances per workgroup and how many workgroups — the library's one statement of the rule
 * (csrc/mtfjsp_heads_select.h; both forwards launch from it).  No handle, no GPU.  batch instances of rows_per_instance scorer rows (n_job for the job
 * actor, n_machine for the machine actor), n_machine machines and task_rows task rows each on num_cu compute units.  flags: what the caller asks to ride
 * in the launch, and the handle's answers that are not the shape's —
 *   MTFJSP_HEADS_GAT          the machine path's GAT passes (a job forward with an armed m_fea1 context that has m_fea2)
 *   MTFJSP_HEADS_MHEADS       ... and the machine actor's heads (mtfjsp_encoder_arm_machine_heads with an armed machine selection)
 *   MTFJSP_HEADS_ENV_TAIL     an armed environment step that reads the last selection made in the launch
 *   MTFJSP_HEADS_VALUES_ONLY  the critic values alone (mtfjsp_encoder_arm_values_only)
 *   MTFJSP_HEADS_F32          product mode bit 4: the f32 matrix instruction
 *   MTFJSP_HEADS_NO_GAT       the handle cannot let the GAT passes ride (MTFJSP_NO_FUSED_GAT, per-instance BatchNorm, a statistics reduction, product
 *                             mode bits 2 | 4, no split weight images)
 *   MTFJSP_HEADS_NO_MHEADS    ... nor the machine heads (MTFJSP_NO_FUSED_MHEADS, no census of co-resident workgroups, no exchange words)
 *   MTFJSP_HEADS_OBS_F64      f64 observations
 * Precedence: "k_heads" with the f32 instruction (groups of 16, nothing rides); the three-in-one launch (the name mtfjsp_fused3_kernel_name_for gives:
 * GAT and machine heads asked for and allowed, shape eligible); "k_headsx_gat3x" (GAT asked for and allowed; whole groups of 16 in one round of
 * workgroups, a grid as wide as the GAT launch's own); "k_headsx_envstep"; "k_headsx_values"; "k_headsx10" (a full group has 7 to 10 tiles of 16 rows);
 * "k_headsx".  Groups of 8 instances only where nothing rides and 2 * ceil(batch / 16) <= num_cu.  MTFJSP_NO_HEADS_HG8, MTFJSP_NO_HEADS10,
 * MTFJSP_FUSED3_NODES_HBM and MTFJSP_FUSED3_GENERIC are read per call (a handle: csrc/mtfjsp_enc_switches.h).  *group_out / *grid_out
 * (may be NULL): instances per workgroup, workgroups.  NULL: a size below 1.
 * mtfjsp_encoder_heads_kernel_name: the kernel that computed the handle's last job (which = 0) / machine (which = 1) forward, with its group size and
 * grid — for a machine forward that the job forward's launch had already run, the three-in-one launch.  NULL: no such forward yet. */
#define MTFJSP_HEADS_GAT 1u
#define MTFJSP_HEADS_MHEADS 2u
#define MTFJSP_HEADS_ENV_TAIL 4u
#define MTFJSP_HEADS_VALUES_ONLY 8u
#define MTFJSP_HEADS_F32 16u
#define MTFJSP_HEADS_NO_GAT 32u
#define MTFJSP_HEADS_NO_MHEADS 64u
#define MTFJSP_HEADS_OBS_F64 128u
const char *mtfjsp_heads_kernel_name_for(int32_t batch, int32_t rows_per_instance, int32_t n_machine, int32_t task_rows, int32_t num_cu, uint32_t flags,
                                         int32_t *group_out, int32_t *grid_out);
const char *mtfjsp_encoder_heads_kernel_name(mtfjsp_encoder_t e, int32_t which, int32_t *group_out, int32_t *grid_out);
/* diagnostic (tests): the exchange words of the handle's last three-in-one launch, copied to host memory after synchronising the stream —
 * [2 sets: fine | wide][8 dispatch groups][256: sum | sum of squares of 128 columns] u64, arrival count in the top 6 bits — and the (time-out, range)
 * words.  Either pointer may be NULL. */
int mtfjsp_encoder_peek_fused3_host(mtfjsp_encoder_t e, uint64_t *words_host, uint32_t *flags_host);
/* number of statistics-exchange time-outs of the single-launch kernels reported on this handle so far */
int mtfjsp_encoder_resident_failures(mtfjsp_encoder_t e, int64_t *count_out);
int mtfjsp_encoder_timing_begin(mtfjsp_encoder_t e);
int mtfjsp_encoder_timing_end(mtfjsp_encoder_t e, double *ms_total, int64_t *launches);
/* per kernel family (between begin and the next begin): "gin0_agg_linear12" (or, round 6, "gin0_moments" / "gin0_stats_only" + "gin0_bn_gemm":
 * the first Linear's output formed by the second launch's producers instead of stored), "gin_gemm_bn_relu", "gin_gemm_agg",
 * "job_pool_gather", "heads", "head_gemm", "gat3", "mach_bn_pool", "sample", "small", "gin_inst", "gat_inst", "gin_resident" */
int mtfjsp_encoder_timing_query(mtfjsp_encoder_t e, const char *family, double *ms_total, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* MTFJSP_H */
