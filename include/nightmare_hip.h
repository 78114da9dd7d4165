/* nightmare_hip.h - C ABI of the MI355X-native NightmareV3Env.step() backend (libnightmare_hip.so).
 *
 * Drop-in boundary for the reference's env hot path. Every entry point names the reference interface it
 * replaces (file:line into the reference tree). Plain pointers and sizes only; device pointers are HIP device
 * memory on the env's device, `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All functions return 0 on success, nonzero on error (text via nm_last_error()). There is NO CPU path:
 * creation fails if no HIP device is usable.
 */
#ifndef NIGHTMARE_HIP_H
#define NIGHTMARE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_NUM_OBS 66      /* envs/nightmare_v3_config.py:11 */
#define NM_NUM_ACTIONS 18  /* envs/nightmare_v3_config.py:13 */
#define NM_NUM_REWARDS 16  /* reward names of envs/nightmare_v3_config.py:78-96 that have a _reward_ function (envs/nightmare_v3_env.py:399-497) */
#define NM_DTYPE_F32 0
#define NM_DTYPE_F64 1     /* verification build of the same kernels in double */

typedef struct nm_env nm_env;

/* The NightmareV3Config fields the step path reads (envs/nightmare_v3_config.py:4-100). Zero-initialised
 * fields are NOT defaults: start from nm_default_config(). Reward scales are the raw config values (before
 * the x dt of envs/nightmare_v3_env.py:128), order = nm_reward_name(i). */
typedef struct {
  int32_t decimation;               /* control.decimation :45 */
  double p_gain;                    /* control.p_gain :36 */
  double action_scale;              /* control.action_scale :46 */
  double default_pos[3];            /* control.default_pos (coxa, femur, tibia) :39-44 */
  double clip_actions;              /* normalization.clip_actions :74 */
  double clip_observations;         /* normalization.clip_observations :73 */
  double obs_lin_vel, obs_ang_vel, obs_dof_pos, obs_dof_vel; /* normalization.obs_scales :68-71 */
  double episode_length_s;          /* env.episode_length_s :14 */
  double resampling_time;           /* commands.resampling_time :60 */
  double max_lin_vel_x, max_ang_vel;/* commands.ranges :62,:64 */
  double termination_contact_force; /* env.termination_contact_force :22 */
  double tracking_sigma;            /* rewards.tracking_sigma :98 */
  double reward_scales[NM_NUM_REWARDS]; /* rewards.scales :78-95; 0 drops the term from the reward table (env.py:123-128) */
  int32_t tibia_contact_mode;       /* env.tibia_contact_mode :18  0 ignore, 1 penalise, 2 terminate (env.py:248-251,479-485) */
  double tibia_max_contact_force;   /* env.tibia_max_contact_force :19 */
  int32_t body_contact_mode;        /* env.body_contact_mode :20 */
  double body_max_contact_force;    /* env.body_max_contact_force :21 */
  double base_height_target;        /* rewards.base_height_target :99 */
  double max_contact_force;         /* rewards.max_contact_force :100 */
} nm_config;

void nm_default_config(nm_config* cfg);
/* "action_rate", "ang_vel_xy", "base_height", "body_contact_forces", "default_position", "dof_acc", "dof_vel", "feet_air_time",
 * "feet_contact_forces", "lin_vel_z", "orientation", "stand_still", "torques", "tracking_ang_vel", "tracking_lin_vel", "termination":
 * the order rewards are evaluated in (class_to_dict iterates dir(), envs/helpers.py:7; termination is added last,
 * envs/nightmare_v3_env.py:132-137, 285). The config names `collision` and `feet_stumble` (:95-96) have no function upstream. */
const char* nm_reward_name(int i);
const char* nm_last_error(void);

/* NightmareV3Env.__init__ (envs/nightmare_v3_env.py:27-140): model tables to the device, N env states at qpos0.
 * env_id_offset = global id of env 0 (multi-GPU sharding: counter-based RNG is keyed by the global id). */
int nm_create(const nm_config* cfg, int32_t num_envs, int32_t device, uint64_t seed, int64_t env_id_offset,
              int32_t dtype, nm_env** out);
int nm_destroy(nm_env* env);
int32_t nm_num_envs(const nm_env* env);
int32_t nm_dtype(const nm_env* env);

/* reset_idx(env_ids) (envs/nightmare_v3_env.py:335-371). ids: HOST int32 array, NULL = all envs.
 * ep_stats_dev [NM_NUM_REWARDS] f32 receives extras['episode'] (mean episode sums / episode_length_s);
 * episode_length_dev [N] i64 is the caller-owned episode_length_buf (envs/nightmare_v3_env.py:88). */
int nm_reset(nm_env* env, const int32_t* ids_host, int32_t n, int64_t* episode_length_dev, float* ep_stats_dev,
             void* stream);

/* step(actions) (envs/nightmare_v3_env.py:145-311) for all N envs, one launch.
 *   actions_dev        [N,18] f32 (read only)
 *   episode_length_dev [N] i64   in/out (episode_length_buf)
 *   obs_dev [N,66] f32, rew_dev [N] f32, done_dev [N] i64: the returned tuple (:311)
 *   time_outs_dev [N] f32, ep_stats_dev [NM_NUM_REWARDS] f32: extras; like the reference (:344-371) they are only
 *   refreshed by a step in which at least one env reset. A refresh of the buffer the previous refresh wrote is incremental (its
 *   ones are cleared, the new ones set), so the caller must not write into time_outs_dev between steps; a buffer at ANOTHER ADDRESS
 *   (a first call, a different allocation) is rewritten in full - decided on the device, also for launches replayed from a graph.
 *   Only the address is compared: a caller that frees the buffer and gets the same address back from its allocator, or overwrites the
 *   buffer's contents, must call nm_invalidate_time_outs() before the next step. */
int nm_step(nm_env* env, const float* actions_dev, int64_t* episode_length_dev, float* obs_dev, float* rew_dev,
            int64_t* done_dev, float* time_outs_dev, float* ep_stats_dev, void* stream);

/* Forget which time_outs buffer the last refresh wrote: the next refresh rewrites the whole buffer it is given (stream-ordered).
 * For callers that re-allocate or overwrite their extras['time_outs'] tensor (envs/nightmare_v3_env.py:369-371 builds a new one each time). */
int nm_invalidate_time_outs(nm_env* env, void* stream);

/* Physics only: action -> PD velocity command -> mj_step x decimation (envs/nightmare_v3_env.py:152-210),
 * no rewards/obs/reset (BASELINE config "dynamics+contact kernel only"). */
int nm_step_physics(nm_env* env, const float* actions_dev, void* stream);

/* The privileged critic row of an asymmetric actor-critic (no reference counterpart: upstream's critic sees the actor's observation,
 * envs/nightmare_v3_env.py:317-319): out_dev [N, NM_NUM_PRIVILEGED_OBS] float32 (device) =
 *   cols 0..65    obs_dev [N, 66], the observation the step wrote, copied bit for bit (its noise and clipping included)
 *   cols 66..88   NM_NUM_PRIVILEGED = 23 values of the env's own physics, read on the device from the per-env rows and the state:
 *     66     friction           mu
 *     67 68  gain ratios        p_gain / the config's p_gain, kv / the model's kv
 *     69     payload mass       base mass - the model's base mass (kg)
 *     70-72  payload com        base ipos - the model's base ipos (m, base body frame)
 *     73     latency steps      delay in substeps / decimation
 *     74-76  gravity            g / 9.81 (the frame of the floor)
 *     77     servo inv rate     1 / rate limit (+inf, no limit -> 0)
 *     78     servo d_gain
 *     79-81  inv torque limit   1 / limit of the coxa, femur, tibia servos (+inf -> 0)
 *     82-87  wrench             F[3] / (m g), tau[3] / (m g x 1 m), m the MODEL's total mass
 *     88     base height        qpos[2]
 *   An env whose rows were never set shows every kind's default: (mu, 1, 1, 0, 0 0 0, 0, 0 0 -1, 0, 0, 0 0 0, 0 x 6).
 * One launch of one small gather kernel (k_priv_obs) on `stream`, in stream order: called behind nm_step it shows the rows and the state AS
 * THAT STEP'S LAUNCHES LEFT THEM - the rows the NEXT step runs under: rows re-drawn at an in-step reset (nm_set_reset_rows), a wrench window
 * that opened or closed, the height after the reset. It reads, never writes, the env: not calling it is the feature off. The K-step
 * launches (nm_rollout, nm_play, nm_step_tape) do not produce the row. */
#define NM_NUM_PRIVILEGED 23
#define NM_NUM_PRIVILEGED_OBS (NM_NUM_OBS + NM_NUM_PRIVILEGED)
int nm_privileged_obs(nm_env* env, const float* obs_dev, float* out_dev, void* stream);

/* MjData state access (data[i].qpos / qvel / qacc_warmstart, envs/nightmare_v3_env.py:217-221,349-350).
 * HOST double arrays [N,25] [N,24] [N,24]; NULL entries are skipped. Synchronous. */
int nm_get_state(nm_env* env, double* qpos, double* qvel, double* qacc_warmstart);
int nm_set_state(nm_env* env, const double* qpos, const double* qvel, const double* qacc_warmstart);
/* The host-side buffers the reference keeps between steps (self.dof_pos, self.dof_vel, self.actions,
 * self.commands, self.episode_sums; envs/nightmare_v3_env.py:60-61,94-96,140). HOST doubles, NULL = skip.
 * episode_sums is [N,NM_NUM_REWARDS] in nm_reward_name order. */
int nm_get_buffers(nm_env* env, double* dof_pos, double* dof_vel, double* actions, double* commands, double* episode_sums);
int nm_set_buffers(nm_env* env, const double* dof_pos, const double* dof_vel, const double* actions,
                   const double* commands, const double* episode_sums);
/* State of _reward_feet_air_time (self.feet_air_time, self.last_contacts, self.last_contacts_filt; envs/nightmare_v3_env.py:90-93,
 * 447-477). HOST arrays: feet_air_time [N,6] double, last_contacts / last_contacts_filt [N,6] uint8. NULL = skip. Synchronous. */
int nm_get_feet_state(nm_env* env, double* feet_air_time, unsigned char* last_contacts, unsigned char* last_contacts_filt);
int nm_set_feet_state(nm_env* env, const double* feet_air_time, const unsigned char* last_contacts, const unsigned char* last_contacts_filt);
/* RNG-free command resampling for parity tests: HOST [N,4] uniforms in [0,1) used by the next steps instead
 * of the counter RNG ((x,yaw) for the periodic resample :235, (x,yaw) for the reset resample :356). NULL = RNG. */
int nm_set_command_uniforms(nm_env* env, const double* u_host);
/* counters: [0] contacts dropped (always 0 since every contact is kept: the matrix-free solver takes what the register-resident one cannot), [1] MuJoCo-style bad-state resets,
 * [2] support-vertex searches that fell back from the warm start to the exhaustive scan */
int nm_get_counters(nm_env* env, int64_t* out3);
/* optional debug dump [N,256] reals (dtype of the env) written by nm_step; NULL disables */
int nm_set_debug_buffer(nm_env* env, void* dbg_dev);
/* Running return kept by the step kernel itself: with a DEVICE float [N] buffer set, every nm_step adds the step's reward
 * (envs/nightmare_v3_env.py:277-288, what step() returns as reward_buffer) to acc[env] - the caller's
 * `cur_reward_sum += rewards` (rsl_rl OnPolicyRunner.learn, the loop train.py:54 drives) without a second launch per step.
 * The caller owns, zeroes and reads the buffer (stream-ordered with nm_step); NULL switches it off (the default). Not touched
 * by nm_step_physics. */
int nm_set_return_accumulator(nm_env* env, float* acc_dev);

/* Observation noise (envs/nightmare_v3_env.py:109-119 builds noise_scale_vec, :304-305 applies it): with a HOST [66] vector
 * set, every nm_step adds (2u-1)*noise_scale_vec[k] to observation k before the clip, u ~ U[0,1) from the counter RNG
 * keyed by (seed, global env id, step, k). NULL switches it off (the default, config add_noise=False :49). */
int nm_set_observation_noise(nm_env* env, const double* noise_scale_vec_host);
/* RNG-free noise for parity tests: HOST [N,66] uniforms used by the following steps instead of the counter RNG
 * (what np.random.rand(N,66) returned at :305). NULL = RNG. */
int nm_set_noise_uniforms(nm_env* env, const double* u_host);
/* Push perturbations - the `domain_rand.push_robots` / `push_interval_s` / `max_push_vel_xy` of legged_gym-shaped config trees, the other
 * half of SURVEY 8(f) row 4 next to the observation noise above; the reference has no such line. Every `interval_steps` env steps the
 * base's world-frame linear velocity qvel[env, 0:2] of every env is SET to (vx, vy), each uniform in [-max_vel_xy, +max_vel_xy), before
 * the physics of that step; nothing else of the state changes. It works alike in nm_step, nm_rollout, nm_play and nm_step_tape.
 * The env counts its full env steps in a push step index s (K per K-step launch; nm_step_physics and nm_reset leave it alone): step s is
 * pushed iff interval_steps > 0 && s > 0 && s % interval_steps == 0, with v = (2u - 1) * max_vel_xy in the env's precision (fp32: max
 * rounded to float first), u ~ U[0,1) from the counter RNG keyed by (seed + "PUSH", global env id, 2 * (s / interval_steps) + axis).
 * The observation the PREVIOUS step returned does not show the push.
 * interval_steps == 0 switches pushes off (the default); a negative interval or a negative / non-finite max_vel_xy is refused. The call
 * sets s = start_step. nm_get_push returns the setting and the current s (any pointer may be NULL): a checkpoint's three numbers. */
int nm_set_push(nm_env* env, int32_t interval_steps, double max_vel_xy, uint64_t start_step);
int nm_get_push(nm_env* env, int32_t* interval_steps, double* max_vel_xy, uint64_t* step);
/* Randomised reset states - the `_reset_dofs` / `_reset_root_states` of legged_gym-shaped stacks, which draw the joint angles and the root
 * velocity afresh at every reset; the reference has no such line (its reset_idx writes qpos0 and zero velocity, env.py:335-371).
 * ranges10_host: five ranges (lo, hi) in the order base_height, dof_pos, base_lin_vel, base_ang_vel, dof_vel. While the feature is on, an
 * env's reset - time-out, termination or nm_reset - writes qpos0 and zero velocity as before and then overwrites 43 words of that env:
 *   column 0       qpos[2]       = qpos0[2] + d(0)           (base_height)
 *   columns 1..18  qpos[7 + j]   = qpos0[7 + j] + d(1 + j)   (dof_pos)
 *   columns 19..21 qvel[0:3]     = d(c)                      (base_lin_vel, world frame)
 *   columns 22..24 qvel[3:6]     = d(c)                      (base_ang_vel)
 *   columns 25..42 qvel[6 + j]   = d(c)                      (dof_vel)
 * qpos[0:2] and the base quaternion keep their qpos0 values. d(c) = lo_r + u * w_r in the env's precision `real`, with lo_r = real(lo),
 * w_r = real(hi) - real(lo), u = rand_u24_bits(seed + "RESET", global env id, 64 k + c) * 2^-24, product and sum rounded separately (the
 * rules of nm_draw_env_params), the counter in 32 bits. k is the env's reset count: read by all 43 columns, then incremented by one.
 * A reset draw is an edit of the state between two steps and nothing else: qacc_warmstart, the stale dof_pos / dof_vel / cvel buffers, the
 * command resample, the command RNG counter and the feet state stay as they are; the resetting step returns the terminal observation, as
 * upstream; the bad-state reset inside the physics still goes to qpos0; nm_step_physics never resets. It works alike in nm_step, nm_reset
 * (distinct ids), nm_rollout, nm_play and nm_step_tape, and the state after any step of any path equals the per-step path's.
 * Off is the default, and "on with ten zeros" equals off bit for bit (+0 offsets).
 * nm_set_reset_noise: ranges10_host NULL switches the feature off. counts_host: HOST [N] reset counts to install, or NULL to keep the
 * env's (zeros at first use). Refused: a NULL env, non-finite values (in fp32: after rounding to float), lo > hi.
 * nm_get_reset_noise: the flag, the ranges in force (zeros while off) and the reset counts (HOST [N]); any pointer may be NULL. A
 * checkpoint's content.
 * nm_reset_noise_offsets: d(0..42) of reset k of the env with global id `global_env` as doubles, computed on the host by the function the
 * kernels call; no env, no device. dtype: NM_DTYPE_F32 or NM_DTYPE_F64. */
int nm_set_reset_noise(nm_env* env, const double* ranges10_host, const uint32_t* counts_host);
int nm_get_reset_noise(nm_env* env, int32_t* on, double* ranges10, uint32_t* counts_host);
int nm_reset_noise_offsets(const double* ranges10, uint64_t seed, int64_t global_env, uint32_t k, int32_t dtype, double* out43);
/* Per-env friction and servo-gain randomisation - the `domain_rand.randomize_friction` / `friction_range` of legged_gym-shaped config
 * trees and the stiffness / damping multipliers their forks add; it replaces nothing upstream (the reference has one floor and one servo).
 * Each env e carries three values in the env's dtype:
 *   mu[e]      sliding friction of every contact of the env (pyramid rows n +- mu t, diagApprox = tran + mu^2 tran, R = 2 mu^2 R0):
 *              what setting the friction of every geom of that env's model would give;
 *   p_gain[e]  in place of control.p_gain in ctrl = ((a - default_pos) - dof_pos) * p_gain (envs/nightmare_v3_env.py:183);
 *   kv[e]      in place of the actuators' kv = 0.8: the force kv (clamp(ctrl) - qvel) and the implicitfast matrix M + h kv I.
 * They hold until the caller changes them: no reset resamples them. It works alike in nm_step, nm_step_physics, nm_rollout, nm_play and
 * nm_step_tape. Off is the default, and off equals "on with (1.0, cfg.p_gain, 0.8) in every env" bit for bit.
 * nm_set_env_params: DEVICE arrays [N] in the env's dtype, copied on `stream`; a NULL array sets that column to its default; all three
 *   NULL switch the feature off (nothing is freed). The values are NOT validated: mu <= 1e-5, a negative gain or a non-finite value is the
 *   caller's responsibility (the physics then divides by zero or diverges, and the bad-state resets of mj_check* take over).
 * nm_get_env_params: the three columns into DEVICE arrays [N] (any may be NULL) on `stream`; the defaults while the feature is off.
 * nm_draw_env_params: value = lo[c] + u (hi[c] - lo[c]) for column c = 0 (mu), 1 (p_gain), 2 (kv) in the env's precision, product and sum
 *   rounded separately, u ~ U[0,1) from the counter RNG keyed by (seed + "ENVP", global env id, c): sharding changes nothing; lo == hi
 *   pins a column. Refused before any device call, named by nm_last_error: non-finite bounds, lo > hi, mu <= 1e-5, negative p_gain / kv. */
int nm_set_env_params(nm_env* env, const void* mu_dev, const void* p_gain_dev, const void* kv_dev, void* stream);
int nm_get_env_params(nm_env* env, void* mu_dev, void* p_gain_dev, void* kv_dev, void* stream);
int nm_draw_env_params(nm_env* env, const double lo[3], const double hi[3], void* stream);
/* Per-env base payload - the `domain_rand.randomize_base_mass` / `added_mass_range` and `randomize_com_displacement` of legged_gym-shaped
 * config trees. There is no reference line: upstream shares one MjModel among all envs and has no payload.
 * Semantics: a payload is a point mass dm (kg, may be negative) rigidly attached to the base body at r (m, base body frame). An env with
 * payload (dm, r) behaves as if mjmodel.xml had been recompiled with that mass added to base_link: NOTHING stays stale. Per env change
 *   the base body: m' = m + dm, ipos' = (m ipos + dm r) / m', I' = I + m P(ipos - ipos') + dm P(r - ipos'), P(d) = (d.d) 1 - d d'
 *     (body frame, about the new COM);
 *   total_mass (subtree COM, cvel of the base);
 *   body_invweight0[b][0] of the 7 colliding bodies (base and six tibias: the base floats, so the tibias' values move too);
 *   pgs_scale = 1 / (meaninertia' nv), the scale of the six PGS / NoSlip exit tests.
 * Link bodies, hull tables, rbound, qpos0, the reset pose and every config value do not change. A row (20 words in the env's dtype) is
 *   ipos[3], I[6] (xx yy zz xy xz yz), mass, total_mass, invweight0[7] (base, tibia 1..6), pgs_scale, pad
 * and is derived on the host (nightmare_rl_amd/model/payload.py payload_rows). Rows hold until the caller changes them; no reset touches
 * them. It works alike in nm_step, nm_step_physics, nm_rollout, nm_play and nm_step_tape, alone or with nm_set_env_params. Off is the
 * default, and off equals "on with the default row in every env" bit for bit.
 * nm_set_body_params: `rows` is a DEVICE array [N,20] in the env's dtype, copied on `stream`; NULL switches the feature off (nothing is
 *   freed). Refused, named by nm_last_error, before anything of the env changes (the rows are read back and judged on the host, which
 *   waits for `stream`): a non-finite word, mass <= 0, total_mass < mass, a non-positive inertia diagonal, invweight0 or pgs_scale.
 * nm_get_body_params: the rows into a DEVICE array [N,20] on `stream`; the model's own row for every env while the feature is off.
 * nm_draw_payload: out[e] = (dm, rx, ry, rz), value = lo[c] + u (hi[c] - lo[c]) in the env's precision, product and sum rounded
 *   separately, u ~ U[0,1) from the counter RNG keyed by (seed + "PAYLO", global env id, c): sharding changes nothing; lo == hi pins a
 *   column. `out` is a DEVICE array [N,4]; the env itself is not changed (derive rows from the draw, then nm_set_body_params). Refused
 *   before any device call: non-finite bounds, lo > hi. */
int nm_set_body_params(nm_env* env, const void* rows_dev, void* stream);
int nm_get_body_params(nm_env* env, void* out_dev, void* stream);
int nm_draw_payload(nm_env* env, const double lo[4], const double hi[4], void* out_dev, void* stream);
/* Per-env actuation latency: the servo targets of an env lag the policy's actions by d physics substeps. There is no reference line:
 * upstream applies every action in the tick it was computed; the real robot's serial servo bus does not.
 * Semantics: a_t is step t's action after scale and clip (float32). Each env has an integer delay d, 0 <= d <= H nsub, H = 3 past
 * actions kept, nsub = decimation (6 substeps = 48 ms at the defaults). With k = d / nsub, r = d % nsub, substep s of step t aims the
 * servos at a_{t-k-1} while s < r and at a_{t-k} from s = r on; either command is ((real(a) - default) - dof_pos buffer) p_gain, today's
 * expression on the step-start dof_pos snapshot and the env's own p_gain, computed from its own action (a delayed env's command has the
 * bits an undelayed env would give the same action). Everything else - observation slots 48..65, action_rate, default_position, the
 * actions buffer, the transition and state-log records - keeps a_t: the policy meets latency through the physics alone.
 * History: hist[e][j] = a_{t-1-j}, j = 0..H-1, float32, zero at construction. Every full step taken WHILE THE FEATURE IS ON shifts it
 * and puts a_t in front; steps taken while it is off leave it alone, and so do resets (upstream's reset_idx keeps self.actions),
 * physics-only launches (which ignore latency altogether) and switching the feature on or off. The MuJoCo bad-state path (ctrl = 0
 * for the rest of that substep) is unchanged. It works alike in nm_step, nm_rollout, nm_play and nm_step_tape, alone or with
 * nm_set_env_params / nm_set_body_params. Off is the default, and off equals "on with delay 0 in every env" bit for bit.
 * nm_set_action_latency: `substeps` is a DEVICE array [N] int32, copied on `stream`; NULL switches the feature off (nothing is freed).
 *   Refused, named by nm_last_error, before anything of the env changes (the delays are read back and judged on the host, which waits
 *   for `stream`): a delay outside [0, H nsub].
 * nm_get_action_latency: the delays into a DEVICE array [N] int32 on `stream`; zeros while the feature is off.
 * nm_draw_action_latency: delay[e] uniform on the integers [lo, hi], lo + floor(u (hi - lo + 1)) with u = bits 2^-24, bits from the
 *   counter RNG keyed by (seed + "LATEN", global env id, 0) - in integers lo + ((bits (hi - lo + 1)) >> 24): sharding changes nothing;
 *   switches the feature on. Refused before the handle is looked at: lo < 0, lo > hi; with the handle: hi > H nsub.
 * nm_set_action_history / nm_get_action_history: DEVICE arrays [N,H,18] float32 in the logical order above (row 0 the latest). */
int nm_set_action_latency(nm_env* env, const int32_t* substeps_dev, void* stream);
int nm_get_action_latency(nm_env* env, int32_t* out_dev, void* stream);
int nm_draw_action_latency(nm_env* env, int32_t lo, int32_t hi, void* stream);
int nm_set_action_history(nm_env* env, const float* hist_dev, void* stream);
int nm_get_action_history(nm_env* env, float* out_dev, void* stream);
/* Per-env gravity vectors: slopes and the `domain_rand.randomize_gravity` / `gravity_range` of legged_gym-shaped config trees. There is no
 * reference line for the physics: upstream has one level floor under (0, 0, -9.81). For an infinite plane a floor inclined by theta is
 * exactly a level floor under a gravity vector tilted by theta, written in the floor's frame: the env's x, y are then the floor's own
 * axes and z its normal. One plane per env; there is no terrain mesh.
 * Each env carries two 3-vectors in the env's dtype, one row of 8 words: g[3], pad, gravity_vec[3], pad.
 *   g            the gravity the physics sees (m/s^2, frame of the floor). It replaces the model's gravity everywhere the physics uses it:
 *                the base's bias acceleration (all three components), and the MuJoCo bad-state path, whose free-fall step from qpos0
 *                becomes qvel[0:3] = g h, qpos[0:3] += g h^2, qacc_warmstart[0:3] = g. Nothing else of the model changes.
 *   gravity_vec  the vector the env layer rotates into the body frame (envs/nightmare_v3_env.py:46, :219): observation slots 6..8, the
 *                `orientation` reward and the 60 degree termination. A caller who wants an IMU's view sets it equal to g (on a slope the
 *                policy then sees the tilt); a caller who keeps upstream's constant (0, 0, -9.81) has upstream's env layer line for line
 *                while only the physics tilts.
 * Rows hold until the caller changes them; no reset touches them. It works alike in nm_step, nm_step_physics, nm_rollout, nm_play and
 * nm_step_tape, alone or with any other per-env kind (a physics-only launch still ignores latency). Off is the default, and off equals
 * "on with (0, 0, -9.81) twice in every env" under == in every output (the additions are t + (-g): exact zeros change no rounding; a
 * zero may differ from today's in sign only).
 * nm_set_gravity: `rows` is a DEVICE array [N,8] in the env's dtype, copied on `stream`; NULL switches the feature off (nothing is
 *   freed). Refused, named by nm_last_error, before anything of the env changes (the rows are read back and judged on the host, which
 *   waits for `stream`): a non-finite word, a zero gravity_vec (the termination divides by its norm). A zero g is admitted: free float.
 * nm_get_gravity: the rows into a DEVICE array [N,8] on `stream`; (0, 0, -9.81) twice for every env while the feature is off. A
 *   checkpoint's content.
 * nm_draw_gravity: out[e] = (offset x, y, z in m/s^2, tilt theta, azimuth phi in rad), value = lo[c] + u (hi[c] - lo[c]) in the env's
 *   precision, product and sum rounded separately, u ~ U[0,1) from the counter RNG keyed by (seed + "GRAV", global env id, c): sharding
 *   changes nothing; lo == hi pins a column. `out` is a DEVICE array [N,5]; the env itself is not changed (derive rows from the draw -
 *   g = 9.81 (sin theta cos phi, sin theta sin phi, -cos theta) + offset, on the host in float64 - then nm_set_gravity). Refused before
 *   any device call: non-finite bounds, lo > hi. */
int nm_set_gravity(nm_env* env, const void* rows_dev, void* stream);
int nm_get_gravity(nm_env* env, void* out_dev, void* stream);
int nm_draw_gravity(nm_env* env, const double lo[5], const double hi[5], void* out_dev, void* stream);
/* Servo target model: a per-env slew-rate limit on the servo target and a damping term. It replaces what upstream keeps commented out:
 * `limited_actions` (envs/nightmare_v3_env.py:97), the limiter line and the damping term (envs/nightmare_v3_env.py:187-188), and
 * `d_gain = 0.05` / `action_rate_limit = 0.08` (envs/nightmare_v3_config.py:37-38).
 * Each env carries one row of 4 words in the env's dtype: rate, d_gain, pad, pad. rate > 0 is the most the servo target may move per
 * control step (rad; +inf = no limit), d_gain >= 0. Each env also carries the state L[18] in the env's dtype, upstream's limited_actions,
 * zero at construction.
 * Semantics: T = real(a) - default_pos, a the float32 action this step brings to the servo: a_t, or with nm_set_action_latency the late
 * action a_{t-k} (the limiter sits behind the delay line; the action history keeps raw a_t). Once per full step
 *   d = T - L;   L' = |d| <= rate ? T : L + copysign(rate, d)
 * (upstream's limited += clip(d, -rate, rate) up to rounding; a select, so rate = +inf gives L' = T bit for bit), and
 *   ctrl = (L_used - dof_pos buffer) p_gain - d_gain dof_vel buffer
 * on the step-start snapshots of both buffers and the env's own p_gain. Substeps before the latency switch substep r use L (the state
 * before the update), substeps from r on use L'; without latency r = 0 and every substep uses L'. Each command is computed from its own
 * target. The physics clips to the +-8 ctrlrange as before. Everything else - observation slots 48..65, action_rate, default_position,
 * the actions buffer, the transition and state-log records - keeps a_t: the policy meets the servo through the physics alone.
 * L is state: every full step taken WHILE THE FEATURE IS ON updates it (the zero-action step of a reset sequence included); steps taken
 * while it is off, resets (upstream's reset_idx touches neither actions nor limited_actions), physics-only launches (which ignore the
 * whole servo row, as they ignore latency) and switching the feature on or off leave it alone. The MuJoCo bad-state path (ctrl = 0 for
 * the rest of that substep) is unchanged. It works alike in nm_step, nm_rollout, nm_play and nm_step_tape, alone or with any other
 * per-env kind. Off is the default, and off equals "on with (+inf, 0) in every env" under == in every output for a finite dof_vel buffer
 * (the damping term is then an exact zero; a zero command may differ from today's in sign only). A non-finite dof_vel buffer makes the
 * command NaN while the feature is on, even at d_gain = 0 (0 x inf); the physics meets it in its bad-state check like any bad control.
 * nm_set_servo: `rows` is a DEVICE array [N,4] in the env's dtype, copied on `stream`; NULL switches the feature off (nothing is freed).
 *   Refused, named by nm_last_error, before anything of the env changes (the rows are read back and judged on the host, which waits for
 *   `stream`): rate not > 0 (NaN included; +inf is admitted), d_gain not finite or < 0.
 * nm_get_servo: the rows into a DEVICE array [N,4] on `stream`; (+inf, 0, 0, 0) for every env while the feature is off.
 * nm_draw_servo: row[e] = (rate, d_gain, 0, 0), value = lo[c] + u (hi[c] - lo[c]) in the env's precision, product and sum rounded
 *   separately, u ~ U[0,1) from the counter RNG keyed by (seed + "SERVO", global env id, c): sharding changes nothing; lo == hi pins a
 *   column; switches the feature on. Refused before any device call: non-finite bounds, lo > hi, rate lo <= 0, d_gain lo < 0.
 * nm_get_servo_state / nm_set_servo_state: L as HOST doubles [N,18], in the style of nm_get_buffers (synchronous; zeros before the first
 *   use of any per-env kind). */
int nm_set_servo(nm_env* env, const void* rows_dev, void* stream);
int nm_get_servo(nm_env* env, void* out_dev, void* stream);
int nm_draw_servo(nm_env* env, const double lo[2], const double hi[2], void* stream);
int nm_get_servo_state(nm_env* env, double* limited);
int nm_set_servo_state(nm_env* env, const double* limited);
/* Servo torque limit: MuJoCo 3.1.2's actuator `forcerange`, per env. The reference's servos are ideal (no forcerange in mjmodel.xml);
 * the semantics are stated from the upstream source of mj_fwdActuation and mjd_actuator_vel.
 * Each env carries one row of 4 words in the env's dtype: fmax_coxa, fmax_femur, fmax_tibia, pad. Word k limits joint 3 leg + k of all
 * six legs; each value > 0, +inf = no limit; the range is symmetric, [-fmax, +fmax].
 * Force (mj_fwdActuation), in every forward pass of every substep, with the env's own kv (nm_set_env_params):
 *   f = kv clip(ctrl, +-8) - kv qvel;   qfrc_actuator = f > fmax ? fmax : (f < -fmax ? -fmax : f)
 * (compares and selects: a NaN force stays NaN and meets the bad-state check as it does without a limit).
 * Implicit factor (mjd_actuator_vel inside mj_implicit, implicitfast): an actuator whose force sits on its bound contributes no velocity
 * derivative, so the step's second factor is that of M + h kv D, D = diag(d_j), d_j = 1 where |f_j| < fmax_j and 0 otherwise (the 6 base
 * dofs 0 as before), decided on the same f as the clamp, in the same forward pass.
 * It is physics, like friction, kv, payload and gravity: nm_step, nm_step_physics, nm_rollout, nm_play and nm_step_tape honour it alike,
 * alone or with any other per-env kind; resets, pushes, latency and the servo target model meet it through the ctrl they produce alone.
 * No observation slot, reward term, record or state-log field changes. Off is the default, and off equals "on with (+inf, +inf, +inf)
 * in every env" under == in every output.
 * nm_set_torque_limit (mj_fwdActuation's clamp, mjd_actuator_vel's mask): `rows` is a DEVICE array [N,4] in the env's dtype, copied on
 *   `stream`; NULL switches the feature off (nothing is freed). Refused, named by nm_last_error, before anything of the env changes (the
 *   rows are read back and judged on the host, which waits for `stream`): a limit that is not > 0 (NaN included; +inf is admitted).
 * nm_get_torque_limit (the forcerange the stages read): the rows into a DEVICE array [N,4] on `stream`; (+inf, +inf, +inf, 0) for every
 *   env while the feature is off.
 * nm_draw_torque_limit (forcerange randomisation): row[e] = (f0, f1, f2, 0), f_c = lo[c] + u (hi[c] - lo[c]) in the env's precision,
 *   product and sum rounded separately, u ~ U[0,1) from the counter RNG keyed by (seed + "TORQUE", global env id, c) - three independent
 *   draws per env; sharding changes nothing; lo == hi pins a column; switches the feature on. Refused before any device call: non-finite
 *   bounds, lo > hi, lo <= 0. */
int nm_set_torque_limit(nm_env* env, const void* rows_dev, void* stream);
int nm_get_torque_limit(nm_env* env, void* out_dev, void* stream);
int nm_draw_torque_limit(nm_env* env, const double lo[3], const double hi[3], void* stream);
/* External wrench on the base: MuJoCo 3.1.2's `xfrc_applied` on the base body, per env - the "external force / torque on the base" of
 * legged_gym-shaped trainers. The reference applies none; the semantics are stated from the upstream source of mj_fwdAcceleration /
 * mj_xfrcAccumulate (mj_applyFT on the body's xipos).
 * Each env carries one row of 8 words in the env's dtype: F[3] (N), pad, tau[3] (N m), pad - both in the world frame (the floor's frame
 * when gravity rows tilt it), F applied at the base body's centre of mass xipos. In every forward pass of every substep the wrench enters
 * qfrc_smooth as J'[F; tau] and nowhere else; for the free joint (translations in the world frame, rotations about the body axes)
 *   qfrc_smooth[0:3] += F;   qfrc_smooth[3:6] += Rb' tau + ipos x (Rb' F)
 * with Rb the base's rotation and ipos its COM offset in its own frame (the env's own body row while a payload is set). It has no velocity
 * derivative: the implicit factor M + h kv D does not change. Unlike a push it goes through the contact solver. The bad-state step
 * (mj_resetData inside mj_step) applies none, as upstream clears xfrc_applied there. It is physics: nm_step, nm_step_physics, nm_rollout,
 * nm_play and nm_step_tape honour it alike, alone or with any other per-env kind. No observation slot, reward term (the `torques` reward
 * reads the joint part, which stays zero), record or state-log field changes; no reset touches the rows, and the rows re-drawn at reset
 * (nm_set_reset_rows) do not include this kind. Off is the default, and off equals "on with zero rows" under == in every output.
 * nm_set_base_wrench (xfrc_applied, constant until set again): `rows` is a DEVICE array [N,8] in the env's dtype, copied on `stream`;
 *   NULL switches the feature off, ends a schedule and refills zero rows (nothing is freed). Refused, named by nm_last_error, before
 *   anything of the env changes (the rows are read back and judged on the host, which waits for `stream`): a non-finite force or torque;
 *   rows while a schedule is on.
 * nm_get_base_wrench (the rows the stages read): into a DEVICE array [N,8] on `stream`; zero for every env while the feature is off.
 * nm_set_wrench_schedule (random wrenches over time windows): switches the feature on and lets the env write its own rows. The env counts
 *   its full env steps in a wrench step index s (K per K-step launch; nm_step_physics and nm_reset leave it alone), and the call sets
 *   s = start_step. With 1 <= duration_steps <= interval_steps, at the start of step s every env's row is
 *     a fresh draw   if s >= interval_steps && s % interval_steps == 0          (window q = s / interval_steps)
 *     set to zero    if s >= interval_steps && s % interval_steps == duration_steps   (only when duration_steps < interval_steps)
 *     unchanged      otherwise,
 *   the draw per axis (0..2 = F, 3..5 = tau) v = (2u - 1) * max[axis] in the env's precision (fp32: max rounded to float first),
 *   u ~ U[0,1) from the counter RNG keyed by (seed + "WRENCH", global env id, 6 q + axis): sharding changes nothing. The call installs
 *   the rows that hold once step start_step has begun - the draw of window start_step / interval_steps if start_step lies inside a window,
 *   zero otherwise - so a checkpoint's numbers continue a run exactly. interval_steps == 0 switches the schedule off and the rows to zero
 *   (the feature stays as it is; the maxima may be NULL). Synchronous. Refused before the handle is looked at: a negative or non-finite
 *   maximum, duration_steps < 1 or > interval_steps, a negative interval or one of 2^31 steps or more.
 * nm_get_wrench_schedule: the setting and the current s (any pointer may be NULL): a checkpoint's numbers. */
int nm_set_base_wrench(nm_env* env, const void* rows_dev, void* stream);
int nm_get_base_wrench(nm_env* env, void* out_dev, void* stream);
int nm_set_wrench_schedule(nm_env* env, int64_t interval_steps, int64_t duration_steps, const double max_force[3], const double max_torque[3],
                           uint64_t start_step);
int nm_get_wrench_schedule(nm_env* env, int64_t* interval_steps, int64_t* duration_steps, double max_force[3], double max_torque[3], uint64_t* step);
/* Per-env sensor model: observation latency and bias. There is no reference line: upstream's policy reads the exact state of the current
 * step (envs/nightmare_v3_env.py:274-305) plus optional white noise; a real robot's IMU / state estimator and servo feedback arrive one
 * to three control periods late and carry offsets that stay constant over an episode. The model is a pure function of the observation
 * rows the step already files and sits between the step and whoever reads the observation; the physics and the rewards do not see it.
 * Columns 0..8 (base lin vel, base ang vel, projected gravity) form the group `imu`, columns 12..47 (dof_pos, dof_vel) the group `joint`;
 * columns 9..11 (commands) and 48..65 (previous actions) are passed through bit for bit, never delayed or biased.
 * Each env carries two delays d_imu, d_joint in 0..3 whole env steps, a float32 bias row b[66] in observation units (already multiplied
 * by the obs scale; zero in the pass-through columns), a history of its last 4 true observations and a count n of the observations pushed
 * since the history was last cleared.
 * Semantics: y_s is the observation the step produces at step s, after its own noise and its own clip - the "true" observation. After
 * every full step, for every env: (1) push y_s, n <- n + 1; (2) a column c of group g reads
 *   sensed[c] = clamp(y_{s - min(d_g, n - 1)}[c] + b[c], -clip_obs, +clip_obs)   (one float32 add, the step's float32 clip_obs)
 * and a pass-through column sensed[c] = y_s[c]; (3) if the step's done flag is set, n <- 0 - after the read: the done step's own reading
 * is delayed like any other, and the next step sees only itself. nm_reset clears n for the ids it resets; nm_create, nm_set_sensor and
 * nm_draw_sensor clear it for all envs: a reading never reaches behind a clear. The model is float32 whatever the env's dtype.
 * While the model is on, the sensed row is what nm_step, nm_rollout, nm_rollout_priv, nm_play and nm_step_tape file wherever they filed
 * the observation before (the caller's buffer, the rollout storage, the observation record, the first 66 columns of the privileged row
 * the asymmetric launch gathers - call nm_privileged_obs on the sensed row); the policy inside the K-step launches reads it; the true row
 * of the last step stays in the env (nm_get_true_obs). Physics-only launches do not touch the model. Off is the default, and delays 0
 * with bias 0 equal off under == in every output.
 * nm_set_sensor: delays_dev is a DEVICE array [N,2] int32 (d_imu, d_joint) or NULL (= zeros), bias_dev a DEVICE array [N,66] float32 or
 *   NULL (= zeros), copied on `stream`; both NULL switch the model off (nothing is freed). It clears the history. Refused, named by
 *   nm_last_error with the env and the column, before anything of the env changes (the arrays are read back and judged on the host, which
 *   waits for `stream`): a delay outside 0..3, a non-finite bias, a non-zero bias in a pass-through column.
 * nm_get_sensor: *on, and the delays / the bias into DEVICE arrays [N,2] int32 / [N,66] float32 on `stream` (any pointer may be NULL);
 *   zeros while the model is off.
 * nm_draw_sensor: delay[e][g] uniform on the integers [lo[g], hi[g]], lo + ((bits (hi - lo + 1)) >> 24); bias[e][c] = (2 u - 1)
 *   float32(bias_max[k]) for a column of kind k (0 lin_vel, 1 ang_vel, 2 gravity, 3 dof_pos, 4 dof_vel; maxima in observation units),
 *   u = bits 2^-24 in float32, zero in the pass-through columns; bits from the counter RNG keyed by (seed + "SENSO", global env id, word),
 *   word = the column for a bias and 66 + g for a delay: sharding changes nothing. It switches the model on and clears the history.
 *   Refused before the handle is looked at: lo < 0, lo > hi, hi > 3, a negative or non-finite maximum.
 * nm_sensor_draw_values: the draw of the env with global id `global_env`, computed on the host by the function the kernel calls; no env,
 *   no device.
 * nm_get_sensor_state / nm_set_sensor_state: the history as HOST arrays, ring [N,4,66] float32 (slot n mod 4 takes the push of an env
 *   whose count is n) and count [N] uint32, in the style of nm_get_servo_state (synchronous; zeros before the first use of the model).
 * nm_get_true_obs: the true observation of the last step into a DEVICE array [N,66] float32 on `stream`; refused while the model is off
 *   (the observation the step returned is then the true one). */
int nm_set_sensor(nm_env* env, const int32_t* delays_dev, const float* bias_dev, void* stream);
int nm_get_sensor(nm_env* env, int32_t* on, int32_t* delays_out_dev, float* bias_out_dev, void* stream);
int nm_draw_sensor(nm_env* env, const int32_t lo[2], const int32_t hi[2], const double bias_max[5], void* stream);
int nm_sensor_draw_values(uint64_t seed, int64_t global_env, const int32_t lo[2], const int32_t hi[2], const double bias_max[5], int32_t out_delays[2],
                          float out_bias[NM_NUM_OBS]);
int nm_get_sensor_state(nm_env* env, float* ring, uint32_t* count);
int nm_set_sensor_state(nm_env* env, const float* ring, const uint32_t* count);
int nm_get_true_obs(nm_env* env, float* out_dev, void* stream);
/* Per-env rows re-drawn at every reset, from pools - the `mode="reset"` events of Isaac Lab, legged_gym's per-reset payload; it replaces
 * nothing upstream (the reference has one robot, one floor and ideal servos, and its reset_idx touches no model constant).
 * kind: 0 friction / gains [4] (mu, p_gain, kv, pad), 1 body rows [20], 2 actuation latency [1] (a 4-byte int in either dtype), 3 gravity
 * rows [8], 4 servo rows [4], 5 torque-limit rows [4]: the rows of nm_set_env_params, nm_set_body_params, nm_set_action_latency,
 * nm_set_gravity, nm_set_servo and nm_set_torque_limit, 41 words in all. Each kind may own a pool of P such rows, 1 <= P <= 65536, in the
 * env's dtype. While a kind has a pool, an env's reset - time-out, termination or nm_reset; not the bad-state reset inside the physics,
 * and nm_step_physics never resets - overwrites that kind's row of that env with pool row
 *   i = (rand_u24_bits(seed + "RESAMP", global env id, 8 k + kind) * P) >> 24        (64-bit integers, the counter in 32 bits)
 * k is the env's reset-row count, a buffer of its own (not the reset count of nm_set_reset_noise), read for all six kinds and then
 * incremented by one. A pool has no arithmetic: fp32 and fp64, host and device agree bit for bit, and correlated parameters are
 * expressible. The new rows hold from the first step of the new episode; the resetting step ran on the old rows and returns the terminal
 * observation, as before. The action history and the servo's limited targets are state and keep what they hold. It works alike in
 * nm_step, nm_reset (distinct ids), nm_rollout, nm_play and nm_step_tape, and the state after any step of any path equals the per-step
 * path's. The key is the global env id: sharding changes nothing. A pool of one row equal to the rows every env holds is the feature
 * off, bit for bit.
 * nm_set_reset_rows: rows_dev is a DEVICE array [P, width] in the env's dtype ([P] int32 for kind 2), copied into memory of the env's
 *   own on `stream`; it switches the kind on, and the rows the envs hold stay until each env's next reset (nm_reset right after it
 *   draws k = 0 for every env). rows_dev NULL drops the pool: the rows stay what they are. Switching a kind off (its nm_set_* with NULL)
 *   drops its pool as well; setting rows by hand while a pool is installed holds until that env's next reset. Refused, named by
 *   nm_last_error, before anything of the env changes: a kind outside 0..5, P outside 1..65536, a NULL env (in this order, before the
 *   first device call), then a pool row that the kind's own setter would refuse (read back and judged on the host, which waits for
 *   `stream`; friction / gains: finite, mu > 1e-5, gains >= 0).
 * nm_get_reset_rows: P (0 = no pool) and, if out_dev is not NULL, the pool into a DEVICE array [P, width] on `stream`.
 * nm_set_reset_row_counts / nm_get_reset_row_counts: the HOST [N] reset-row counts (zeros at first use): a checkpoint's content.
 * nm_reset_rows_pick: i of all six kinds for reset k of the env with global id `global_env` and the pool sizes sizes[6] (size 0 -> 0),
 *   computed on the host by the function the kernels call; no env, no device. */
int nm_set_reset_rows(nm_env* env, int32_t kind, const void* rows_dev, int32_t P, void* stream);
int nm_get_reset_rows(nm_env* env, int32_t kind, int32_t* P, void* out_dev, void* stream);
int nm_set_reset_row_counts(nm_env* env, const uint32_t* counts_host);
int nm_get_reset_row_counts(nm_env* env, uint32_t* counts_host);
int nm_reset_rows_pick(uint64_t seed, int64_t global_env, uint32_t k, const uint32_t sizes[6], uint32_t out[6]);
/* State log (envs/nightmare_v3_env.py:261-272 records data[0]): env_index >= 0 makes every nm_step keep that env's
 * post-physics, pre-reset qpos/qvel; -1 = off. nm_get_state_record copies the last record to HOST qpos[25], qvel[24] and
 * the number of MuJoCo bad-state resets inside that step (data.time restarts there). Synchronous. */
int nm_set_state_record(nm_env* env, int32_t env_index);
int nm_get_state_record(nm_env* env, double* qpos, double* qvel, int32_t* bad_state_resets);
/* The same log inside a K-step launch (nm_rollout*, nm_play): with recording on, the launch keeps one row [qpos 25 | qvel 24 | bad-state
 * resets 1] per step for the chosen env (envs/nightmare_v3_env.py:261-272 appends one record per step; reader open_custom_play.py:50-66),
 * and nm_get_state_record returns the launch's last step. nm_get_state_log copies rows first_step .. first_step + count - 1 of the LAST
 * K-step launch to HOST rows_host[count, 50] (doubles). Synchronous. */
int nm_get_state_log(nm_env* env, int32_t first_step, int32_t count, double* rows_host);
/* The logged env's reset flag (reset_buf[0] at envs/nightmare_v3_env.py:263: the step at which the reader starts a new file) for the same
 * steps of the last nm_play launch, HOST dones_host[count] uint8. After nm_rollout* the flags are column env_index of its dones rows. Synchronous. */
int nm_get_state_log_dones(nm_env* env, int32_t first_step, int32_t count, unsigned char* dones_host);

/* Measurement hook (no reference counterpart): when enabled, every nm_step / nm_step_physics brackets its step
 * kernel with HIP events on the launch stream. Each call synchronises, returns the summed kernel time and the
 * launch count since the previous call, clears them, and sets the new enable state. */
int nm_profile(nm_env* env, int32_t enable, double* sum_ms, int64_t* count);
/* Which instantiation of the step kernel nm_step launches. The library holds two for fp32 envs without per-env rows: the generic one,
 * which asks the configuration at run time, and a lean one compiled for the shipped default configuration (the model's link frames,
 * solimp power 2, tibia / body contact mode 1, no reward term beyond the default table, no debug buffer, state record, observation
 * noise or injected command uniforms). Both compute the same bits. mode 0 (the default): the lean one whenever a launch qualifies,
 * decided per launch; mode 1: always the generic one. nm_get_step_variant returns what the last nm_step / nm_step_physics of this env
 * launched: 0 generic, 1 lean (0 before the first step). Every other launch (fp64, per-env rows set, nm_step_physics, the K-step
 * entry points) is generic. */
int nm_set_step_variant(nm_env* env, int32_t mode);
int nm_get_step_variant(nm_env* env);
/* Self-test of the lean kernel's cross-lane helpers (no env needed): each helper that the lean kernel takes in another form than the
 * generic kernels (csrc/simt.h: the half-wave row broadcast as two DPP moves, the lane-mask select as a compiler-visible instruction)
 * runs in both forms on the caller's values, one wave per 64 of them, a last partial wave included. Device x / a / g [n] floats, HOST
 * masks_host[4] lane masks; device out [2][36][n]: out[0] the generic forms, out[1] the lean forms; slot I < 32 is g + a * (x of lane I
 * of the lane's half-wave), slot 32 + k is a under masks_host[k] and g elsewhere. The two halves must agree bit for bit. Stream-ordered. */
#define NM_LANE_SELFTEST_SLOTS 36
int nm_lane_selftest(const float* x_dev, const float* a_dev, const float* g_dev, const uint64_t* masks_host, int32_t n, float* out_dev, void* stream);
/* Stage-skipping measurement switches are NOT part of this ABI: they exist only in the -DNM_MEASURE build
 * (libnightmare_hip_measure.so, include/nightmare_hip_measure.h). */

/* ---- Hidden-layer activation of the networks below (rsl_rl v1.0.2 ActorCritic's get_activation; the user's choice is the reference
 * config's `activation = 'elu' # can be elu, relu, selu, crelu, lrelu, tanh, sigmoid`, envs/nightmare_v3_config.py:109; crelu is a plain
 * ReLU upstream). SELU uses torch's constants, LRELU torch's default slope 0.01. Every entry point without an activation argument means
 * NM_ACT_ELU. An unknown code is refused before any device call (nm_last_error names it). */
typedef enum {
  NM_ACT_ELU = 0,
  NM_ACT_SELU = 1,
  NM_ACT_RELU = 2,
  NM_ACT_LRELU = 3,
  NM_ACT_TANH = 4,
  NM_ACT_SIGMOID = 5
} nm_activation;
#define NM_NUM_ACTIVATIONS 6

/* ---- ActorCritic MLP forward on the matrix cores (rsl_rl v1.0.2 ActorCritic: Linear -> activation x n_hidden -> Linear; reference call
 * sites play.py:122 `nn.act(obs)`, train.py:40), batched over envs, exact-f32 MFMA, all layers in one launch.
 * One handle = one network: it owns a packed copy of the parameters, so nothing is shared between networks, streams or devices.
 * dims = {n_in, h1, ..., n_out}, n_layers = len(dims) - 1. Networks of <= 4 layers and <= 256 units run fused; others per layer.
 * nm_policy_create: ELU hidden layers; nm_policy_create_act: any NM_ACT_* code (reference envs/nightmare_v3_config.py:109). */
typedef struct nm_policy nm_policy;
int nm_policy_create(const int32_t* dims, int32_t n_layers, int32_t device, nm_policy** out);
int nm_policy_create_act(const int32_t* dims, int32_t n_layers, int32_t activation, int32_t device, nm_policy** out);
int nm_policy_destroy(nm_policy* h);
/* Copy + repack the parameters (device f32, torch.nn.Linear layout: weights[l] is [out_l, in_l] row-major, bias[l] is [out_l]).
 * Stream-ordered; call again after every optimiser step / load_state_dict - the handle never reads the caller's tensors later. */
int nm_policy_load(nm_policy* h, const float* const* weights_dev, const float* const* bias_dev, void* stream);
/* out_dev[N, n_out] = MLP(obs_dev[N, n_in]) with the parameters of the last nm_policy_load. One launch on the fused path. */
int nm_policy_forward(nm_policy* h, const float* obs_dev, int32_t num_envs, float* out_dev, void* stream);

/* GAE(lambda) returns of one rollout (rsl_rl v1.0.2 RolloutStorage.compute_returns; caller reference train.py:54).
 * rewards/values/returns [T,N] f32, dones [T,N] u8, last_values [N] f32, all device memory. */
int nm_gae(const float* rewards_dev, const float* values_dev, const unsigned char* dones_dev, const float* last_values_dev,
           int32_t T, int32_t N, float gamma, float lam, float* returns_dev, void* stream);
/* The same plus the rest of RolloutStorage.compute_returns (rsl_rl v1.0.2 `storage/rollout_storage.py`; caller reference train.py:54):
 * advantages[T,N] = returns - values and, normalize != 0, (advantages - mean) / (std + 1e-8) over all T x N entries (unbiased std) - two
 * launches, reproducible summation order. scratch_dev: 2 * ceil(N / 256) floats. One GPU's envs only: a multi-rank job normalises over
 * all ranks (normalize = 0 here, then the caller's all-reduced statistics). */
int nm_gae_advantages(const float* rewards_dev, const float* values_dev, const unsigned char* dones_dev, const float* last_values_dev, int32_t T, int32_t N,
                      float gamma, float lam, float* returns_dev, float* advantages_dev, float* scratch_dev, int32_t normalize, void* stream);

/* Rollout collection of the on-policy loop (rsl_rl v1.0.2 PPO.act / PPO.process_env_step; caller reference train.py:54), one launch each.
 * nm_ppo_sample: net_out_dev [N, A+1] = action means | critic value (nm_policy_forward on the merged actor+critic network), std_dev [A];
 *   draws a = mean + std * N(0,1) from the counter generator keyed by (seed, *iter_dev, step, env, j) and writes step `step` of the rollout
 *   storage: actions/mu/sigma [N,A], log-probability and value [N], and (if obs_store_dev != NULL) a copy of obs_dev [N, n_obs].
 * nm_ppo_record: rewards_store = rew + gamma * value * time_out (time_outs_dev may be NULL), dones_store (u8), running episode return /
 *   length per env, and fin3_dev += (sum of returns, sum of lengths, count) over the episodes that ended in this step; if n_ep > 0 also the
 *   runner's sum of extras['episode'] over the rollout: ep_acc_dev[i] += ep_stats_dev[ep_idx_dev[i]], i < n_ep <= 256. */
int nm_ppo_sample(const float* net_out_dev, const float* std_dev, const float* obs_dev, int32_t N, int32_t A, int32_t n_obs, uint64_t seed,
                  const int64_t* iter_dev, int32_t step, float* actions_dev, float* logp_dev, float* values_dev, float* mu_dev, float* sigma_dev,
                  float* obs_store_dev, void* stream);
int nm_ppo_record(const float* rew_dev, const int64_t* done_dev, const float* time_outs_dev, const float* values_dev, float gamma, int32_t N,
                  float* rewards_store_dev, unsigned char* dones_store_dev, float* cur_ret_dev, float* cur_len_dev, float* fin3_dev,
                  const float* ep_stats_dev, const int32_t* ep_idx_dev, int32_t n_ep, float* ep_acc_dev, void* stream);
/* nm_ppo_sample for an asymmetric actor-critic: obs_dev [N, n_obs] is the CRITIC's row, whose first n_prefix columns are the actor's
 * observation. obs_store_dev (if not NULL) receives the rows as before; prefix_store_dev (if not NULL) [N, n_prefix] receives the
 * prefix - the storage's observations and privileged observations of one step, filled in the same launch. */
int nm_ppo_sample_prefix(const float* net_out_dev, const float* std_dev, const float* obs_dev, int32_t N, int32_t A, int32_t n_obs, uint64_t seed,
                         const int64_t* iter_dev, int32_t step, float* actions_dev, float* logp_dev, float* values_dev, float* mu_dev, float* sigma_dev,
                         float* obs_store_dev, int32_t n_prefix, float* prefix_store_dev, void* stream);

/* ---- PPO mini-batch update (rsl_rl v1.0.2 `algorithms/ppo.py` PPO.update: clipped surrogate + clipped value loss + entropy bonus,
 * adaptive-KL learning rate, gradient-norm clipping, Adam; caller reference train.py:54; hyper-parameters envs/nightmare_v3_config.py:111-128)
 * as two launches per mini-batch (forward/backward; then partial-gradient reduction, gradient-norm clip, KL-adaptive learning rate, Adam and
 * the repacking of the weights in one launch with one grid barrier) with no host synchronisation. actor_dims / critic_dims = {n_in, h1, ..., n_out} (same depth,
 * critic output 1, hidden activation ELU - or any NM_ACT_* code with nm_ppo_create_act, reference envs/nightmare_v3_config.py:109).
 * actor_dims[0] <= critic_dims[0]: the actor reads the FIRST actor_dims[0] columns of the row the critic reads (equal widths: the shared
 * observation; a wider critic row: observation + privileged columns, nm_privileged_obs). Every `obs` / n_obs below is then the critic's row
 * and its width. A wider actor is refused. Asymmetric networks run the generic kernels (nm_ppo_has_fast_path = 0).
 * The parameters live in ONE caller-owned flat device vector in the order
 * actor W0 b0 W1 b1 ..., critic W0 b0 ..., std[A] (W row-major [out, in] as torch.nn.Linear); Adam's moments in two more such vectors. */
typedef struct nm_ppo nm_ppo;
int nm_ppo_create(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers, int32_t device, nm_ppo** out);
int nm_ppo_create_act(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers, int32_t activation, int32_t device, nm_ppo** out);
int nm_ppo_destroy(nm_ppo* h);
int32_t nm_ppo_num_params(const nm_ppo* h);
/* (re)read the flat parameters (after load_state_dict or a step taken elsewhere) and set the learning rate / Adam step count */
int nm_ppo_sync_params(nm_ppo* h, const float* flat_dev, float lr, int64_t step, void* stream);
/* one mini-batch: rows of obs [B,n_obs], actions / old_mu / old_sigma [B,A], old_logp / adv / ret / target_values [B] (device f32).
 * phase 0 = everything; 1 = gradient only (fetch it with nm_ppo_copy_grad, e.g. for an all-reduce); 2 = the step from the current gradient, the KL of the
 * learning-rate rule read from the slot behind it (kl_override >= 0 replaces the KL mean in either phase, < 0 keeps it).
 * Data-parallel update: phase 1, nm_ppo_copy_grad(0), all-reduce + divide by the ranks, nm_ppo_copy_grad(1), phase 2 - one collective
 * per mini-batch, no host synchronisation. */
int nm_ppo_minibatch(nm_ppo* h, float* flat_dev, float* exp_avg_dev, float* exp_avg_sq_dev, const float* obs, const float* actions,
                     const float* old_mu, const float* old_sigma, const float* old_logp, const float* adv, const float* ret, const float* target_values,
                     int32_t B, int32_t n_obs, float clip, float value_coef, float entropy_coef, int32_t clip_value, float desired_kl,
                     int32_t adaptive, float max_grad_norm, float beta1, float beta2, float eps, int32_t phase, float kl_override, void* stream);
/* nm_ppo_minibatch with the mini-batch given as ROW NUMBERS into the whole rollout (rsl_rl's mini_batch_generator gathers obs[batch_idx], ...;
 * here the forward / backward kernel gathers the rows itself, nothing is copied): row i of the mini-batch is row rows_dev[i] (int32, device)
 * of the [T*N, .] arrays. rows_dev == NULL = rows 0..B-1 (nm_ppo_minibatch). */
int nm_ppo_minibatch_rows(nm_ppo* h, float* flat_dev, float* exp_avg_dev, float* exp_avg_sq_dev, const float* obs, const float* actions,
                          const float* old_mu, const float* old_sigma, const float* old_logp, const float* adv, const float* ret, const float* target_values,
                          const int32_t* rows_dev, int32_t B, int32_t n_obs, float clip, float value_coef, float entropy_coef, int32_t clip_value, float desired_kl,
                          int32_t adaptive, float max_grad_norm, float beta1, float beta2, float eps, int32_t phase, float kl_override, void* stream);
/* Declares how many rows the [T*N, .] arrays behind a row list hold (row numbers are in [0, n_rows)); must precede nm_ppo_minibatch_rows with
 * rows_dev != NULL. LIMIT: the kernels address a row as base + a 32-bit byte offset, so n_rows * max(n_obs, n_actions) * 4 must stay below
 * 2^32 (16.2 M rows of 66 floats; BASELINE config 5 has 32768 x 80 = 2.6 M); beyond it this call - and nm_ppo_minibatch for B - fails. */
int nm_ppo_set_storage_rows(nm_ppo* h, int64_t n_rows);
/* 1 if the mini-batch step of this handle is the one-launch k_ppo_step (one grid barrier), 0 if it is the four-launch chain: asked for with
 * NM_PPO_UNFUSED_STEP=1, chosen at creation because the device cannot hold the step's grid at once (occupancy query), or after a barrier
 * time-out. A barrier that times out makes that step and every later fused step a NO-OP (no parameter, moment or packed weight is written)
 * until nm_ppo_get_state has reported it. */
int32_t nm_ppo_step_is_fused(const nm_ppo* h);
/* TEST HOOK: the next fused step's grid barrier will time out (about one second of spinning), to exercise the no-op path. */
int nm_ppo_debug_break_barrier(nm_ppo* h, void* stream);
/* The mini-batch order of one PPO.update (rsl_rl v1.0.2 mini_batch_generator: indices = torch.randperm(num_mini_batches * mini_batch_size)):
 * out_dev[i] (int32) = image of i under a pseudo-random permutation of 0..n-1 keyed by (seed, counter) - a cycle-walked Feistel network,
 * one launch, no sort. */
int nm_ppo_permutation(int32_t* out_dev, int32_t n, uint64_t seed, uint64_t counter, void* stream);
/* 1 if the network runs on the compiled register-resident kernels (the reference's 66 -> 54 -> 42 -> 30 -> 18 | 1 shape, any activation), else 0 */
int32_t nm_ppo_has_fast_path(const nm_ppo* h);
/* rsl_rl v1.0.2 PPO.act (caller reference train.py:54) in ONE launch, fast-path networks only: merged actor+critic forward from the
 * update's packed weights (always current: no repack between update and collection), then exactly what nm_ppo_sample does */
int nm_ppo_act(nm_ppo* h, const float* flat_dev, const float* obs_dev, int32_t N, uint64_t seed, const int64_t* iter_dev, int32_t step,
               float* actions_dev, float* logp_dev, float* values_dev, float* mu_dev, float* sigma_dev, float* obs_store_dev, void* stream);
/* nm_ppo_record of the PREVIOUS step and nm_ppo_act of this one in one launch (the record part runs first; arguments as in the two
 * calls, prev_values_dev = the values nm_ppo_act filed for the previous step): PPO.process_env_step(s - 1) + PPO.act(s) of rsl_rl
 * v1.0.2 (caller reference train.py:54). A rollout of T steps needs T + 1 of these launches besides the env's instead of 2 T. */
int nm_ppo_record_act(nm_ppo* h, const float* rew_dev, const int64_t* done_dev, const float* time_outs_dev, const float* prev_values_dev, float gamma,
                      float* rewards_store_dev, unsigned char* dones_store_dev, float* cur_ret_dev, float* cur_len_dev, float* fin3_dev,
                      const float* ep_stats_dev, const int32_t* ep_idx_dev, int32_t n_ep, float* ep_acc_dev,
                      const float* flat_dev, const float* obs_dev, int32_t N, uint64_t seed, const int64_t* iter_dev, int32_t step,
                      float* actions_dev, float* logp_dev, float* values_dev, float* mu_dev, float* sigma_dev, float* obs_store_dev, void* stream);
/* gradient of the last mini-batch in flat order followed by the mini-batch's mean KL to the behaviour policy, [num_params + 1] floats:
 * direction 0 copies them to grad_dev, 1 replaces them by grad_dev */
int nm_ppo_copy_grad(nm_ppo* h, float* grad_dev, int32_t direction, void* stream);
/* The same vector in a buffer the caller owns ([num_params + 1] floats on the device): phase 1 writes gradient | KL there, phase 2 reads it
 * from there, and a data-parallel update all-reduces it IN PLACE between the two - one collective per mini-batch and nothing else (the 60 KB
 * gradient all-reduce of SURVEY 8(e); rsl_rl v1.0.2 itself is single-process, caller reference train.py:54). NULL = the handle's own buffer. */
int nm_ppo_set_grad_buffer(nm_ppo* h, float* grad_kl_dev);
/* HOST out[8]: lr, Adam steps, last KL, sum of value losses, sum of surrogate losses, mini-batches, clip coefficient, grad norm;
 * reset_sums != 0 clears the two loss sums and the count afterwards. Synchronises the stream. */
int nm_ppo_get_state(nm_ppo* h, float* out8_host, int32_t reset_sums, void* stream);
/* DEVICE out[9]: the same eight values and, [8], != 0 if the fused step's grid barrier timed out in the launches since the last read.
 * Stream-ordered, no host synchronisation (rsl_rl's OnPolicyRunner.log reads its statistics after every update, caller reference
 * train.py:54; the runner here reads this snapshot one iteration later, while the next rollout is already running). */
int nm_ppo_snapshot_state(nm_ppo* h, float* out9_dev, int32_t reset_sums, void* stream);

/* ---- The collection loop of rsl_rl v1.0.2 OnPolicyRunner.learn (`for i in range(num_steps_per_env): actions = alg.act(obs, critic_obs);
 * obs, _, rewards, dones, infos = env.step(actions); alg.process_env_step(rewards, dones, infos)`; caller reference train.py:54, horizon
 * envs/nightmare_v3_config.py:135) as ONE launch of `steps` steps: every wavefront keeps its two envs for the whole rollout and evaluates
 * the policy itself between two physics steps (no launch per step, no wait for the step's slowest env). Networks of the reference's shape
 * (envs/nightmare_v3_config.py:105-109; nm_rollout_supported) on the fp32 env only. Results per step are those of the step-by-step path
 * nm_rollout_act + nm_step + nm_ppo_record: bit-identical observations / actions / values / log-probabilities / rewards / dones in the storage
 * (sums that go through float atomics - fin3, ep_acc, ep_stats - agree to rounding). All pointers are device memory except the dims. */
typedef struct {
  int32_t steps;                       /* K, at most the episode length in steps */
  const float* params_flat_dev;        /* actor W0 b0 W1 b1 ..., critic W0 b0 ..., std[18] (the flat vector of nm_ppo_*) */
  uint64_t seed;                       /* action noise: counter generator keyed by (seed, *iter_dev, step, env, action pair) like nm_ppo_sample */
  const int64_t* iter_dev;
  const float* obs0_dev;               /* [N,66] the observation the first act sees (the env's current observation) */
  float* obs_final_dev;                /* [N,66] receives the observation after the last step (may alias obs0_dev) */
  int64_t* episode_length_dev;         /* [N] episode_length_buf, in/out */
  float* rew_dev; int64_t* done_dev;   /* [N] the env's reward / reset buffers: hold the last step's values afterwards */
  float* time_outs_dev;                /* [N] extras['time_outs'] in/out (NULL: not kept), ep_stats_dev [NM_NUM_REWARDS] extras['episode'] in/out */
  float* ep_stats_dev;
  int32_t bootstrap_time_outs;         /* 1: rewards += gamma * value * extras['time_outs'] (what PPO.process_env_step does when the env sends time_outs,
                                          cfg.env.send_timeouts, envs/nightmare_v3_env.py:369); 0: the buffer is kept up to date, the rewards stay raw */
  float *s_obs, *s_actions, *s_logp, *s_values, *s_mu, *s_sigma, *s_rewards;   /* rollout storage rows [K,N,66] [K,N,18] [K,N] [K,N] [K,N,18] [K,N,18] [K,N] */
  unsigned char* s_dones;              /* [K,N] */
  float gamma;                         /* time-out bootstrap: rewards += gamma * value * extras['time_outs'] (PPO.process_env_step) */
  float *cur_ret, *cur_len, *fin3;     /* [N] [N] [3]: as nm_ppo_record */
  const int32_t* ep_idx_dev; int32_t n_ep; float* ep_acc_dev;   /* ep_acc[i] += extras['episode'][ep_idx[i]] after every step, i < n_ep <= NM_NUM_REWARDS */
  float* last_values_dev;              /* [N] or NULL: the critic's value of the observation after the last step - rsl_rl PPO.compute_returns'
                                          `last_values = actor_critic.evaluate(last_critic_obs)` - evaluated by the env's wave at the end of the launch */
} nm_rollout_args;
/* 1 if nm_rollout / nm_rollout_act are compiled for these networks (dims = {n_obs, h1, h2, h3, n_out}, HOST arrays); ELU hidden layers */
int nm_rollout_supported(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers);
/* the same for hidden layers of activation `activation` (reference envs/nightmare_v3_config.py:109): 0 for an unknown code. Host only. */
int nm_rollout_supported_act(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers, int32_t activation);
int nm_rollout(nm_env* env, const nm_rollout_args* args, void* stream);
/* nm_rollout for networks with hidden activation `activation` (NM_ACT_*; reference envs/nightmare_v3_config.py:109, collection loop train.py:54).
 * nm_rollout = nm_rollout_ex(..., NM_ACT_ELU, ...). */
int nm_rollout_ex(nm_env* env, const nm_rollout_args* args, int32_t activation, void* stream);
/* PPO.act alone, on the code the rollout's waves run (one wave = two envs): the per-step counterpart of nm_rollout. Arguments as nm_ppo_act. */
int nm_rollout_act(nm_env* env, const float* params_flat_dev, const float* obs_dev, uint64_t seed, const int64_t* iter_dev, int32_t step,
                   float* actions_dev, float* logp_dev, float* values_dev, float* mu_dev, float* sigma_dev, float* obs_store_dev, void* stream);
/* nm_rollout_act with hidden activation `activation` (the per-step counterpart of nm_rollout_ex; reference envs/nightmare_v3_config.py:109,
 * PPO.act caller train.py:54). nm_rollout_act = nm_rollout_act_ex(..., NM_ACT_ELU, ...). */
int nm_rollout_act_ex(nm_env* env, const float* params_flat_dev, const float* obs_dev, uint64_t seed, const int64_t* iter_dev, int32_t step,
                      float* actions_dev, float* logp_dev, float* values_dev, float* mu_dev, float* sigma_dev, float* obs_store_dev, int32_t activation,
                      void* stream);

/* ---- The same collection loop for the asymmetric actor-critic (no upstream line for the rows: the reference's critic reads the actor's
 * observation, envs/nightmare_v3_config.py:105-109; the loop is train.py:54's `alg.act(obs, critic_obs)` with critic_obs = the privileged
 * row of nm_privileged_obs). Actor {66,54,42,30,18} on columns 0..65 of the row, critic {89,54,42,30,1} on all NM_NUM_PRIVILEGED_OBS of it.
 * The wave that owns the env gathers the privileged columns itself between two steps, with the arithmetic of nm_privileged_obs (the same
 * bits), where the per-step path calls it: behind the step's reset draws, in front of the next step's push and wrench. */
typedef struct {
  const float* priv0_dev;              /* [N,89] the row the first act sees (the env's current privileged row); nm_rollout_args.obs0_dev is not read */
  float* priv_final_dev;               /* [N,89] receives the row after the last step (a buffer of its own, as the env double-buffers it); last_values_dev is evaluated on it */
  float* s_priv;                       /* [K,N,89] storage: row t = what act t saw; s_obs row t = its first 66 columns */
} nm_rollout_priv_args;
/* 1 exactly for actor_dims {66,54,42,30,18}, critic_dims {89,54,42,30,1}, n_layers 4 and a known activation code (reference hidden layers and
 * activation: envs/nightmare_v3_config.py:107-109). Host only. */
int nm_rollout_supported_priv(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers, int32_t activation);
/* nm_rollout_ex with the privileged rows (collection loop: reference train.py:54). params_flat_dev is the flat vector of the 66 / 89 networks
 * (actor W0 [54,66] ..., critic W0 [54,89] ..., std[18]). Refuses an fp64 env, steps beyond the episode length and NULL privileged pointers. */
int nm_rollout_priv(nm_env* env, const nm_rollout_args* args, const nm_rollout_priv_args* priv, int32_t activation, void* stream);
/* nm_rollout_act_ex reading an [N,89] row (PPO.act caller: reference train.py:54): the step-by-step reference of nm_rollout_priv.
 * obs_store_dev [N,66] receives the row's first 66 columns, row_store_dev [N,89] the row; either may be NULL. Refuses an fp64 env. */
int nm_rollout_act_priv(nm_env* env, const float* params_flat_dev, const float* rows_dev, uint64_t seed, const int64_t* iter_dev, int32_t step,
                        float* actions_dev, float* logp_dev, float* values_dev, float* mu_dev, float* sigma_dev, float* obs_store_dev,
                        float* row_store_dev, int32_t activation, void* stream);

/* ---- Playing a policy (the loop of reference play.py:118-132: `actions = nn.act(obs)`, scale / clip, servo command, mj_step x decimation)
 * as ONE launch of `steps` steps with nothing collected for PPO: every wavefront keeps its two envs, evaluates the actor on the observation
 * its previous step left and steps the env. fp32 env, networks nm_play_supported accepts. Per step the results are those of nm_rollout_act_ex
 * (its `mu` row when deterministic, its `actions` row otherwise; noise key step = step0 + t) followed by nm_step, bit for bit; extras
 * (time_outs, ep_stats), counters and episode lengths afterwards are what the last of `steps` nm_step calls would have left. `steps` may
 * exceed the episode length (an env may time out several times per launch). All pointers are device memory. */
typedef struct {
  int32_t steps;                       /* K in 1..4096; longer runs are consecutive launches (step0 continues the noise keys) */
  int32_t deterministic;               /* != 0: action = actor mean (rsl_rl act_inference); 0: mean + std * N(0,1) (nn.act, reference play.py:122) */
  const float* params_flat_dev;        /* actor W0 b0 W1 b1 ..., critic W0 b0 ..., std[18]: the flat vector nm_rollout reads (the critic's shape is the reference's) */
  uint64_t seed;                       /* action noise: (seed, *iter_dev * 4096 + step0 + t, env, action pair), the keys of nm_rollout_act_ex */
  const int64_t* iter_dev;
  uint64_t step0;
  const float* obs0_dev;               /* [N,66] the observation the first act sees */
  float* obs_dev;                      /* [N,66] every step files its observation here; holds the last one afterwards (may alias obs0_dev) */
  float* actions_dev;                  /* [N,18] the actions of the step under way; holds the last step's afterwards */
  int64_t* episode_length_dev;         /* [N] episode_length_buf, in/out */
  float* rew_dev; int64_t* done_dev;   /* [N] reward / reset buffers: the last step's values afterwards */
  float* time_outs_dev;                /* [N] extras['time_outs'] in/out or NULL */
  float* ep_stats_dev;                 /* [NM_NUM_REWARDS] extras['episode'] in/out or NULL */
  float *cur_ret, *cur_len, *fin3;     /* [N] [N] [3] or NULL: running return / length per env, finished episodes (sum of returns, of lengths, count) as nm_ppo_record */
  float *ret_sum, *ret_cnt;            /* [N] [N] or NULL: per env the sum and the number of the returns of the episodes it finished (no atomics) */
  const int32_t* ep_idx_dev; int32_t n_ep; float* ep_acc_dev;   /* ep_acc[i] += extras['episode'][ep_idx[i]] after every step, as nm_rollout */
} nm_play_args;
/* 1 if nm_play is compiled for this actor (dims = {n_obs, h1, h2, h3, n_actions}, HOST array; reference play.py:118-132 plays the network of
 * envs/nightmare_v3_config.py:105-109) with hidden activation `activation`; the shapes nm_rollout_supported_act accepts. Host only. */
int nm_play_supported(const int32_t* actor_dims, int32_t n_layers, int32_t activation);
/* reference play.py:118-132, `steps` iterations per launch; stream-ordered, no host synchronisation */
int nm_play(nm_env* env, const nm_play_args* args, int32_t activation, void* stream);

/* ---- Stepping from an action tape: K x env.step(actions[t]) (reference envs/nightmare_v3_env.py:145-311, the joint-target hook at :186;
 * the loop of custom_play.py:66-76 and of every caller that already has its actions) as ONE launch. No policy, no sampling: before step t the
 * env's wavefront takes row t of the tape as its actions. fp32 env only. Afterwards every buffer, extra (time_outs, ep_stats), counter and
 * episode length is what the last of `steps` nm_step calls with those actions would have left, bit for bit; sums that go through float
 * atomics (fin3, ep_acc, ep_stats) agree to rounding, as for nm_play. `steps` may exceed the episode length. Observation noise and the
 * state log (nm_set_state_record, nm_get_state_log, nm_get_state_log_dones) work as in nm_play. All pointers are device memory. */
typedef struct {
  int32_t steps;                      /* K in 1..4096 */
  const float* actions_dev;           /* [K,N,18] the tape; row t is what nm_step would be given at step t */
  float* obs_dev;                     /* [N,66] holds the last step's observation afterwards */
  int64_t* episode_length_dev; float* rew_dev; int64_t* done_dev;   /* as nm_play_args */
  float* time_outs_dev; float* ep_stats_dev;                         /* or NULL */
  float *cur_ret, *cur_len, *fin3, *ret_sum, *ret_cnt;               /* or NULL, pairs as nm_play_args */
  const int32_t* ep_idx_dev; int32_t n_ep; float* ep_acc_dev;
  float* rec_obs_dev;                 /* [K,N,66] or NULL: the observation every step returned (obs_dev then receives a copy of the last row) */
  float* rec_rew_dev;                 /* [K,N]    or NULL */
  unsigned char* rec_done_dev;        /* [K,N]    or NULL */
} nm_tape_args;
/* reference custom_play.py:66-76 / envs/nightmare_v3_env.py:145-311, `steps` iterations per launch; stream-ordered, no host synchronisation */
int nm_step_tape(nm_env* env, const nm_tape_args* args, void* stream);

/* ---- scripted gait / IK engine (reference nikengine/engine.py; caller custom_play.py:49-76), batched over envs ----
 * One handle = num_envs independent EngineNode objects (engine.py:660-677), all in IdleState. */
typedef struct nm_nik nm_nik;
nm_nik* nm_nik_create(int32_t num_envs, int32_t device);
void nm_nik_destroy(nm_nik* h);
/* back to IdleState with the default pose (a fresh EngineNode). ids_host NULL = all envs. */
int nm_nik_reset(nm_nik* h, const int32_t* ids_host, int32_t n, void* stream);
/* state.cmd.gait (engine.py:297; the gait table :214-225): 0 'tripod' (default), 1 'ripple', 2 'wave'; ids_host NULL = all envs. Upstream the
 * field sits on a Command object shared by every EngineNode (RobotState.cmd is a class attribute, :402-406) and EngineNode.update does not
 * touch it; here it is per env. Takes effect like upstream: when WalkState is entered (:543) or the running step completes (:627). */
int nm_nik_set_gait(nm_nik* h, const int32_t* ids_host, int32_t n, int32_t gait, void* stream);
/* EngineNode.update(lin_speed, ang_speed, state, mode) (engine.py:710-715) for every env, one launch.
 *   lin_dev, ang_dev [N] f64 device: walk translation along +y (m/s) and yaw rate (rad/s) commands
 *   awake_dev, walk_dev [N] u8 device or NULL: state == 'awake' (else 'idle'), mode == 'walk' (else 'stand'); NULL = 1
 *   now_s: the engine clock (set_time_s, engine.py:12-19); engine_fps: config.ENGINE_FPS, read every tick like upstream
 *   angles_f32_dev / angles_f64_dev [N,18] device, either may be NULL: the 18 joint targets set_hardware_pose returns
 *   (IK + SERVO_OFFSET + URDF_JOINT_OFFSETS, engine.py:700-708). Arithmetic is f64. */
int nm_nik_update(nm_nik* h, const double* lin_dev, const double* ang_dev, const unsigned char* awake_dev,
                  const unsigned char* walk_dev, double now_s, double engine_fps, float* angles_f32_dev,
                  double* angles_f64_dev, void* stream);
/* K ticks of EngineNode.update in ONE launch (the engine is open loop: reference custom_play.py:66-76 feeds it commands and the clock,
 * never the env), the FSM state in registers. Tick t runs at now = (double)(tick0 + t) * dt (one IEEE multiply) and writes row t of a
 * [K,N,18] tape of set_hardware_pose's joint targets, bit for bit what K nm_nik_update calls with those clocks write; afterwards the
 * handle's state (fsm, gait step, gait, t0, gait_step_state, pose, start, last) is theirs.
 * Optional servo stage (servo_targets_dev and actions_dev both non-NULL, or both NULL): custom_play.py:72's rate limit and the inverse of
 * the env's action -> joint target mapping (envs/nightmare_v3_env.py:152-156,183-188, hook :186) in fp32, every operation rounded on its
 * own: q += clamp(float(goal) - q, -action_rate, +action_rate); a = (q + default_pos[j % 3]) * inv_action_scale. The mapping MULTIPLIES by
 * inv_action_scale = float32(1.0 / action_scale), computed by the host (the library has no correctly rounded fp32 division). */
typedef struct {
  int32_t steps;                      /* K >= 1 */
  const double *lin_dev, *ang_dev;    /* [N] commands, held for the K ticks */
  const unsigned char *awake_dev, *walk_dev;   /* [N] or NULL = 1 */
  int64_t tick0; double dt;           /* engine clock of tick t: now = (double)(tick0 + t) * dt  (one IEEE multiply) */
  double engine_fps;
  double* angles_f64_dev;             /* [K,N,18] or NULL: set_hardware_pose's joint targets per tick */
  float*  angles_f32_dev;             /* [K,N,18] or NULL: the same, rounded once */
  /* optional servo stage (all or none): custom_play.py:72 rate limit + the inverse of env.py:152-156,183-188 */
  float*  servo_targets_dev;          /* [N,18] in/out: the rate limiter's memory */
  float   action_rate;                /* q += clamp(float(goal) - q, -action_rate, +action_rate) */
  float   default_pos[3]; float inv_action_scale;   /* a = (q + default_pos[j % 3]) * inv_action_scale */
  float*  actions_dev;                /* [K,N,18]: what nm_step_tape reads */
} nm_nik_tape_args;
int nm_nik_tape(nm_nik* h, const nm_nik_tape_args* args, void* stream);
/* FSM inspection for tests: HOST pose [N,18] (foot positions in the body frame), fsm id [N]
 * (0 idle 1 adjust-get-up 2 get-up 3 sit 4 adjust-sit 5 stand 6 walk), gait_step_state [N]. NULL = skip. Synchronous. */
int nm_nik_get_state(nm_nik* h, double* pose_host, int32_t* fsm_host, double* gait_step_state_host);

#ifdef __cplusplus
}
#endif
#endif
