// nm_hip.hip - gfx950 kernels + the C ABI of include/nightmare_hip.h. Device-only: there is no CPU path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nightmare_hip.h"
#include "nm_host_model.h"
#include "nm_env_loop.h"
#include "nm_env_rows.h"
#include "nm_priv_obs.h"
#include "nm_push.h"
#include "nm_reset_noise.h"
#include "nm_reset_rows.h"
#include "nm_rollout.h"
#include "nm_sensor.h"
#include "nm_wrench.h"

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return 1; }
#define HIPCHK(x)                                                                                        \
  do {                                                                                                   \
    hipError_t e_ = (x);                                                                                 \
    if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_));                  \
  } while (0)

#include "nm_step_kernel.h"


// reset_idx (reference envs/nightmare_v3_env.py:335-371): one thread per env to reset
template <class real>
__global__ void k_reset(nm::Model<real> M, nm::Args<real> A, const int32_t* ids, int n) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int env = ids ? ids[j] : j;
  for (int k = 0; k < nm::kNQ; k++) A.qpos[env * nm::kNQ + k] = M.qpos0[k];
  for (int k = 0; k < nm::kNV; k++) A.qvel[env * nm::kNV + k] = real(0);
  real ux, uy;
  uint32_t ctr = A.rngctr[env];
  if (A.cmd_u) { ux = A.cmd_u[env * 4 + 2]; uy = A.cmd_u[env * 4 + 3]; }
  else {
    ux = (real)nm::rand_u24_bits(A.seed, (uint64_t)(A.env_offset + env), ctr) * real(1.0 / 16777216.0);
    uy = (real)nm::rand_u24_bits(A.seed, (uint64_t)(A.env_offset + env), ctr + 1) * real(1.0 / 16777216.0);
    ctr += 2;
  }
  real c0 = ux * real(2) * M.max_lin_x - M.max_lin_x, c2 = uy * real(2) * M.max_ang - M.max_ang;
  real keep = sqrt(c0 * c0) > real(0.02) ? real(1) : real(0);
  A.cmd[env * 3] = c0 * keep; A.cmd[env * 3 + 1] = real(0); A.cmd[env * 3 + 2] = c2;
  A.rngctr[env] = ctr;
  A.eplen[env] = 0;
  for (int k = 0; k < nm::kNLEG; k++) A.feetair[env * nm::kNLEG + k] = real(0);   // env.py:359 (last_contacts* are not cleared)
  for (int k = 0; k < nm::kNREW; k++) {
    atomicAdd(A.stat_sum + k, A.epsum[env * nm::kNREW + k]);
    A.epsum[env * nm::kNREW + k] = real(0);
  }
  atomicAdd(A.stat_cnt, 1);
}

// the same closing step as a kernel of its own, for reset_idx() (k_reset fills the accumulators, nothing else is in flight)
template <class real>
__global__ void k_finalize(int N, real* stat_sum, int* stat_cnt, float* ep_stats, const float* timeout_now, float* time_outs,
                           real ep_len_s, long long* counters) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = stat_cnt[0];
  __syncthreads();
  if (cnt > 0) {
    if (threadIdx.x < nm::kNREW && ep_stats) ep_stats[threadIdx.x] = (float)(stat_sum[threadIdx.x] / (real)cnt / ep_len_s);
    if (time_outs && timeout_now)
      for (int i = threadIdx.x; i < N; i += blockDim.x) time_outs[i] = timeout_now[i];
  }
  __syncthreads();
  if (threadIdx.x < nm::kNREW) stat_sum[threadIdx.x] = real(0);
  if (threadIdx.x == 0) {
    stat_cnt[0] = 0;
    counters[0] += stat_cnt[1];
    counters[1] += stat_cnt[2];
    counters[2] += stat_cnt[3];
    stat_cnt[1] = 0;
    stat_cnt[2] = 0;
    stat_cnt[3] = 0;
  }
}

// Per-env physics parameters (nm::Args::envp rows: mu, p_gain, kv, pad), one thread per (env, column). `set`: a column comes from the
// caller's [N] array, or is the default where there is none. `get`: the columns of the rows, or the defaults where there are no rows.
// `draw`: lo + u (hi - lo) in the env's precision, product and sum rounded separately (contraction switched off: a host restatement in
// plain arithmetic gives the same bits), u = rand_u24_bits(seed + kEnvParamKey, global env id, column) * 2^-24.
template <class real, int L> struct Vals { real v[L]; };      // L values as one kernel argument
template <class real> using EnvP3 = Vals<real, 3>;
template <class real> struct EnvP3P { const real* p[3]; };
template <class real> struct EnvP3W { real* p[3]; };
template <class real>
__global__ void k_envp_set(real* __restrict__ rows, int N, EnvP3P<real> src, EnvP3<real> dflt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * N) return;
  const int env = i >> 2, col = i & 3;
  real v = real(0);
  if (col < 3) v = src.p[col] ? src.p[col][env] : dflt.v[col];
  rows[i] = v;
}
template <class real>
__global__ void k_envp_get(const real* __restrict__ rows, int N, EnvP3W<real> dst, EnvP3<real> dflt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * N) return;
  const int env = i >> 2, col = i & 3;
  if (col < 3 && dst.p[col]) dst.p[col][env] = rows ? rows[i] : dflt.v[col];
}
// (the pragma, not __fmul_rn / __fadd_rn: those are plain inline * and + here and fuse into one v_fma once inlined)
template <class real> __device__ __forceinline__ real envp_lerp(real lo, real u, real d) {
#pragma clang fp contract(off)
  const real p = u * d;
  return lo + p;
}
// The uniform draw of every kind (friction / gains into the rows; payload and gravity parameters into the caller's buffer): C columns per
// env at a stride of S words, the pad columns zero, under the kind's own `key`.
template <class real, int C, int S>
__global__ void k_uniform_draw(real* __restrict__ out, int N, uint64_t seed, uint64_t key, int64_t env_offset, Vals<real, C> lo, Vals<real, C> hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * N) return;
  const int env = i / S, col = i - S * env;
  real v = real(0);
  if (col < C) {
    const real u = (real)nm::rand_u24_bits(seed + key, (uint64_t)(env_offset + env), (uint32_t)col) * real(1.0 / 16777216.0);
    v = envp_lerp(lo.v[col], u, hi.v[col] - lo.v[col]);
  }
  out[i] = v;
}
// `fill`: one row of W words for every env - a kind's default row, into its region or into the caller's buffer (what nm_get_body_params /
// nm_get_gravity report while the block does not exist).
template <class real, int W>
__global__ void k_row_fill(real* __restrict__ rows, int N, Vals<real, W> row) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * N) return;
  rows[i] = row.v[i % W];
}

// Per-env actuation latency (nm_core.h kLatP): delay[e] = lo + floor(u (hi - lo + 1)), u = bits * 2^-24 with bits =
// rand_u24_bits(seed + kLatencyKey, global env id, 0): in integers, lo + ((bits * (hi - lo + 1)) >> 24) - exact, the same in either dtype.
__global__ void k_latency_draw(int* __restrict__ delay, int N, uint64_t seed, int64_t env_offset, int lo, int hi) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const uint64_t bits = nm::rand_u24_bits(seed + nm::kLatencyKey, (uint64_t)(env_offset + e), 0u);
  delay[e] = lo + (int)((bits * (uint64_t)(hi - lo + 1)) >> 24);
}

// ------------------------------------------------------------------------------------------------ host object
struct nm_env {
  int N = 0, device = 0, dtype = 0;
  virtual ~nm_env() {}
  virtual int reset(const int32_t* ids, int n, int64_t* eplen, float* ep_stats, hipStream_t s) = 0;
  virtual int step(const float* actions, int64_t* eplen, float* obs, float* rew, int64_t* done, float* time_outs, float* ep_stats,
                   int physics_only, hipStream_t s) = 0;
  virtual int get_state(double* qpos, double* qvel, double* qw) = 0;
  virtual int set_state(const double* qpos, const double* qvel, const double* qw) = 0;
  virtual int get_buffers(double* dp, double* dv, double* act, double* cmd, double* es) = 0;
  virtual int set_buffers(const double* dp, const double* dv, const double* act, const double* cmd, const double* es) = 0;
  virtual int set_cmd_u(const double* u) = 0;
  virtual int get_feet(double* air, unsigned char* last, unsigned char* filt) = 0;
  virtual int set_feet(const double* air, const unsigned char* last, const unsigned char* filt) = 0;
  virtual int counters(int64_t* out) = 0;
  virtual void set_dbg(void* p) = 0;
  virtual void set_ret_acc(float* p) = 0;
  virtual int invalidate_time_outs(hipStream_t s) = 0;
  virtual int rollout(const nm_rollout_args* r, int act, hipStream_t s) = 0;
  virtual int rollout_act(const float* flat, const float* obs, uint64_t seed, const int64_t* iter_dev, int step, int act, float* actions, float* logp, float* values,
                          float* mu, float* sigma, float* obs_store, hipStream_t s) = 0;
  virtual int profiling(int on, double* sum_ms, int64_t* count) = 0;
  virtual void set_ablate(int m) = 0;
  virtual int set_noise(const double* vec) = 0;
  virtual int set_noise_u(const double* u) = 0;
  virtual int set_record(int idx) = 0;
  virtual int get_record(double* qpos, double* qvel, int32_t* nbad) = 0;
  virtual int play(const nm_play_args* r, int act, hipStream_t s) = 0;
  virtual int tape(const nm_tape_args* r, hipStream_t s) = 0;
  virtual int get_log(int first, int count, double* rows) = 0;
  virtual int get_log_dones(int first, int count, unsigned char* dones) = 0;
  virtual int set_env_params(const void* mu, const void* p_gain, const void* kv, hipStream_t s) = 0;
  virtual int get_env_params(void* mu, void* p_gain, void* kv, hipStream_t s) = 0;
  virtual int draw_env_params(const double* lo, const double* hi, hipStream_t s) = 0;
  virtual int set_body_params(const void* rows, hipStream_t s) = 0;
  virtual int get_body_params(void* out, hipStream_t s) = 0;
  virtual int draw_payload(const double* lo, const double* hi, void* out, hipStream_t s) = 0;
  virtual int set_action_latency(const int* substeps, hipStream_t s) = 0;
  virtual int get_action_latency(int* out, hipStream_t s) = 0;
  virtual int draw_action_latency(int lo, int hi, hipStream_t s) = 0;
  virtual int set_action_history(const float* h, hipStream_t s) = 0;
  virtual int get_action_history(float* out, hipStream_t s) = 0;
  virtual int set_gravity(const void* rows, hipStream_t s) = 0;
  virtual int get_gravity(void* out, hipStream_t s) = 0;
  virtual int draw_gravity(const double* lo, const double* hi, void* out, hipStream_t s) = 0;
  virtual int set_servo(const void* rows, hipStream_t s) = 0;
  virtual int get_servo(void* out, hipStream_t s) = 0;
  virtual int draw_servo(const double* lo, const double* hi, hipStream_t s) = 0;
  virtual int get_servo_state(double* L) = 0;
  virtual int set_servo_state(const double* L) = 0;
  virtual int set_torque_limit(const void* rows, hipStream_t s) = 0;
  virtual int get_torque_limit(void* out, hipStream_t s) = 0;
  virtual int draw_torque_limit(const double* lo, const double* hi, hipStream_t s) = 0;
  virtual int set_base_wrench(const void* rows, hipStream_t s) = 0;
  virtual int get_base_wrench(void* out, hipStream_t s) = 0;
  virtual int install_wrench_schedule() = 0;
  // the wrench schedule (nm_wrench.h): the setting and the wrench step index, counted like the push step index
  int wrench_interval = 0, wrench_duration = 0;
  double wrench_max[6] = {};
  uint64_t wrench_step = 0;
  // push perturbations (nm_push.h): the setting and the push step index - full env steps taken, K per K-step launch; physics-only
  // launches and nm_reset leave it alone
  int push_interval = 0;
  double push_max = 0.0;
  uint64_t push_step = 0;
  // randomised reset states (nm_reset_noise.h): the setting; the envs' reset counts are device memory of the env object
  int rnoise_on = 0;
  double rnoise_ranges[2 * nm::kResetRanges] = {};
  // which k_env_step nm_step launches (nm_set_step_variant): 0 = the lean instantiation whenever the launch qualifies (fp32, no per-env
  // rows, nm::lean_config), 1 = always the generic one; and what the last nm_step launched (0 generic, 1 lean)
  int step_variant_mode = 0, step_variant_last = 0;
  virtual int set_reset_counts(const uint32_t* counts_host) = 0;
  virtual int get_reset_counts(uint32_t* counts_host) = 0;
  // per-env rows re-drawn at reset (nm_reset_rows.h): the pools' sizes as the device descriptor holds them (0 = no pool)
  uint32_t rrows_size[nm::kResetRowKinds] = {};
  virtual int set_reset_rows(int kind, const void* rows_dev, uint32_t P, hipStream_t s) = 0;
  virtual int get_reset_rows(int kind, uint32_t* P, void* out_dev, hipStream_t s) = 0;
  virtual int set_reset_row_counts(const uint32_t* counts_host) = 0;
  virtual int get_reset_row_counts(uint32_t* counts_host) = 0;
  virtual int priv_obs(const float* obs, float* out, hipStream_t s) = 0;
  // the sensor model (nm_sensor.h): on or off; its delays, bias, ring, counts and true-obs buffer are device memory of the env object
  bool sensor_on = false;
  virtual int set_sensor(const int32_t* delays, const float* bias, hipStream_t s) = 0;
  virtual int get_sensor(int32_t* on, int32_t* delays_out, float* bias_out, hipStream_t s) = 0;
  virtual int draw_sensor(const int32_t* lo, const int32_t* hi, const double* bias_max, hipStream_t s) = 0;
  virtual int get_sensor_state(float* ring, uint32_t* count) = 0;
  virtual int set_sensor_state(const float* ring, const uint32_t* count) = 0;
  virtual int get_true_obs(float* out, hipStream_t s) = 0;
  virtual int rollout_priv(const nm_rollout_args* r, const nm_rollout_priv_args* pv, int act, hipStream_t s) = 0;
  virtual int rollout_act_priv(const float* flat, const float* rows, uint64_t seed, const int64_t* iter_dev, int step, int act, float* actions, float* logp,
                               float* values, float* mu, float* sigma, float* obs_store, float* row_store, hipStream_t s) = 0;
};

// what puts a K-step launch's nmr::WrenchArgs behind the wrench rows (nm::wrench_args_of), on the launch's stream
__global__ void k_wrench_args(nmr::WrenchArgs* dst, nmr::WrenchArgs w) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = w;
}

// the same for the nm::PrivObsArgs an asymmetric K-step launch gathers its privileged rows with (device memory of the env object)
__global__ void k_priv_args(nm::PrivObsArgs<float>* dst, nm::PrivObsArgs<float> p) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = p;
}

template <class real> struct Env : nm_env {
  nmhost::Tables<real> T;
  nm::Model<real> M;
  nm::Args<real> A;
  std::vector<void*> allocs;
  real* cmd_u_dev = nullptr;
  bool cmd_u_on = false;
  float* timeout_now = nullptr;
  int32_t* ids_dev = nullptr;
  long long* counters_dev = nullptr;
  nm::Model<real>* M_dev = nullptr;
  real* noise_vec_dev = nullptr;
  real* noise_u_dev = nullptr;
  bool noise_on = false, noise_u_on = false;
  uint64_t noise_step = 0;
  real* rec_dev = nullptr;
  int rec_env = -1;
  // the state log of a K-step launch (nm_rollout / nm_play): one row [qpos 25 | qvel 24 | bad-state resets] per step
  real* rec_log = nullptr;
  int rec_log_cap = 0, rec_log_rows = 0;
  unsigned char* rec_done = nullptr;   // [rec_log_cap]: the logged env's reset flag per step of the last nm_play
  bool rec_done_valid = false;
  const real* rec_last = nullptr;      // where the last step's record is: rec_dev after nm_step, the last row of rec_log after a K-step launch
  bool prof_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev;
  size_t prof_used = 0;

  // All device memory of an env comes out of ONE slab (a multiple of 2 MiB): the driver maps large allocations with 2 MiB
  // page-table fragments, so the shared hull tables and the per-env rows stay within a handful of TLB entries instead of one
  // 4 KiB-granular mapping per small hipMalloc.
  char* slab = nullptr;
  size_t slab_size = 0, slab_used = 0;
  int slab_init(size_t bytes) {
    slab_size = (bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
    HIPCHK(hipMalloc((void**)&slab, slab_size));
    HIPCHK(hipMemset(slab, 0, slab_size));
    allocs.push_back(slab);
    return 0;
  }
  template <class X> int dalloc(X** p, size_t n) {
    const size_t bytes = (n * sizeof(X) + 255) & ~(size_t)255;
    if (slab && slab_used + bytes <= slab_size) {
      *p = (X*)(slab + slab_used);
      slab_used += bytes;
      return 0;
    }
    HIPCHK(hipMalloc((void**)p, n * sizeof(X)));
    HIPCHK(hipMemset(*p, 0, n * sizeof(X)));
    allocs.push_back(*p);
    return 0;
  }
  template <class X> int upload(const X** p, const std::vector<X>& v) {
    X* d;
    if (dalloc(&d, v.size())) return 1;
    HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(X), hipMemcpyHostToDevice));
    *p = d;
    return 0;
  }
  int init(const nmhost::EnvConfig& cfg, int n, int dev, uint64_t seed, int64_t off) {
    N = n; device = dev; dtype = sizeof(real) == 8;
    HIPCHK(hipSetDevice(dev));
    T.build();
    memset(&M, 0, sizeof M);
    memset(&A, 0, sizeof A);
    T.fill_scalars(M, cfg);
#ifdef NM_MEASURE   // measurement builds only (results change): cost per solver sweep
    if (const char* e = getenv("NM_MEASURE_PGS_ITERS")) M.pgs_iters = atoi(e);
    if (const char* e = getenv("NM_MEASURE_NOSLIP_ITERS")) M.noslip_iters = atoi(e);
#endif
    if (slab_init((T.hullv.size() + T.hullnv.size()) * sizeof(real) + (size_t)n * 300 * sizeof(real) + (size_t)n * 64 + (1u << 20))) return 1;
    if (upload(&M.hullv, T.hullv) || upload(&M.hullnv, T.hullnv)) return 1;
    A.N = N; A.seed = seed; A.env_offset = off; A.nsub = cfg.decimation;
    {
      int nx = 0;     // the dispatcher's round-robin width: 8 on an MI355X in SPX mode; anything else switches the remap off
      if (hipDeviceGetAttribute(&nx, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess) { (void)hipGetLastError(); nx = 0; }
      A.nxcd = nx;
    }
    size_t n_ = (size_t)N;
    if (dalloc(&A.qpos, n_ * 25) || dalloc(&A.qvel, n_ * 24) || dalloc(&A.qwarm, n_ * 24) || dalloc(&A.dofpos, n_ * 18) ||
        dalloc(&A.dofvel, n_ * 18) || dalloc(&A.act, n_ * 18) || dalloc(&A.cmd, n_ * 3) || dalloc(&A.epsum, n_ * nm::kNREW) || dalloc(&A.feetair, n_ * nm::kNLEG) || dalloc(&A.feetflags, n_) ||
        dalloc(&A.rngctr, n_) || dalloc(&A.hullcache, n_ * 8) || dalloc(&A.stat_sum, nm::kNREW) || dalloc(&A.stat_cnt, 4) || dalloc(&cmd_u_dev, n_ * 4) ||
        dalloc(&timeout_now, n_) || dalloc(&ids_dev, n_) || dalloc(&counters_dev, 4) || dalloc(&A.wave_done, ((n_ + nm::kTicketGroup - 1) / nm::kTicketGroup + 2) * nm::kTicketStride) || dalloc(&A.nto, 1) || dalloc(&A.to_list, n_) || dalloc(&A.nprev, 1) || dalloc(&A.to_prev, n_) || dalloc(&A.to_owner, 1))
      return 1;
    {
      nm::ModelBlock<real>* mb = nullptr;      // the struct and its padding (zeros) up to the step kernel's whole copy rounds
      if (dalloc(&mb, 1)) return 1;
      M_dev = &mb->m;
    }
    HIPCHK(hipMemcpy(M_dev, &M, sizeof M, hipMemcpyHostToDevice));
    std::vector<real> q0(n_ * 25);
    for (size_t i = 0; i < n_; i++)
      for (int k = 0; k < 25; k++) q0[i * 25 + k] = T.qpos0[k];
    HIPCHK(hipMemcpy(A.qpos, q0.data(), q0.size() * sizeof(real), hipMemcpyHostToDevice));
    return 0;
  }
  ~Env() override {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();   // kernels of this env may still be in flight on the caller's stream
    for (auto& ev : prof_ev) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (void* p : allocs) (void)hipFree(p);
  }
  int finalize(float* ep_stats, float* time_outs, hipStream_t s) {
    hipLaunchKernelGGL(k_finalize<real>, dim3(1), dim3(1024), 0, s, N, A.stat_sum, A.stat_cnt, ep_stats, timeout_now, time_outs, M.ep_len_s,
                       counters_dev);
    HIPCHK(hipGetLastError());
    return 0;
  }
  int reset(const int32_t* ids, int n, int64_t* eplen, float* ep_stats, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!eplen) return fail("nm_reset: episode_length_dev is NULL");
    const int32_t* idp = nullptr;
    if (ids) {
      if (n <= 0) return 0;  // reset_idx returns early on an empty id list (env.py:344)
      for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= N) return fail("nm_reset: env id out of range");
      HIPCHK(hipMemcpyAsync(ids_dev, ids, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));   // the caller's host array may go away as soon as we return
      idp = ids_dev;
    } else n = N;
    nm::Args<real> a = A;
    a.eplen = eplen;
    a.cmd_u = cmd_u_on ? cmd_u_dev : nullptr;
    hipLaunchKernelGGL(k_reset<real>, dim3((n + 255) / 256), dim3(256), 0, s, M, a, idp, n);
    HIPCHK(hipGetLastError());
    if (rnoise_on && launch_reset_noise(nullptr, idp, n, s)) return 1;     // the same envs' reset draw (nm_reset_noise.h)
    if (rrows_any() && launch_reset_rows(nullptr, idp, n, s)) return 1;    // and the re-draw of their per-env rows (nm_reset_rows.h)
    if (sensor.count) HIPCHK(nm_launch_sensor_clear(sensor.count, idp, n, s));      // a reading never reaches behind a reset (nm_sensor.h)
    return finalize(ep_stats, nullptr, s);
  }
  int step(const float* actions, int64_t* eplen, float* obs, float* rew, int64_t* done, float* time_outs, float* ep_stats, int physics_only,
           hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!actions) return fail("nm_step: actions_dev is NULL");
    if (!physics_only && (!eplen || !obs || !rew || !done)) return fail("nm_step: NULL output pointer");
    nm::Args<real> a = A;
    a.actions = actions; a.eplen = eplen; a.obs = obs; a.rew = rew; a.done = done; a.timeout_now = timeout_now;
    a.cmd_u = cmd_u_on ? cmd_u_dev : nullptr;
    a.physics_only = physics_only;
    a.ep_stats = ep_stats; a.time_outs = time_outs; a.counters = counters_dev;
    if (!physics_only && sensor_on) a.obs = sensor.true_obs;      // the sensor model (nm_sensor.h): the step files the true row, k_sensor below the caller's
    if (!physics_only) {
      a.noise_vec = noise_on ? noise_vec_dev : nullptr;
      a.noise_u = noise_on && noise_u_on ? noise_u_dev : nullptr;
      a.noise_step = noise_step++;
      a.rec = rec_env >= 0 ? rec_dev : nullptr;
      a.rec_env = rec_env;
      if (rec_env >= 0) rec_last = rec_dev;
      const uint64_t ps = push_step++;
      if (nm::push_due(push_interval, ps)) {   // a launch of its own on due steps only; every other step launches nothing extra
        hipLaunchKernelGGL(nm::k_push<real>, dim3((2 * N + 255) / 256), dim3(256), 0, s, A.qvel, N, A.seed, A.env_offset,
                           nm::push_counter(push_interval, ps), (real)push_max);
        HIPCHK(hipGetLastError());
      }
      const uint64_t ws = wrench_step++;
      if (const int due = nm::wrench_due(wrench_interval, wrench_duration, ws))      // as the push: a launch of its own on the steps that open or close a window
        if (launch_wrench(nm::wrench_window(wrench_interval, ws), due == 1, s)) return 1;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (prof_on) {  // HIP events on the launch stream around the dominant kernel only (bench.py's roofline leg)
      if (prof_used == prof_ev.size()) {
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        prof_ev.push_back({e0, e1});
      }
      e0 = prof_ev[prof_used].first; e1 = prof_ev[prof_used].second;
      prof_used++;
      HIPCHK(hipEventRecord(e0, s));
    }
    constexpr int G = sizeof(real) == 8 ? 1 : NM_ENVS_PER_WAVE;  // the fp64 verification build keeps one env per wave (LDS)
    constexpr int W = sizeof(real) == 8 ? 1 : kWG;
    bool lean = false;
#ifndef NM_MEASURE   // (the measurement build holds the generic kernels only)
    if constexpr (sizeof(real) == 4 && G == 2)
      lean = step_variant_mode == 0 && rows.level(physics_only) == 0 && nm::lean_config(M, a);
#endif
    step_variant_last = lean ? 1 : 0;
    if (lean) {
#ifndef NM_MEASURE
      if constexpr (sizeof(real) == 4 && G == 2) HIPCHK(nm_launch_step_lean(N, s, (const nm::Model<float>*)M_dev, a));
#endif
    } else {
      nmrows::with_level(rows.level(physics_only), [&](auto L) {
        hipLaunchKernelGGL((k_env_step<real, G, decltype(L)::value>), dim3((N + G * W - 1) / (G * W)), dim3(64 * W), 0, s, (const nm::Model<real>*)M_dev, a);
      });
      HIPCHK(hipGetLastError());
    }
    if (prof_on) HIPCHK(hipEventRecord(e1, s));
    // randomised reset states: the draw of the envs this step reset, decided on the device from done[] (nm_reset_noise.h)
    if (!physics_only && rnoise_on && launch_reset_noise(done, nullptr, N, s)) return 1;
    // per-env rows re-drawn at reset: the same decision on the device, for the kinds that have a pool (nm_reset_rows.h)
    if (!physics_only && rrows_any() && launch_reset_rows(done, nullptr, N, s)) return 1;
    // the sensor model: the true row -> ring, count and the sensed row in the caller's buffer (nm_sensor.h)
    if (!physics_only && sensor_on) HIPCHK(nm_launch_sensor(sensor, done, obs, N, s));
    return 0;
  }
  int d2h(const real* dev, double* host, size_t n) {
    if (!host) return 0;
    std::vector<real> tmp(n);
    HIPCHK(hipMemcpy(tmp.data(), dev, n * sizeof(real), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) host[i] = (double)tmp[i];
    return 0;
  }
  int h2d(real* dev, const double* host, size_t n) {
    if (!host) return 0;
    std::vector<real> tmp(n);
    for (size_t i = 0; i < n; i++) tmp[i] = (real)host[i];
    HIPCHK(hipMemcpy(dev, tmp.data(), n * sizeof(real), hipMemcpyHostToDevice));
    return 0;
  }
  int get_state(double* qpos, double* qvel, double* qw) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    return d2h(A.qpos, qpos, (size_t)N * 25) || d2h(A.qvel, qvel, (size_t)N * 24) || d2h(A.qwarm, qw, (size_t)N * 24);
  }
  int set_state(const double* qpos, const double* qvel, const double* qw) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    return h2d(A.qpos, qpos, (size_t)N * 25) || h2d(A.qvel, qvel, (size_t)N * 24) || h2d(A.qwarm, qw, (size_t)N * 24);
  }
  int get_buffers(double* dp, double* dv, double* act, double* cmd, double* es) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    return d2h(A.dofpos, dp, (size_t)N * 18) || d2h(A.dofvel, dv, (size_t)N * 18) || d2h(A.act, act, (size_t)N * 18) ||
           d2h(A.cmd, cmd, (size_t)N * 3) || d2h(A.epsum, es, (size_t)N * nm::kNREW);
  }
  int set_buffers(const double* dp, const double* dv, const double* act, const double* cmd, const double* es) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    return h2d(A.dofpos, dp, (size_t)N * 18) || h2d(A.dofvel, dv, (size_t)N * 18) || h2d(A.act, act, (size_t)N * 18) ||
           h2d(A.cmd, cmd, (size_t)N * 3) || h2d(A.epsum, es, (size_t)N * nm::kNREW);
  }
  int get_feet(double* air, unsigned char* last, unsigned char* filt) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    if (d2h(A.feetair, air, (size_t)N * 6)) return 1;
    std::vector<int> fl(N);
    HIPCHK(hipMemcpy(fl.data(), A.feetflags, sizeof(int) * N, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; i++)
      for (int k = 0; k < 6; k++) {
        if (last) last[i * 6 + k] = (fl[i] >> k) & 1;
        if (filt) filt[i * 6 + k] = (fl[i] >> (6 + k)) & 1;
      }
    return 0;
  }
  int set_feet(const double* air, const unsigned char* last, const unsigned char* filt) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    if (h2d(A.feetair, air, (size_t)N * 6)) return 1;
    if (last || filt) {
      std::vector<int> fl(N);
      HIPCHK(hipMemcpy(fl.data(), A.feetflags, sizeof(int) * N, hipMemcpyDeviceToHost));
      for (int i = 0; i < N; i++)
        for (int k = 0; k < 6; k++) {
          if (last) fl[i] = (fl[i] & ~(1 << k)) | ((last[i * 6 + k] ? 1 : 0) << k);
          if (filt) fl[i] = (fl[i] & ~(1 << (6 + k))) | ((filt[i * 6 + k] ? 1 : 0) << (6 + k));
        }
      HIPCHK(hipMemcpy(A.feetflags, fl.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    }
    return 0;
  }
  int set_cmd_u(const double* u) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    cmd_u_on = u != nullptr;
    return h2d(cmd_u_dev, u, (size_t)N * 4);
  }
  int counters(int64_t* out) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    long long c[3];
    HIPCHK(hipMemcpy(c, counters_dev, sizeof c, hipMemcpyDeviceToHost));
    std::vector<int> hc((size_t)N * 8);
    HIPCHK(hipMemcpy(hc.data(), A.hullcache, hc.size() * sizeof(int), hipMemcpyDeviceToHost));
    long long fb = 0;
    for (int i = 0; i < N; i++) fb += hc[(size_t)i * 8 + 7];    // per-env running counts (wrap after 2^31 fallbacks of one env)
    out[0] = c[0]; out[1] = c[1]; out[2] = fb;
    return 0;
  }
  int set_noise(const double* vec) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    noise_on = vec != nullptr;
    if (vec && !noise_vec_dev && dalloc(&noise_vec_dev, NM_NUM_OBS)) return 1;
    return vec ? h2d(noise_vec_dev, vec, NM_NUM_OBS) : 0;
  }
  int set_noise_u(const double* u) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    noise_u_on = u != nullptr;
    if (u && !noise_u_dev && dalloc(&noise_u_dev, (size_t)N * NM_NUM_OBS)) return 1;
    return u ? h2d(noise_u_dev, u, (size_t)N * NM_NUM_OBS) : 0;
  }
  int set_record(int idx) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    if (idx >= N) return fail("nm_set_state_record: env index out of range");
    if (idx >= 0 && !rec_dev && dalloc(&rec_dev, 64)) return 1;
    rec_env = idx < 0 ? -1 : idx;
    rec_last = nullptr; rec_log_rows = 0; rec_done_valid = false;
    return 0;
  }
  int get_record(double* qpos, double* qvel, int32_t* nbad) override {
    HIPCHK(hipSetDevice(device));
    if (rec_env < 0) return fail("nm_get_state_record: recording is off (nm_set_state_record)");
    if (!rec_last) return fail("nm_get_state_record: no step has been recorded yet");
    HIPCHK(hipDeviceSynchronize());
    double tmp[50];
    if (d2h(rec_last, tmp, 50)) return 1;
    if (qpos) for (int i = 0; i < 25; i++) qpos[i] = tmp[i];
    if (qvel) for (int i = 0; i < 24; i++) qvel[i] = tmp[25 + i];
    if (nbad) *nbad = (int32_t)tmp[49];
    return 0;
  }

  int get_log(int first, int count, double* rows) override {
    HIPCHK(hipSetDevice(device));
    if (rec_env < 0) return fail("nm_get_state_log: recording is off (nm_set_state_record)");
    if (first < 0 || count < 0 || first + count > rec_log_rows) return fail("nm_get_state_log: rows outside the last K-step launch");
    if (count == 0) return 0;
    if (!rows) return fail("nm_get_state_log: rows_host is NULL");
    HIPCHK(hipDeviceSynchronize());
    return d2h(rec_log + (size_t)first * nmr::kRecRow, rows, (size_t)count * nmr::kRecRow);
  }
  int get_log_dones(int first, int count, unsigned char* dones) override {
    HIPCHK(hipSetDevice(device));
    if (rec_env < 0) return fail("nm_get_state_log_dones: recording is off (nm_set_state_record)");
    if (!rec_done_valid) return fail("nm_get_state_log_dones: the last K-step launch was not nm_play (nm_rollout files the flags in its dones rows)");
    if (first < 0 || count < 0 || first + count > rec_log_rows) return fail("nm_get_state_log_dones: steps outside the last K-step launch");
    if (count == 0) return 0;
    if (!dones) return fail("nm_get_state_log_dones: dones_host is NULL");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dones, rec_done + first, (size_t)count, hipMemcpyDeviceToHost));
    return 0;
  }
  // the log rows of a launch of K steps (null: recording is off); sized with the per-step accumulators (roll_cap)
  int log_rows(int K, real** out) {
    *out = nullptr;
    if (rec_env < 0) return 0;
    if (K > rec_log_cap) {
      if (dalloc(&rec_log, (size_t)roll_cap * nmr::kRecRow) || dalloc(&rec_done, (size_t)roll_cap)) return 1;
      rec_log_cap = roll_cap;
    }
    rec_log_rows = K;
    rec_done_valid = false;
    rec_last = rec_log + (size_t)(K - 1) * nmr::kRecRow;
    *out = rec_log;
    return 0;
  }
  int roll_reserve(int K) {   // per-step accumulators (zero: the slab and hipMalloc'ed blocks are cleared, k_rollout_clear keeps them so)
    if (K > roll_cap) {
      const int cap = (K + 127) & ~127;
      if (dalloc(&roll_sum, (size_t)cap * nm::kNREW) || dalloc(&roll_cnt, (size_t)cap * 4)) return 1;
      if (!roll_to && dalloc(&roll_to, (size_t)N)) return 1;
      roll_cap = cap;
    }
    return 0;
  }
  // ---- K-step rollout with the policy in the wave (nm_rollout; fp32 two-env waves and the reference's network shape only)
  float *roll_wp = nullptr, *roll_bp = nullptr;
  real* roll_sum = nullptr;
  int *roll_cnt = nullptr, *roll_to = nullptr;
  int roll_cap = 0;
  typedef nmr::RefShape RS;
  int roll_pack(const float* flat, hipStream_t s) {
    if (!roll_wp && (dalloc(&roll_wp, (size_t)RS::nfrag() * 256) || dalloc(&roll_bp, (size_t)RS::nbias()))) return 1;
    if (nmr::launch_pack(flat, roll_wp, roll_bp, s)) return fail("nm_rollout: packing the policy failed to launch");
    return 0;
  }
  int rollout_act(const float* flat, const float* obs, uint64_t seed, const int64_t* iter_dev, int step, int act, float* actions, float* logp, float* values,
                  float* mu, float* sigma, float* obs_store, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!flat || !obs || !iter_dev || !actions || !logp || !values || !mu || !sigma) return fail("nm_rollout_act: NULL pointer");
    if (roll_pack(flat, s)) return 1;
    nmr::ActOut o{actions, logp, values, mu, sigma, obs_store};
    if (nmr::launch_act(roll_wp, roll_bp, flat + RS::stdoff(), obs, N, seed, iter_dev, step, o, act, s)) return fail("nm_rollout_act: launch failed");
    return 0;
  }
  // what nm_rollout and nm_play check alike: the range of `steps` and the episode-statistics arguments (`who`: the entry point's name)
  int kstep_check(const char* who, int K, const char* hint, int n_ep, const int* ep_idx, const float* ep_acc, const float* ep_stats) {
    if (K < 1 || K > 4096) return fail(std::string(who) + ": steps must be in 1..4096" + hint);
    if (n_ep < 0 || n_ep > nm::kNREW || (n_ep > 0 && (!ep_idx || !ep_acc || !ep_stats))) return fail(std::string(who) + ": bad episode-statistics arguments");
    return 0;
  }
  // the nm::Args of a K-step launch (the kernel sets stat_sum / stat_cnt / noise_step / rec per step; extras are closed by k_rollout_tail);
  // advances noise_step by K
  nm::Args<real> kstep_args(int K, const float* actions, int64_t* eplen, float* obs, float* rew, int64_t* done, real* log) {
    nm::Args<real> a = A;
    a.actions = actions; a.eplen = eplen; a.obs = obs; a.rew = rew; a.done = done; a.timeout_now = timeout_now;
    a.cmd_u = cmd_u_on ? cmd_u_dev : nullptr;
    a.physics_only = 0;
    a.ep_stats = nullptr; a.time_outs = nullptr; a.counters = counters_dev;
    a.to_list = nullptr;
    a.noise_vec = noise_on ? noise_vec_dev : nullptr;
    a.noise_u = noise_on && noise_u_on ? noise_u_dev : nullptr;
    a.noise_step = noise_step;
    noise_step += (uint64_t)K;
    a.rec = log; a.rec_env = log ? rec_env : -1; a.dbg = nullptr; a.ret_acc = nullptr;    // (rec: row t, set by the kernel before every step)
    return a;
  }
  // ---- randomised reset states (nm_reset_noise.h): the reset counts, allocated (zeroed) at first use
  uint32_t* rnoise_count = nullptr;
  int rnoise_reserve() {
    if (rnoise_count) return 0;
    if (dalloc(&rnoise_count, (size_t)N)) return 1;
    HIPCHK(hipMemset(rnoise_count, 0, (size_t)N * sizeof(uint32_t)));
    HIPCHK(hipDeviceSynchronize());
    return 0;
  }
  int set_reset_counts(const uint32_t* counts_host) override {
    HIPCHK(hipSetDevice(device));
    if (rnoise_reserve()) return 1;
    if (!counts_host) return 0;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(rnoise_count, counts_host, (size_t)N * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
  }
  int get_reset_counts(uint32_t* counts_host) override {
    if (!counts_host) return 0;
    if (!rnoise_count) { memset(counts_host, 0, (size_t)N * sizeof(uint32_t)); return 0; }
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(counts_host, rnoise_count, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
  }
  const real* qpos0_dev() const { return reinterpret_cast<const real*>(reinterpret_cast<const char*>(M_dev) + offsetof(nm::Model<real>, qpos0)); }
  // the reset draw behind a step (done: the step's reset flags) or behind k_reset (done = null: the n listed envs); on the same stream
  int launch_reset_noise(const int64_t* done, const int32_t* ids, int n, hipStream_t s) {
    hipLaunchKernelGGL(nm::k_reset_noise<real>, dim3((unsigned)(((size_t)n * 64 + 255) / 256)), dim3(256), 0, s, A.qpos, A.qvel, rnoise_count, qpos0_dev(),
                       nm::reset_noise_params<real>(rnoise_ranges), A.seed, A.env_offset, done, ids, n);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // the reset-noise arguments of a K-step launch
  nmr::ResetNoiseArgs kstep_rnoise() {
    nmr::ResetNoiseArgs r{};
    if constexpr (sizeof(real) == 4) {
      if (rnoise_on) { r.on = 1; r.p = nm::reset_noise_params<float>(rnoise_ranges); r.qpos0 = qpos0_dev(); r.count = rnoise_count; }
    }
    return r;
  }
  // ---- per-env rows re-drawn at reset (nm_reset_rows.h): the pools are copies in device memory of this object, the descriptor the
  // kernels read lies in device memory too and is rewritten stream-ordered after synchronising; the reset-row counts are allocated
  // (zeroed) at first use
  nm::ResetRowsDesc* rrows_desc_dev = nullptr;
  nm::ResetRowsDesc rrows_desc = {};
  uint32_t rrows_cap[nm::kResetRowKinds] = {};      // rows the kind's device buffer holds
  uint32_t* rrows_count = nullptr;
  bool rrows_any() const {
    for (int k = 0; k < nm::kResetRowKinds; k++) if (rrows_size[k]) return true;
    return false;
  }
  int rrows_reserve() {
    if (rrows_count) return 0;
    if (dalloc(&rrows_count, (size_t)N) || dalloc(&rrows_desc_dev, 1)) return 1;
    HIPCHK(hipMemset(rrows_count, 0, (size_t)N * sizeof(uint32_t)));
    HIPCHK(hipMemset(rrows_desc_dev, 0, sizeof(nm::ResetRowsDesc)));
    HIPCHK(hipDeviceSynchronize());
    return 0;
  }
  static size_t rrows_word(int kind) { return kind == nmrows::kLat ? sizeof(int) : sizeof(real); }
  // the descriptor as the host holds it -> device, behind everything `s` carries (a launch in flight may be reading the old one)
  int rrows_publish(hipStream_t s) {
    for (int k = 0; k < nm::kResetRowKinds; k++) rrows_desc.size[k] = rrows_size[k];
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpyAsync(rrows_desc_dev, &rrows_desc, sizeof rrows_desc, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
  }
  // what switching a kind off does to its pool (nm_set_* with null): dropped; the buffer stays for the next pool
  int rrows_drop(int kind, hipStream_t s) {
    if (!rrows_size[kind]) return 0;
    rrows_size[kind] = 0;
    return rrows_publish(s);
  }
  int set_reset_rows(int kind, const void* rows_in, uint32_t P, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!rows_in) return rrows_drop(kind, s);       // the kind stays on or off as it is, its rows keep what they hold
    // the pool is judged on the host before anything of the env changes
    const size_t bytes = (size_t)P * nmrows::kind_width(kind) * rrows_word(kind);
    std::vector<char> h(bytes);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(h.data(), rows_in, bytes, hipMemcpyDeviceToHost));
    const std::string why = nmrows::pool_rows_fault<real>(kind, h.data(), (int)P, A.nsub);
    if (!why.empty()) return fail("nm_set_reset_rows: " + why);
    if (rows_alloc(s) || rrows_reserve()) return 1;
    if (P > rrows_cap[kind]) {       // a buffer of its own per kind; an outgrown one stays allocated until the env goes (a launch may hold it)
      char* buf = nullptr;
      HIPCHK(hipMalloc((void**)&buf, bytes));
      allocs.push_back(buf);
      rrows_desc.pool[kind] = (uint64_t)(uintptr_t)buf;
      rrows_cap[kind] = P;
    }
    HIPCHK(hipMemcpyAsync((void*)(uintptr_t)rrows_desc.pool[kind], rows_in, bytes, hipMemcpyDeviceToDevice, s));
    rrows_size[kind] = P;
    if (rrows_publish(s)) return 1;
    return rows_turn((nmrows::Kind)kind, true);      // the current rows stay until each env's next reset
  }
  int get_reset_rows(int kind, uint32_t* P, void* out, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (P) *P = rrows_size[kind];
    if (out && rrows_size[kind])
      HIPCHK(hipMemcpyAsync(out, (const void*)(uintptr_t)rrows_desc.pool[kind], (size_t)rrows_size[kind] * nmrows::kind_width(kind) * rrows_word(kind),
                            hipMemcpyDeviceToDevice, s));
    return 0;
  }
  int set_reset_row_counts(const uint32_t* counts_host) override {
    HIPCHK(hipSetDevice(device));
    if (!counts_host) return fail("nm_set_reset_row_counts: counts_host is NULL");
    if (rrows_reserve()) return 1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(rrows_count, counts_host, (size_t)N * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
  }
  int get_reset_row_counts(uint32_t* counts_host) override {
    if (!counts_host) return 0;
    if (!rrows_count) { memset(counts_host, 0, (size_t)N * sizeof(uint32_t)); return 0; }
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(counts_host, rrows_count, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
  }
  // the re-draw behind a step (done: the step's reset flags) or behind k_reset (done = null: the n listed envs); on the same stream
  int launch_reset_rows(const int64_t* done, const int32_t* ids, int n, hipStream_t s) {
    hipLaunchKernelGGL(nm::k_reset_rows<real>, dim3((unsigned)(((size_t)n * 64 + 255) / 256)), dim3(256), 0, s, A, (const nm::ResetRowsDesc*)rrows_desc_dev,
                       rrows_count, done, ids, n);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // ---- the sensor model (nm_sensor.h): delays, bias, ring, counts and the true-obs buffer, allocated (zeroed) at first use; `sensor` is the
  // descriptor as the host holds it (k_sensor takes it by value), sensor_desc_dev the copy the K-step kernels read, rewritten
  // stream-ordered in front of a launch whenever the host's differs from what was last published (only `out` ever does)
  nm::SensorDesc sensor = {};
  nm::SensorDesc* sensor_desc_dev = nullptr;
  float* sensor_out_published = nullptr;
  bool sensor_published = false;
  int sensor_reserve() {
    if (sensor.count) return 0;
    const size_t n_ = (size_t)N;
    int32_t* dl = nullptr; float* bs = nullptr;
    if (dalloc(&dl, n_ * nm::kSensorGroups) || dalloc(&bs, n_ * nm::kNOBS) || dalloc(&sensor.ring, n_ * nm::kSensorSlots * nm::kNOBS) ||
        dalloc(&sensor.true_obs, n_ * nm::kNOBS) || dalloc(&sensor_desc_dev, 1) || dalloc(&sensor.count, n_))
      return 1;
    sensor.delay = dl; sensor.bias = bs;
    sensor.clip_obs = (float)M.clip_obs;
    HIPCHK(hipMemset(dl, 0, n_ * nm::kSensorGroups * sizeof(int32_t)));
    HIPCHK(hipMemset(bs, 0, n_ * nm::kNOBS * sizeof(float)));
    HIPCHK(hipMemset(sensor.ring, 0, n_ * nm::kSensorSlots * nm::kNOBS * sizeof(float)));
    HIPCHK(hipMemset(sensor.true_obs, 0, n_ * nm::kNOBS * sizeof(float)));
    HIPCHK(hipMemset(sensor.count, 0, n_ * sizeof(uint32_t)));
    HIPCHK(hipDeviceSynchronize());
    return 0;
  }
  // the sensor arguments of a K-step launch; out: the env's observation buffer of this launch
  int kstep_sensor(nmr::SensorArgs& a, float* out, hipStream_t s) {
    a = nmr::SensorArgs{};
    if (!sensor_on) return 0;
    sensor.out = out;
    if (!sensor_published || sensor_out_published != out) {
      HIPCHK(nm_launch_sensor_desc(sensor_desc_dev, sensor, s));
      sensor_published = true; sensor_out_published = out;
    }
    a.desc = sensor_desc_dev; a.on = 1;
    return 0;
  }
  int set_sensor(const int32_t* delays, const float* bias, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!delays && !bias) { sensor_on = false; return 0; }      // off; nothing is freed, the model and its history keep what they hold
    // the model is judged on the host before anything of the env changes
    const size_t n_ = (size_t)N;
    std::vector<int32_t> hd(delays ? n_ * nm::kSensorGroups : 0);
    std::vector<float> hb(bias ? n_ * nm::kNOBS : 0);
    HIPCHK(hipStreamSynchronize(s));
    if (delays) HIPCHK(hipMemcpy(hd.data(), delays, hd.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (bias) HIPCHK(hipMemcpy(hb.data(), bias, hb.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < hd.size(); i++)
      if (hd[i] < 0 || hd[i] > nm::kSensorMaxDelay)
        return fail("nm_set_sensor: env " + std::to_string(i / nm::kSensorGroups) + " column " + std::to_string(i % nm::kSensorGroups) + " (" +
                    (i % nm::kSensorGroups ? "joint" : "imu") + " delay): " + std::to_string(hd[i]) + " outside 0.." + std::to_string(nm::kSensorMaxDelay) + " env steps");
    for (size_t i = 0; i < hb.size(); i++) {
      const int c = (int)(i % nm::kNOBS);
      if (!std::isfinite(hb[i])) return fail("nm_set_sensor: env " + std::to_string(i / nm::kNOBS) + " column " + std::to_string(c) + ": the bias is not finite");
      if (nm::sensor_col_group(c) < 0 && hb[i] != 0.0f)
        return fail("nm_set_sensor: env " + std::to_string(i / nm::kNOBS) + " column " + std::to_string(c) + ": a bias in a pass-through column (commands 9..11, actions 48..65)");
    }
    if (sensor_reserve()) return 1;
    if (delays) HIPCHK(hipMemcpyAsync((void*)sensor.delay, delays, hd.size() * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    else HIPCHK(hipMemsetAsync((void*)sensor.delay, 0, n_ * nm::kSensorGroups * sizeof(int32_t), s));
    if (bias) HIPCHK(hipMemcpyAsync((void*)sensor.bias, bias, hb.size() * sizeof(float), hipMemcpyDeviceToDevice, s));
    else HIPCHK(hipMemsetAsync((void*)sensor.bias, 0, n_ * nm::kNOBS * sizeof(float), s));
    HIPCHK(hipMemsetAsync(sensor.count, 0, n_ * sizeof(uint32_t), s));      // the history is cleared
    sensor_on = true;
    return 0;
  }
  int get_sensor(int32_t* on, int32_t* delays_out, float* bias_out, hipStream_t s) override {
    if (on) *on = sensor_on ? 1 : 0;
    const bool have = sensor_on && sensor.count;
    return words_out(delays_out, have ? sensor.delay : nullptr, (size_t)N * nm::kSensorGroups, s) ||
           words_out(bias_out, have ? sensor.bias : nullptr, (size_t)N * nm::kNOBS, s);
  }
  int draw_sensor(const int32_t* lo, const int32_t* hi, const double* bias_max, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (sensor_reserve()) return 1;
    nm_sensor_draw_args a;
    for (int g = 0; g < nm::kSensorGroups; g++) { a.lo[g] = lo[g]; a.hi[g] = hi[g]; }
    for (int k = 0; k < nm::kSensorKinds; k++) a.bmax[k] = (float)bias_max[k];
    HIPCHK(nm_launch_sensor_draw((int32_t*)sensor.delay, (float*)sensor.bias, N, A.seed, A.env_offset, a, s));
    HIPCHK(hipMemsetAsync(sensor.count, 0, (size_t)N * sizeof(uint32_t), s));
    sensor_on = true;
    return 0;
  }
  int get_sensor_state(float* ring, uint32_t* count) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    const size_t n_ = (size_t)N, rw = n_ * nm::kSensorSlots * nm::kNOBS;
    if (!sensor.count) {      // never allocated: zero, as at construction
      if (ring) memset(ring, 0, rw * sizeof(float));
      if (count) memset(count, 0, n_ * sizeof(uint32_t));
      return 0;
    }
    if (ring) HIPCHK(hipMemcpy(ring, sensor.ring, rw * sizeof(float), hipMemcpyDeviceToHost));
    if (count) HIPCHK(hipMemcpy(count, sensor.count, n_ * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
  }
  int set_sensor_state(const float* ring, const uint32_t* count) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    if (!ring || !count) return fail("nm_set_sensor_state: the state is NULL");
    if (sensor_reserve()) return 1;
    const size_t n_ = (size_t)N;
    HIPCHK(hipMemcpy(sensor.ring, ring, n_ * nm::kSensorSlots * nm::kNOBS * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(sensor.count, count, n_ * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
  }
  int get_true_obs(float* out, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!out) return fail("nm_get_true_obs: out_dev is NULL");
    if (!sensor_on) return fail("nm_get_true_obs: the sensor model is off (the observation the step returned is the true one)");
    HIPCHK(hipMemcpyAsync(out, sensor.true_obs, (size_t)N * nm::kNOBS * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
  }
  // ---- the privileged critic row (nm_priv_obs.h): obs [N, 66] and what the block and the state hold now -> out [N, 89], on `s` behind
  // whatever it carries; the regions are null while the block does not exist (the kernel then writes the default rows' values)
  int priv_obs(const float* obs, float* out, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!obs || !out) return fail("nm_privileged_obs: NULL pointer");
    nm::PrivObsArgs<real> p = priv_args();
    p.obs = obs; p.out = out;
    HIPCHK(nm_launch_priv_obs(p, s));
    return 0;
  }
  // the regions and model constants of the privileged row, as they are now
  nm::PrivObsArgs<real> priv_args() {
    nm::PrivObsArgs<real> p{};
    if (envp_dev) {
      p.fric = nmrows::fric_rows(envp_dev, N); p.body = nmrows::body_rows(envp_dev, N); p.delay = nmrows::delays(envp_dev, N);
      p.grav = nmrows::grav_rows(envp_dev, N); p.servo = nmrows::servo_rows(envp_dev, N); p.torque = nmrows::torque_rows(envp_dev, N);
      p.wrench = nmrows::wrench_rows(envp_dev, N);
    }
    p.qpos = A.qpos; p.N = N; p.nxcd = A.nxcd; p.nsub = A.nsub;
    p.mu = (double)M.mu; p.p_gain = (double)M.p_gain; p.kv = (double)M.kv; p.base_mass = (double)M.basec[nm::BP_MASS];
    for (int j = 0; j < 3; j++) p.base_ipos[j] = (double)M.basec[nm::BP_IPOS + j];
    p.grav0 = (double)M.grav; p.weight = (double)M.total_mass * (double)M.grav;
    return p;
  }
  // the reset-rows arguments of a K-step launch
  nmr::ResetRowsArgs kstep_rrows() {
    nmr::ResetRowsArgs r{};
    if (rrows_any()) { r.on = 1; r.desc = rrows_desc_dev; r.count = rrows_count; }
    return r;
  }
  // the push arguments of a K-step launch (nmr::PushArgs says how the step index travels); advances push_step by K
  nmr::PushArgs kstep_push(int K) {
    nmr::PushArgs p{};
    if (push_interval > 0) {
      p.interval = push_interval;
      p.phase = (uint32_t)(push_step % (uint64_t)push_interval);
      p.ctr0 = nm::push_counter(push_interval, push_step);
      p.past0 = push_step > 0;
      p.maxv = (float)push_max;
    }
    push_step += (uint64_t)K;
    return p;
  }
  // the rows of the wrench schedule on the device: the draw of window q for every env, or zero (nm::k_wrench)
  int launch_wrench(uint32_t q, bool draw, hipStream_t s) {
    nm::WrenchMax<real> mx;
    for (int k = 0; k < 6; k++) mx.v[k] = (real)wrench_max[k];
    hipLaunchKernelGGL(nm::k_wrench<real>, dim3((6 * N + 255) / 256), dim3(256), 0, s, nmrows::wrench_rows(envp_dev, N), N, A.seed, A.env_offset, q, draw ? 1 : 0, mx);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // the wrench arguments of a K-step launch (nmr::WrenchArgs says how the step index travels), written behind the wrench rows on the
  // launch's stream while the kind is on (the level-7 kernels alone read them); advances wrench_step by K
  int kstep_wrench(int K, hipStream_t s) {
    nmr::WrenchArgs w{};
    if (wrench_interval > 0) {
      w.interval = wrench_interval; w.duration = wrench_duration;
      w.phase = (uint32_t)(wrench_step % (uint64_t)wrench_interval);
      w.q0 = nm::wrench_window(wrench_interval, wrench_step);
      w.past0 = wrench_step >= (uint64_t)wrench_interval;
      for (int k = 0; k < 6; k++) w.maxv[k] = (float)wrench_max[k];
    }
    wrench_step += (uint64_t)K;
    if (!rows.on[nmrows::kWrench]) return 0;
    hipLaunchKernelGGL(k_wrench_args, dim3(1), dim3(64), 0, s, static_cast<nmr::WrenchArgs*>(nmrows::wrench_args(envp_dev, N)), w);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // what closes a K-step launch (k_rollout_tail), from the entry point's arguments `r`; the rollout alone bootstraps time-outs
  template <class R> nmr::TailArgs kstep_tail(const R* r, int K, float gamma = -1.0f, const float* s_values = nullptr, float* s_rewards = nullptr) {
    return {N, K, roll_sum, roll_cnt, roll_to, r->ep_stats_dev, r->time_outs_dev, M.ep_len_s, counters_dev, gamma, s_values, s_rewards,
            r->ep_idx_dev, r->n_ep, r->ep_acc_dev, A.to_owner};
  }
  // the books nmr::PlayArgs and nmr::TapeArgs share, from nm_play_args / nm_tape_args: play_scratch ([4 N + 4], allocated by the caller)
  // stands in for the bookkeeping tensors the caller does not want; advances push_step by K
  float* play_scratch = nullptr;
  template <class P, class R> void kstep_books(P& p, const R* r, int K, real* log) {
    const size_t n_ = (size_t)N;
    p.cur_ret = r->cur_ret ? r->cur_ret : play_scratch; p.cur_len = r->cur_len ? r->cur_len : play_scratch + n_;
    p.ret_sum = r->ret_sum ? r->ret_sum : play_scratch + 2 * n_; p.ret_cnt = r->ret_cnt ? r->ret_cnt : play_scratch + 3 * n_;
    p.fin3 = r->fin3 ? r->fin3 : play_scratch + 4 * n_;
    p.st_sum = roll_sum; p.st_cnt = roll_cnt; p.to_step = roll_to;
    p.rec_log = log; p.rec_done = log ? rec_done : nullptr; p.rec_env = rec_env;
    p.push = kstep_push(K); p.rnoise = kstep_rnoise(); p.rrows = kstep_rrows();
    p.sensor = nmr::SensorArgs{};      // (the entry point fills it: kstep_sensor needs the launch's stream)
    rec_done_valid = log != nullptr;
  }
  int rollout(const nm_rollout_args* r, int act, hipStream_t s) override { return rollout_any("nm_rollout", r, nullptr, act, s); }
  int rollout_priv(const nm_rollout_args* r, const nm_rollout_priv_args* pv, int act, hipStream_t s) override {
    if (!pv) return fail("nm_rollout_priv: priv args is NULL");
    return rollout_any("nm_rollout_priv", r, pv, act, s);
  }
  // ---- the asymmetric rollout (nm_rollout_priv, nm_rollout_act_priv): the packed PrivShape networks and the gather's descriptor
  typedef nmr::PrivShape PS;
  float *rollp_wp = nullptr, *rollp_bp = nullptr;
  nm::PrivObsArgs<float>* priv_desc_dev = nullptr;
  int roll_pack_priv(const float* flat, hipStream_t s) {
    if (!rollp_wp && (dalloc(&rollp_wp, (size_t)PS::nfrag() * 256) || dalloc(&rollp_bp, (size_t)PS::nbias()))) return 1;
    if (nmr::launch_pack_priv(flat, rollp_wp, rollp_bp, s)) return fail("nm_rollout_priv: packing the policy failed to launch");
    return 0;
  }
  int rollout_act_priv(const float* flat, const float* rows, uint64_t seed, const int64_t* iter_dev, int step, int act, float* actions, float* logp, float* values,
                       float* mu, float* sigma, float* obs_store, float* row_store, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if constexpr (sizeof(real) == 8) return fail("nm_rollout_act_priv: the privileged rollout runs on the fp32 env only");
    if (!flat || !rows || !iter_dev || !actions || !logp || !values || !mu || !sigma) return fail("nm_rollout_act_priv: NULL pointer");
    if (roll_pack_priv(flat, s)) return 1;
    nmr::ActOut o{actions, logp, values, mu, sigma, row_store};
    if (nmr::launch_act_priv(rollp_wp, rollp_bp, flat + PS::stdoff(), rows, N, seed, iter_dev, step, o, obs_store, act, s)) return fail("nm_rollout_act_priv: launch failed");
    return 0;
  }
  // nm_rollout (pv = null) and nm_rollout_priv: the same arguments, books and closing launches; `who` names the entry point in messages
  int rollout_any(const char* who_, const nm_rollout_args* r, const nm_rollout_priv_args* pv, int act, hipStream_t s) {
    HIPCHK(hipSetDevice(device));
    const std::string who(who_);
    if constexpr (sizeof(real) == 8 || NM_ENVS_PER_WAVE != 2) {
      return fail(who + ": the fused rollout runs on the fp32 kernel (two envs per wave) only");
    } else {
      if (!r) return fail(who + ": args is NULL");
      const int K = r->steps;
      if (kstep_check(who_, K, "", r->n_ep, r->ep_idx_dev, r->ep_acc_dev, r->ep_stats_dev)) return 1;
      if ((double)K > (double)M.max_ep_len) return fail(who + ": more steps than an episode has (an env may time out once per rollout)");
      if (pv && (!pv->priv0_dev || !pv->priv_final_dev || !pv->s_priv)) return fail(who + ": NULL privileged pointer");
      if (!r->params_flat_dev || !r->iter_dev || (!pv && !r->obs0_dev) || !r->obs_final_dev || !r->episode_length_dev || !r->rew_dev || !r->done_dev || !r->s_obs ||
          !r->s_actions || !r->s_logp || !r->s_values || !r->s_mu || !r->s_sigma || !r->s_rewards || !r->s_dones || !r->cur_ret || !r->cur_len || !r->fin3)
        return fail(who + ": NULL pointer");
      real* log = nullptr;
      if (roll_reserve(K) || log_rows(K, &log)) return 1;
      if (pv ? roll_pack_priv(r->params_flat_dev, s) : roll_pack(r->params_flat_dev, s)) return 1;
      if (pv) {      // the gather's descriptor: the regions and constants as they are now, written in front of the launch on its stream
        if (!priv_desc_dev && dalloc(&priv_desc_dev, 1)) return 1;
        hipLaunchKernelGGL(k_priv_args, dim3(1), dim3(64), 0, s, priv_desc_dev, priv_args());
        HIPCHK(hipGetLastError());
      }
      const nm::Args<real> a = kstep_args(K, nullptr, r->episode_length_dev, sensor_on ? sensor.true_obs : r->obs_final_dev, r->rew_dev, r->done_dev, log);
      nmr::RollPrivArgs R;
      if (pv) {
        R.K = K; R.wp = (const nmr::f32x4*)rollp_wp; R.bp = rollp_bp; R.stdv = r->params_flat_dev + PS::stdoff();
        R.desc = priv_desc_dev; R.priv0 = pv->priv0_dev; R.priv_final = pv->priv_final_dev; R.s_priv = pv->s_priv;
      } else {
        R.K = K; R.wp = (const nmr::f32x4*)roll_wp; R.bp = roll_bp; R.stdv = r->params_flat_dev + RS::stdoff();
        R.desc = nullptr; R.priv0 = nullptr; R.priv_final = nullptr; R.s_priv = nullptr;
      }
      R.seed = r->seed; R.iter_dev = r->iter_dev; R.obs0 = r->obs0_dev; R.obs_final = r->obs_final_dev;
      R.s_obs = r->s_obs; R.s_actions = r->s_actions; R.s_logp = r->s_logp; R.s_values = r->s_values; R.s_mu = r->s_mu; R.s_sigma = r->s_sigma;
      R.s_rewards = r->s_rewards; R.s_dones = r->s_dones; R.cur_ret = r->cur_ret; R.cur_len = r->cur_len; R.fin3 = r->fin3;
      R.st_sum = roll_sum; R.st_cnt = roll_cnt; R.to_step = roll_to;
      R.last_values = r->last_values_dev;
      R.rec_log = log;
      R.push = kstep_push(K); R.rnoise = kstep_rnoise(); R.rrows = kstep_rrows();
      if (kstep_sensor(R.sensor, r->obs_final_dev, s)) return 1;
      R.wave_clock = A.dbg ? reinterpret_cast<unsigned long long*>(A.dbg) : nullptr;   // measurement: the debug buffer ([N,256] reals) takes the waves' clocks instead
      const nmr::TailArgs ta = kstep_tail(r, K, r->bootstrap_time_outs ? r->gamma : -1.0f, r->s_values, r->s_rewards);
      if (kstep_wrench(K, s)) return 1;
      if (pv ? nmr::launch_rollout_priv(M_dev, a, R, ta, act, rows.level(), s) : nmr::launch_rollout(M_dev, a, R, ta, act, rows.level(), s))
        return fail(who + ": launch failed");
      return 0;
    }
  }
  // ---- K x [policy, step] per launch with nothing collected (nm_play; reference play.py:118-132)
  int play(const nm_play_args* r, int act, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if constexpr (sizeof(real) == 8 || NM_ENVS_PER_WAVE != 2) {
      return fail("nm_play: the play kernel runs on the fp32 kernel (two envs per wave) only");
    } else {
      if (!r) return fail("nm_play: args is NULL");
      const int K = r->steps;
      if (kstep_check("nm_play", K, " (longer runs: consecutive launches)", r->n_ep, r->ep_idx_dev, r->ep_acc_dev, r->ep_stats_dev)) return 1;
      if (!r->params_flat_dev || !r->iter_dev || !r->obs0_dev || !r->obs_dev || !r->actions_dev || !r->episode_length_dev || !r->rew_dev || !r->done_dev)
        return fail("nm_play: NULL pointer");
      if ((r->cur_ret == nullptr) != (r->cur_len == nullptr) || (r->ret_sum == nullptr) != (r->ret_cnt == nullptr))
        return fail("nm_play: cur_ret / cur_len and ret_sum / ret_cnt come in pairs");
      real* log = nullptr;
      if (roll_reserve(K) || log_rows(K, &log)) return 1;
      if (!play_scratch && dalloc(&play_scratch, (size_t)N * 4 + 4)) return 1;
      if (roll_pack(r->params_flat_dev, s)) return 1;
      const nm::Args<real> a = kstep_args(K, r->actions_dev, r->episode_length_dev, sensor_on ? sensor.true_obs : r->obs_dev, r->rew_dev, r->done_dev, log);
      nmr::PlayArgs P;
      P.K = K; P.deterministic = r->deterministic != 0;
      P.wp = (const nmr::f32x4*)roll_wp; P.bp = roll_bp; P.stdv = r->params_flat_dev + RS::stdoff();
      P.seed = r->seed; P.iter_dev = r->iter_dev; P.step0 = r->step0;
      P.obs0 = r->obs0_dev; P.obs = r->obs_dev; P.actions = r->actions_dev;
      kstep_books(P, r, K, log);
      if (kstep_sensor(P.sensor, r->obs_dev, s) || kstep_wrench(K, s)) return 1;
      if (nmr::launch_play(M_dev, a, P, kstep_tail(r, K), act, rows.level(), s)) return fail("nm_play: launch failed");
      return 0;
    }
  }
  // ---- K x step from an action tape (nm_step_tape; reference custom_play.py:66-76 around envs/nightmare_v3_env.py:145-311)
  int tape(const nm_tape_args* r, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if constexpr (sizeof(real) == 8 || NM_ENVS_PER_WAVE != 2) {
      return fail("nm_step_tape: the tape kernel runs on the fp32 kernel (two envs per wave) only");
    } else {
      if (!r) return fail("nm_step_tape: args is NULL");
      const int K = r->steps;
      if (kstep_check("nm_step_tape", K, " (longer tapes: consecutive launches)", r->n_ep, r->ep_idx_dev, r->ep_acc_dev, r->ep_stats_dev)) return 1;
      if (!r->actions_dev || !r->obs_dev || !r->episode_length_dev || !r->rew_dev || !r->done_dev) return fail("nm_step_tape: NULL pointer");
      if ((r->cur_ret == nullptr) != (r->cur_len == nullptr) || (r->ret_sum == nullptr) != (r->ret_cnt == nullptr))
        return fail("nm_step_tape: cur_ret / cur_len and ret_sum / ret_cnt come in pairs");
      real* log = nullptr;
      if (roll_reserve(K) || log_rows(K, &log)) return 1;
      if (!play_scratch && dalloc(&play_scratch, (size_t)N * 4 + 4)) return 1;
      const nm::Args<real> a = kstep_args(K, r->actions_dev, r->episode_length_dev, sensor_on ? sensor.true_obs : r->obs_dev, r->rew_dev, r->done_dev, log);
      nmr::TapeArgs T;
      T.K = K; T.tape = r->actions_dev;
      T.rec_obs = r->rec_obs_dev; T.rec_rew = r->rec_rew_dev; T.rec_dones = r->rec_done_dev;
      kstep_books(T, r, K, log);
      if (kstep_sensor(T.sensor, r->obs_dev, s) || kstep_wrench(K, s)) return 1;
      if (nmr::launch_tape(M_dev, a, T, kstep_tail(r, K), rows.level(), s)) return fail("nm_step_tape: launch failed");
      // with an observation record every step filed its observation in its row: the env's own buffer receives the last one
      const size_t n_ = (size_t)N;
      if (r->rec_obs_dev)
        HIPCHK(hipMemcpyAsync(r->obs_dev, r->rec_obs_dev + (size_t)(K - 1) * n_ * nm::kNOBS, n_ * nm::kNOBS * sizeof(float), hipMemcpyDeviceToDevice, s));
      return 0;
    }
  }
  // ---- per-env rows (friction / gains, body rows, actuation latency, gravity, servo target model, servo torque limit, base wrench): ONE lazily allocated block behind A.envp, which every launch copies
  // with the rest of A. Where each kind lies in it, what an unset kind holds, which rows are admitted and which level of the step a launch
  // takes: nm_env_rows.h, and its invariant - once the block exists, every region whose kind is off holds that kind's defaults - is what
  // the functions below keep: each writes or refills its own region and looks at no other kind.
  real* envp_dev = nullptr;
  nmrows::State rows;
  EnvP3<real> envp_default() const { EnvP3<real> d; nmrows::fric_default(M, d.v); return d; }
  int envp_write(EnvP3P<real> src, hipStream_t s) {      // a null column = its default: all null refills the defaults
    hipLaunchKernelGGL(k_envp_set<real>, dim3((4 * N + 255) / 256), dim3(256), 0, s, envp_dev, N, src, envp_default());
    HIPCHK(hipGetLastError());
    return 0;
  }
  // at first use, from the slab (zeroed: the delays, the history and the servo's limited targets start at zero); the fills are ordered on the first caller's stream
  int rows_alloc(hipStream_t s) {
    if (envp_dev) return 0;
    if (dalloc(&envp_dev, nmrows::wrench_block_reals<real>((size_t)N))) return 1;
    return envp_write({}, s) || nmrows::for_each_row_kind([&](auto D) { return kind_fill<decltype(D)>(decltype(D)::rows(envp_dev, N), s) != 0; });
  }
  int rows_turn(nmrows::Kind k, bool on) {
    rows.on[k] = on;
    A.envp = rows.envp(envp_dev);
    return 0;
  }
  // ---- the kinds with a descriptor D (nm_env_rows.h RowKind: body rows, gravity rows, servo rows, torque rows, wrench rows); `who`: the entry point's name
  template <class D> int kind_fill(real* dst, hipStream_t s) {      // the default row for every env
    Vals<real, D::W> r;
    D::dflt(M, r.v);
    hipLaunchKernelGGL((k_row_fill<real, D::W>), dim3((D::W * N + 255) / 256), dim3(256), 0, s, dst, N, r);
    HIPCHK(hipGetLastError());
    return 0;
  }
  template <class D> int kind_set(const char* who, const void* rows_in, hipStream_t s) {
    HIPCHK(hipSetDevice(device));
    if (!rows_in) {       // off; nothing is freed
      if (envp_dev && kind_fill<D>(D::rows(envp_dev, N), s)) return 1;
      if constexpr (D::kind < nmrows::kKinds)       // off also drops the kind's reset pool (nm_reset_rows.h); the base wrench has none
        if (rrows_drop(D::kind, s)) return 1;
      return rows_turn(D::kind, false);
    }
    // the rows are judged on the host before anything of the env changes
    std::vector<real> h((size_t)N * D::W);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(h.data(), rows_in, h.size() * sizeof(real), hipMemcpyDeviceToHost));
    const std::string why = D::fault(h.data(), N);
    if (!why.empty()) return fail(std::string(who) + ": " + why);
    if (rows_alloc(s)) return 1;
    HIPCHK(hipMemcpyAsync(D::rows(envp_dev, N), rows_in, h.size() * sizeof(real), hipMemcpyDeviceToDevice, s));
    return rows_turn(D::kind, true);
  }
  template <class D> int kind_get(void* out, hipStream_t s) {
    HIPCHK(hipSetDevice(device));
    if (!out) return 0;
    if (!envp_dev) return kind_fill<D>((real*)out, s);
    HIPCHK(hipMemcpyAsync(out, D::rows(envp_dev, N), (size_t)N * D::W * sizeof(real), hipMemcpyDeviceToDevice, s));
    return 0;
  }
  // C uniform columns per env at a stride of S words under `key` (k_uniform_draw), into the rows or into the caller's buffer
  template <int C, int S> int draw(real* out, uint64_t key, const double* lo, const double* hi, hipStream_t s) {
    Vals<real, C> l, h;
    for (int k = 0; k < C; k++) { l.v[k] = (real)lo[k]; h.v[k] = (real)hi[k]; }
    hipLaunchKernelGGL((k_uniform_draw<real, C, S>), dim3((S * N + 255) / 256), dim3(256), 0, s, out, N, A.seed, key, A.env_offset, l, h);
    HIPCHK(hipGetLastError());
    return 0;
  }
  int set_env_params(const void* mu, const void* p_gain, const void* kv, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!mu && !p_gain && !kv) {     // off; the rows stay allocated (a launch in flight may read them)
      if (envp_dev && envp_write({}, s)) return 1;
      if (rrows_drop(nmrows::kFric, s)) return 1;
      return rows_turn(nmrows::kFric, false);
    }
    if (rows_alloc(s) || envp_write({{(const real*)mu, (const real*)p_gain, (const real*)kv}}, s)) return 1;
    return rows_turn(nmrows::kFric, true);
  }
  int get_env_params(void* mu, void* p_gain, void* kv, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!mu && !p_gain && !kv) return 0;
    EnvP3W<real> dst{{(real*)mu, (real*)p_gain, (real*)kv}};
    hipLaunchKernelGGL(k_envp_get<real>, dim3((4 * N + 255) / 256), dim3(256), 0, s, (const real*)envp_dev, N, dst, envp_default());
    HIPCHK(hipGetLastError());
    return 0;
  }
  int draw_env_params(const double* lo, const double* hi, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (rows_alloc(s) || draw<3, nm::kEnvP>(envp_dev, nm::kEnvParamKey, lo, hi, s)) return 1;
    return rows_turn(nmrows::kFric, true);
  }
  // ---- per-env body rows (base payload) and gravity rows: the descriptor kinds
  int set_body_params(const void* rows_in, hipStream_t s) override { return kind_set<nmrows::BodyKind>("nm_set_body_params", rows_in, s); }
  int get_body_params(void* out, hipStream_t s) override { return kind_get<nmrows::BodyKind>(out, s); }
  int draw_payload(const double* lo, const double* hi, void* out, hipStream_t s) override {      // (dm, rx, ry, rz)
    HIPCHK(hipSetDevice(device));
    return draw<4, 4>((real*)out, nm::kPayloadKey, lo, hi, s);
  }
  int set_gravity(const void* rows_in, hipStream_t s) override { return kind_set<nmrows::GravKind>("nm_set_gravity", rows_in, s); }
  int get_gravity(void* out, hipStream_t s) override { return kind_get<nmrows::GravKind>(out, s); }
  int draw_gravity(const double* lo, const double* hi, void* out, hipStream_t s) override {      // (three offsets, tilt, azimuth)
    HIPCHK(hipSetDevice(device));
    return draw<5, 5>((real*)out, nm::kGravityKey, lo, hi, s);
  }
  // ---- the servo target model: rows (rate, d_gain, pad, pad) through the descriptor; the limited targets are state (like the history)
  int set_servo(const void* rows_in, hipStream_t s) override { return kind_set<nmrows::ServoKind>("nm_set_servo", rows_in, s); }
  int get_servo(void* out, hipStream_t s) override { return kind_get<nmrows::ServoKind>(out, s); }
  int draw_servo(const double* lo, const double* hi, hipStream_t s) override {      // (rate, d_gain) into the rows
    HIPCHK(hipSetDevice(device));
    if (rows_alloc(s) || draw<2, nm::kServoP>(nmrows::servo_rows(envp_dev, N), nm::kServoKey, lo, hi, s)) return 1;
    return rows_turn(nmrows::kServo, true);
  }
  int get_servo_state(double* L) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    if (!L) return 0;
    if (!envp_dev) { for (size_t i = 0; i < (size_t)N * nm::kNU; i++) L[i] = 0.0; return 0; }      // never allocated: zero, as at construction
    return d2h(nmrows::servo_state(envp_dev, N), L, (size_t)N * nm::kNU);
  }
  int set_servo_state(const double* L) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    if (!L) return fail("nm_set_servo_state: the state is NULL");
    if (rows_alloc(nullptr)) return 1;
    HIPCHK(hipDeviceSynchronize());
    return h2d(nmrows::servo_state(envp_dev, N), L, (size_t)N * nm::kNU);
  }
  // ---- the servo torque limit: rows (fmax coxa, femur, tibia, pad) through the descriptor
  int set_torque_limit(const void* rows_in, hipStream_t s) override { return kind_set<nmrows::TorqueKind>("nm_set_torque_limit", rows_in, s); }
  int get_torque_limit(void* out, hipStream_t s) override { return kind_get<nmrows::TorqueKind>(out, s); }
  int draw_torque_limit(const double* lo, const double* hi, hipStream_t s) override {      // three independent limits into the rows
    HIPCHK(hipSetDevice(device));
    if (rows_alloc(s) || draw<3, nm::kTorqueP>(nmrows::torque_rows(envp_dev, N), nm::kTorqueKey, lo, hi, s)) return 1;
    return rows_turn(nmrows::kTorque, true);
  }
  // ---- the external wrench on the base: rows (F[3], pad, tau[3], pad) through the descriptor; the schedule's rows through k_wrench
  int set_base_wrench(const void* rows_in, hipStream_t s) override { return kind_set<nmrows::WrenchKind>("nm_set_base_wrench", rows_in, s); }
  int get_base_wrench(void* out, hipStream_t s) override { return kind_get<nmrows::WrenchKind>(out, s); }
  // the rows that hold once step wrench_step has begun, and the kind on; without a schedule (interval 0) zero rows, and the kind stays
  // what it is. Synchronous, like nm_set_servo_state: the entry point has no stream
  int install_wrench_schedule() override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    if (wrench_interval == 0) {
      if (envp_dev && kind_fill<nmrows::WrenchKind>(nmrows::wrench_rows(envp_dev, N), nullptr)) return 1;
    } else {
      if (rows_alloc(nullptr)) return 1;
      if (launch_wrench(nm::wrench_window(wrench_interval, wrench_step), nm::wrench_held(wrench_interval, wrench_duration, wrench_step) == 1, nullptr)) return 1;
      rows_turn(nmrows::kWrench, true);
    }
    HIPCHK(hipDeviceSynchronize());
    return 0;
  }
  // ---- per-env actuation latency
  int set_action_latency(const int* substeps, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!substeps) {       // off; nothing is freed, the history keeps what it holds
      if (envp_dev) HIPCHK(hipMemsetAsync(nmrows::delays(envp_dev, N), 0, (size_t)N * sizeof(int), s));
      if (rrows_drop(nmrows::kLat, s)) return 1;
      return rows_turn(nmrows::kLat, false);
    }
    // the delays are judged on the host before anything of the env changes
    std::vector<int> h((size_t)N);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(h.data(), substeps, h.size() * sizeof(int), hipMemcpyDeviceToHost));
    const std::string why = nmrows::delays_fault(h.data(), N, A.nsub);
    if (!why.empty()) return fail("nm_set_action_latency: " + why);
    if (rows_alloc(s)) return 1;
    HIPCHK(hipMemcpyAsync(nmrows::delays(envp_dev, N), substeps, h.size() * sizeof(int), hipMemcpyDeviceToDevice, s));
    return rows_turn(nmrows::kLat, true);
  }
  // a region of 4-byte words for the caller (src null: the block was never allocated - zero, as at construction)
  int words_out(void* out, const void* src, size_t words, hipStream_t s) {
    HIPCHK(hipSetDevice(device));
    if (!out) return 0;
    if (src) HIPCHK(hipMemcpyAsync(out, src, words * 4, hipMemcpyDeviceToDevice, s));
    else HIPCHK(hipMemsetAsync(out, 0, words * 4, s));
    return 0;
  }
  int get_action_latency(int* out, hipStream_t s) override { return words_out(out, envp_dev ? nmrows::delays(envp_dev, N) : nullptr, (size_t)N, s); }
  int draw_action_latency(int lo, int hi, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    const int top = nmrows::delay_max(A.nsub);
    if (hi > top) return fail("nm_draw_action_latency: hi " + std::to_string(hi) + " above " + std::to_string(top) + " substeps");
    if (rows_alloc(s)) return 1;
    hipLaunchKernelGGL(k_latency_draw, dim3((N + 255) / 256), dim3(256), 0, s, nmrows::delays(envp_dev, N), N, A.seed, A.env_offset, lo, hi);
    HIPCHK(hipGetLastError());
    return rows_turn(nmrows::kLat, true);
  }
  int set_action_history(const float* h, hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    if (!h) return fail("nm_set_action_history: the history is NULL");
    if (rows_alloc(s)) return 1;
    HIPCHK(hipMemcpyAsync(nmrows::histories(envp_dev, N), h, nmrows::hist_words((size_t)N) * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
  }
  int get_action_history(float* out, hipStream_t s) override {
    return words_out(out, envp_dev ? nmrows::histories(envp_dev, N) : nullptr, nmrows::hist_words((size_t)N), s);
  }
  void set_dbg(void* p) override { A.dbg = (real*)p; }
  void set_ret_acc(float* p) override { A.ret_acc = p; }
  int invalidate_time_outs(hipStream_t s) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemsetAsync(A.to_owner, 0, sizeof(unsigned long long), s));   // no buffer is "the one the last refresh wrote" any more
    return 0;
  }
  void set_ablate(int m) override { A.ablate = m; }
  int profiling(int on, double* sum_ms, int64_t* count) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    double sum = 0;
    for (size_t i = 0; i < prof_used; i++) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, prof_ev[i].first, prof_ev[i].second));
      sum += ms;
    }
    if (sum_ms) *sum_ms = sum;
    if (count) *count = (int64_t)prof_used;
    prof_used = 0;
    prof_on = on != 0;
    return 0;
  }
};

// ------------------------------------------------------------------------------------------------ C ABI
static const char* kRewardNames[NM_NUM_REWARDS] = {"action_rate", "ang_vel_xy", "base_height", "body_contact_forces", "default_position", "dof_acc",
                                                   "dof_vel", "feet_air_time", "feet_contact_forces", "lin_vel_z", "orientation", "stand_still",
                                                   "torques", "tracking_ang_vel", "tracking_lin_vel", "termination"};
static_assert(NM_NUM_REWARDS == nm::kNREW, "reward table size");
// nm_config (the ABI's) <-> nmhost::EnvConfig (the host model's): the same fields, in either direction; the reward table alone has two names
static double* scales_of(nm_config& c) { return c.reward_scales; }
static const double* scales_of(const nm_config& c) { return c.reward_scales; }
static double* scales_of(nmhost::EnvConfig& c) { return c.rew_scales; }
static const double* scales_of(const nmhost::EnvConfig& c) { return c.rew_scales; }
template <class Dst, class Src> static void config_copy(Dst& d, const Src& s) {
  d.decimation = s.decimation; d.p_gain = s.p_gain; d.action_scale = s.action_scale;
  for (int i = 0; i < 3; i++) d.default_pos[i] = s.default_pos[i];
  d.clip_actions = s.clip_actions; d.clip_observations = s.clip_observations;
  d.obs_lin_vel = s.obs_lin_vel; d.obs_ang_vel = s.obs_ang_vel; d.obs_dof_pos = s.obs_dof_pos; d.obs_dof_vel = s.obs_dof_vel;
  d.episode_length_s = s.episode_length_s; d.resampling_time = s.resampling_time;
  d.max_lin_vel_x = s.max_lin_vel_x; d.max_ang_vel = s.max_ang_vel;
  d.termination_contact_force = s.termination_contact_force; d.tracking_sigma = s.tracking_sigma;
  for (int i = 0; i < NM_NUM_REWARDS; i++) scales_of(d)[i] = scales_of(s)[i];
  d.tibia_contact_mode = s.tibia_contact_mode; d.tibia_max_contact_force = s.tibia_max_contact_force;
  d.body_contact_mode = s.body_contact_mode; d.body_max_contact_force = s.body_max_contact_force;
  d.base_height_target = s.base_height_target; d.max_contact_force = s.max_contact_force;
}
extern "C" {
const char* nm_last_error(void) { return g_err.c_str(); }
int nm_policy_set_error(const char* m) { return fail(m); }
const char* nm_reward_name(int i) { return (i >= 0 && i < NM_NUM_REWARDS) ? kRewardNames[i] : ""; }
void nm_default_config(nm_config* c) { config_copy(*c, nmhost::EnvConfig()); }
int nm_create(const nm_config* cfg, int32_t num_envs, int32_t device, uint64_t seed, int64_t env_id_offset, int32_t dtype, nm_env** out) {
  if (!out) return fail("nm_create: out is NULL");
  *out = nullptr;
  if (num_envs <= 0) return fail("nm_create: num_envs must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail("nm_create: no HIP device available (this backend has no CPU path)");
  if (device < 0 || device >= ndev) return fail("nm_create: bad device index");
  nmhost::EnvConfig c;
  if (cfg) {
    if (cfg->decimation < 1) return fail("nm_create: decimation must be >= 1");
    if (!(cfg->episode_length_s > 0)) return fail("nm_create: episode_length_s must be positive");
    // env.py:235 takes episode_length % int(resampling_time / dt): a period below one step is a division by zero upstream
    if ((int)(cfg->resampling_time / (NM_TIMESTEP * cfg->decimation)) < 1) return fail("nm_create: resampling_time must be at least one env step (dt)");
    if (cfg->tibia_contact_mode < 0 || cfg->tibia_contact_mode > 2 || cfg->body_contact_mode < 0 || cfg->body_contact_mode > 2)
      return fail("nm_create: contact modes are 0 (ignore), 1 (penalise) or 2 (terminate)");
    config_copy(c, *cfg);
  }
  nm_env* e;
  int rc;
  if (dtype == NM_DTYPE_F64) { auto* p = new Env<double>(); rc = p->init(c, num_envs, device, seed, env_id_offset); e = p; }
  else if (dtype == NM_DTYPE_F32) { auto* p = new Env<float>(); rc = p->init(c, num_envs, device, seed, env_id_offset); e = p; }
  else return fail("nm_create: dtype must be NM_DTYPE_F32 or NM_DTYPE_F64");
  if (rc) { delete e; return 1; }
  *out = e;
  return 0;
}
int nm_destroy(nm_env* env) { delete env; return 0; }
int32_t nm_num_envs(const nm_env* env) { return env ? env->N : 0; }
int32_t nm_dtype(const nm_env* env) { return env ? env->dtype : -1; }
#define NEED(e) if (!(e)) return fail("null nm_env")
int nm_reset(nm_env* env, const int32_t* ids, int32_t n, int64_t* eplen, float* ep_stats, void* stream) {
  NEED(env); return env->reset(ids, n, eplen, ep_stats, (hipStream_t)stream);
}
int nm_step(nm_env* env, const float* actions, int64_t* eplen, float* obs, float* rew, int64_t* done, float* time_outs, float* ep_stats,
            void* stream) {
  NEED(env); return env->step(actions, eplen, obs, rew, done, time_outs, ep_stats, 0, (hipStream_t)stream);
}
int nm_privileged_obs(nm_env* env, const float* obs_dev, float* out_dev, void* stream) { NEED(env); return env->priv_obs(obs_dev, out_dev, (hipStream_t)stream); }
int nm_step_physics(nm_env* env, const float* actions, void* stream) {
  NEED(env); return env->step(actions, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, (hipStream_t)stream);
}
int nm_get_state(nm_env* env, double* qpos, double* qvel, double* qw) { NEED(env); return env->get_state(qpos, qvel, qw); }
int nm_set_state(nm_env* env, const double* qpos, const double* qvel, const double* qw) { NEED(env); return env->set_state(qpos, qvel, qw); }
int nm_get_buffers(nm_env* env, double* dp, double* dv, double* act, double* cmd, double* es) { NEED(env); return env->get_buffers(dp, dv, act, cmd, es); }
int nm_set_buffers(nm_env* env, const double* dp, const double* dv, const double* act, const double* cmd, const double* es) {
  NEED(env); return env->set_buffers(dp, dv, act, cmd, es);
}
int nm_get_feet_state(nm_env* env, double* air, unsigned char* last, unsigned char* filt) { NEED(env); return env->get_feet(air, last, filt); }
int nm_set_feet_state(nm_env* env, const double* air, const unsigned char* last, const unsigned char* filt) { NEED(env); return env->set_feet(air, last, filt); }
int nm_set_command_uniforms(nm_env* env, const double* u) { NEED(env); return env->set_cmd_u(u); }
int nm_get_counters(nm_env* env, int64_t* out2) { NEED(env); return env->counters(out2); }
int nm_set_debug_buffer(nm_env* env, void* dbg) { NEED(env); env->set_dbg(dbg); return 0; }
int nm_set_return_accumulator(nm_env* env, float* acc) { NEED(env); env->set_ret_acc(acc); return 0; }
int nm_invalidate_time_outs(nm_env* env, void* stream) { NEED(env); return env->invalidate_time_outs((hipStream_t)stream); }
int nm_rollout_supported(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers) {
  return nm_rollout_supported_act(actor_dims, critic_dims, n_layers, NM_ACT_ELU);
}
int nm_rollout_supported_act(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers, int32_t activation) {
  typedef nmr::RefShape RS;
  if (!nmact::valid(activation)) return 0;
  if (!actor_dims || !critic_dims || n_layers != RS::NL) return 0;
  if (actor_dims[0] != RS::I || critic_dims[0] != RS::I) return 0;
  for (int l = 0; l < RS::NL; l++)
    if (actor_dims[l + 1] != RS::aout(l) || critic_dims[l + 1] != RS::cout(l)) return 0;
  return 1;
}
static int bad_activation(const char* who, int32_t act) {
  return fail(std::string(who) + ": unknown activation code " + std::to_string(act) + " (NM_ACT_*: 0.." + std::to_string(NM_NUM_ACTIVATIONS - 1) + ")");
}
int nm_rollout(nm_env* env, const nm_rollout_args* args, void* stream) { return nm_rollout_ex(env, args, NM_ACT_ELU, stream); }
int nm_rollout_ex(nm_env* env, const nm_rollout_args* args, int32_t activation, void* stream) {
  NEED(env);
  if (!nmact::valid(activation)) return bad_activation("nm_rollout", activation);
  return env->rollout(args, activation, (hipStream_t)stream);
}
int nm_rollout_act(nm_env* env, const float* flat, const float* obs, uint64_t seed, const int64_t* iter_dev, int32_t step, float* actions, float* logp,
                   float* values, float* mu, float* sigma, float* obs_store, void* stream) {
  return nm_rollout_act_ex(env, flat, obs, seed, iter_dev, step, actions, logp, values, mu, sigma, obs_store, NM_ACT_ELU, stream);
}
int nm_rollout_act_ex(nm_env* env, const float* flat, const float* obs, uint64_t seed, const int64_t* iter_dev, int32_t step, float* actions, float* logp,
                      float* values, float* mu, float* sigma, float* obs_store, int32_t activation, void* stream) {
  NEED(env);
  if (!nmact::valid(activation)) return bad_activation("nm_rollout_act", activation);
  return env->rollout_act(flat, obs, seed, iter_dev, step, activation, actions, logp, values, mu, sigma, obs_store, (hipStream_t)stream);
}
int nm_rollout_supported_priv(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers, int32_t activation) {
  typedef nmr::PrivShape PS;
  if (!nmact::valid(activation)) return 0;
  if (!actor_dims || !critic_dims || n_layers != PS::NL) return 0;
  if (actor_dims[0] != PS::IA || critic_dims[0] != PS::I) return 0;
  for (int l = 0; l < PS::NL; l++)
    if (actor_dims[l + 1] != PS::aout(l) || critic_dims[l + 1] != PS::cout(l)) return 0;
  return 1;
}
int nm_rollout_priv(nm_env* env, const nm_rollout_args* args, const nm_rollout_priv_args* priv, int32_t activation, void* stream) {
  NEED(env);
  if (!nmact::valid(activation)) return bad_activation("nm_rollout_priv", activation);
  return env->rollout_priv(args, priv, activation, (hipStream_t)stream);
}
int nm_rollout_act_priv(nm_env* env, const float* flat, const float* rows, uint64_t seed, const int64_t* iter_dev, int32_t step, float* actions, float* logp,
                        float* values, float* mu, float* sigma, float* obs_store, float* row_store, int32_t activation, void* stream) {
  NEED(env);
  if (!nmact::valid(activation)) return bad_activation("nm_rollout_act_priv", activation);
  return env->rollout_act_priv(flat, rows, seed, iter_dev, step, activation, actions, logp, values, mu, sigma, obs_store, row_store, (hipStream_t)stream);
}
#ifdef NM_MEASURE   // include/nightmare_hip_measure.h: not part of the shipped ABI
int nm_set_ablation(nm_env* env, int32_t mask) { NEED(env); env->set_ablate(mask); return 0; }
#endif
int nm_set_observation_noise(nm_env* env, const double* vec) { NEED(env); return env->set_noise(vec); }
int nm_set_noise_uniforms(nm_env* env, const double* u) { NEED(env); return env->set_noise_u(u); }
int nm_set_state_record(nm_env* env, int32_t idx) { NEED(env); return env->set_record(idx); }
int nm_get_state_record(nm_env* env, double* qpos, double* qvel, int32_t* nbad) { NEED(env); return env->get_record(qpos, qvel, nbad); }
int nm_get_state_log(nm_env* env, int32_t first_step, int32_t count, double* rows_host) { NEED(env); return env->get_log(first_step, count, rows_host); }
int nm_get_state_log_dones(nm_env* env, int32_t first_step, int32_t count, unsigned char* dones_host) { NEED(env); return env->get_log_dones(first_step, count, dones_host); }
int nm_play_supported(const int32_t* actor_dims, int32_t n_layers, int32_t activation) {
  typedef nmr::RefShape RS;
  if (!nmact::valid(activation) || !actor_dims || n_layers != RS::NL || actor_dims[0] != RS::I) return 0;
  for (int l = 0; l < RS::NL; l++)
    if (actor_dims[l + 1] != RS::aout(l)) return 0;
  return 1;
}
int nm_play(nm_env* env, const nm_play_args* args, int32_t activation, void* stream) {
  NEED(env);
  if (!nmact::valid(activation)) return bad_activation("nm_play", activation);
  return env->play(args, activation, (hipStream_t)stream);
}
int nm_set_push(nm_env* env, int32_t interval_steps, double max_vel_xy, uint64_t start_step) {
  if (!env) return fail("nm_set_push: env is NULL");
  if (interval_steps < 0) return fail("nm_set_push: interval_steps must be >= 0 (0 = off)");
  if (!(max_vel_xy >= 0.0) || !std::isfinite(max_vel_xy) || (env->dtype == NM_DTYPE_F32 && !std::isfinite((float)max_vel_xy)))
    return fail("nm_set_push: max_vel_xy must be finite and >= 0");
  env->push_interval = interval_steps; env->push_max = max_vel_xy; env->push_step = start_step;
  return 0;
}
int nm_get_push(nm_env* env, int32_t* interval_steps, double* max_vel_xy, uint64_t* step) {
  if (!env) return fail("nm_get_push: env is NULL");
  if (interval_steps) *interval_steps = env->push_interval;
  if (max_vel_xy) *max_vel_xy = env->push_max;
  if (step) *step = env->push_step;
  return 0;
}
#define NEED_ENV(e) if (!(e)) return fail(std::string(__func__) + ": env is NULL")
// the ranges of randomised reset states, judged for `dtype` (NM_DTYPE_*); `who`: the entry point's name
static int reset_ranges_bad(const char* who, const double* r, int dtype) {
  static const char* kName[nm::kResetRanges] = {"base_height", "dof_pos", "base_lin_vel", "base_ang_vel", "dof_vel"};
  for (int k = 0; k < nm::kResetRanges; k++) {
    const double lo = r[2 * k], hi = r[2 * k + 1];
    if (!std::isfinite(lo) || !std::isfinite(hi) || (dtype == NM_DTYPE_F32 && (!std::isfinite((float)lo) || !std::isfinite((float)hi))))
      return fail(std::string(who) + ": the bounds of " + kName[k] + " must be finite");
    if (lo > hi) return fail(std::string(who) + ": lo > hi for " + kName[k]);
    if (dtype == NM_DTYPE_F32 ? !std::isfinite((float)hi - (float)lo) : !std::isfinite(hi - lo))
      return fail(std::string(who) + ": the width of " + kName[k] + " must be finite");
  }
  return 0;
}
int nm_set_reset_noise(nm_env* env, const double* ranges10_host, const uint32_t* counts_host) {
  // every refusal comes before the first device call; the ranges are judged first, so a bad range is named whatever the handle is
  if (ranges10_host && reset_ranges_bad("nm_set_reset_noise", ranges10_host, NM_DTYPE_F64)) return 1;
  NEED_ENV(env);
  if (ranges10_host && reset_ranges_bad("nm_set_reset_noise", ranges10_host, env->dtype)) return 1;
  if ((ranges10_host || counts_host) && env->set_reset_counts(counts_host)) return 1;
  env->rnoise_on = ranges10_host != nullptr;
  for (int i = 0; i < 2 * nm::kResetRanges; i++) env->rnoise_ranges[i] = ranges10_host ? ranges10_host[i] : 0.0;
  return 0;
}
int nm_get_reset_noise(nm_env* env, int32_t* on, double* ranges10, uint32_t* counts_host) {
  NEED_ENV(env);
  if (on) *on = env->rnoise_on;
  if (ranges10) for (int i = 0; i < 2 * nm::kResetRanges; i++) ranges10[i] = env->rnoise_ranges[i];
  return env->get_reset_counts(counts_host);
}
int nm_reset_noise_offsets(const double* ranges10, uint64_t seed, int64_t global_env, uint32_t k, int32_t dtype, double* out43) {
  if (!ranges10 || !out43) return fail("nm_reset_noise_offsets: ranges10 / out43 is NULL");
  if (dtype != NM_DTYPE_F32 && dtype != NM_DTYPE_F64) return fail("nm_reset_noise_offsets: dtype must be NM_DTYPE_F32 or NM_DTYPE_F64");
  if (reset_ranges_bad("nm_reset_noise_offsets", ranges10, dtype)) return 1;
  if (dtype == NM_DTYPE_F32) {
    const nm::ResetNoise<float> p = nm::reset_noise_params<float>(ranges10);
    for (int c = 0; c < nm::kResetCols; c++) out43[c] = (double)nm::reset_noise_draw<float>(p, seed, (uint64_t)global_env, k, c);
  } else {
    const nm::ResetNoise<double> p = nm::reset_noise_params<double>(ranges10);
    for (int c = 0; c < nm::kResetCols; c++) out43[c] = nm::reset_noise_draw<double>(p, seed, (uint64_t)global_env, k, c);
  }
  return 0;
}
// per-env rows re-drawn at reset, from pools (nm_reset_rows.h). Every refusal that needs no look at the pool comes before the first device
// call, the kind and the size first, so a bad pool is named whatever the handle is
int nm_set_reset_rows(nm_env* env, int32_t kind, const void* rows_dev, int32_t P, void* stream) {
  if (kind < 0 || kind >= nm::kResetRowKinds) return fail("nm_set_reset_rows: kind must be 0..5 (friction / gains, body, latency, gravity, servo, torque limit)");
  if (rows_dev && (P < 1 || (uint32_t)P > nm::kResetRowsMaxPool)) return fail("nm_set_reset_rows: a pool holds 1..65536 rows");
  NEED_ENV(env);
  return env->set_reset_rows(kind, rows_dev, (uint32_t)P, (hipStream_t)stream);
}
int nm_get_reset_rows(nm_env* env, int32_t kind, int32_t* P, void* out_dev, void* stream) {
  if (kind < 0 || kind >= nm::kResetRowKinds) return fail("nm_get_reset_rows: kind must be 0..5");
  NEED_ENV(env);
  uint32_t p = 0;
  if (env->get_reset_rows(kind, &p, out_dev, (hipStream_t)stream)) return 1;
  if (P) *P = (int32_t)p;
  return 0;
}
int nm_set_reset_row_counts(nm_env* env, const uint32_t* counts_host) {
  NEED_ENV(env);
  return env->set_reset_row_counts(counts_host);
}
int nm_get_reset_row_counts(nm_env* env, uint32_t* counts_host) {
  NEED_ENV(env);
  return env->get_reset_row_counts(counts_host);
}
int nm_reset_rows_pick(uint64_t seed, int64_t global_env, uint32_t k, const uint32_t sizes[6], uint32_t out[6]) {
  if (!sizes || !out) return fail("nm_reset_rows_pick: sizes / out is NULL");
  for (int i = 0; i < nm::kResetRowKinds; i++)
    if (sizes[i] > nm::kResetRowsMaxPool) return fail("nm_reset_rows_pick: a pool holds at most 65536 rows");
  nm::nm_reset_rows_pick(seed, (uint64_t)global_env, k, sizes, out);
  return 0;
}
int nm_set_env_params(nm_env* env, const void* mu_dev, const void* p_gain_dev, const void* kv_dev, void* stream) {
  NEED_ENV(env);
  return env->set_env_params(mu_dev, p_gain_dev, kv_dev, (hipStream_t)stream);
}
int nm_get_env_params(nm_env* env, void* mu_dev, void* p_gain_dev, void* kv_dev, void* stream) {
  NEED_ENV(env);
  return env->get_env_params(mu_dev, p_gain_dev, kv_dev, (hipStream_t)stream);
}
// What the draws that take lo[n] / hi[n] refuse before the first device call, in this order: null bounds; per column finite, lo <= hi and the
// entry point's own `extra` check (null: none; it returns what is wrong with the column or null); the handle; `out` where there is one;
// the bounds in float32 for an fp32 env. The bounds come first, so a bad range is named whatever the handle is. `who`: the entry point's name.
static int draw_bounds_bad(const char* who, nm_env* env, const double* lo, const double* hi, const char* const* col, int n,
                           const char* (*extra)(int k, double lo), bool has_out, const void* out) {
  const std::string w = std::string(who) + ": ";
  if (!lo || !hi) return fail(w + "lo / hi is NULL");
  for (int k = 0; k < n; k++) {
    if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return fail(w + "the bounds of " + col[k] + " must be finite");
    if (lo[k] > hi[k]) return fail(w + "lo > hi for " + col[k]);
    if (const char* why = extra ? extra(k, lo[k]) : nullptr) return fail(w + why);
  }
  if (!env) return fail(w + "env is NULL");
  if (has_out && !out) return fail(w + "out is NULL");
  if (env->dtype == NM_DTYPE_F32)
    for (int k = 0; k < n; k++)
      if (!std::isfinite((float)lo[k]) || !std::isfinite((float)hi[k])) return fail(w + "the bounds of " + col[k] + " must be finite in float32");
  return 0;
}
int nm_draw_env_params(nm_env* env, const double lo[3], const double hi[3], void* stream) {
  static const char* kCol[3] = {"mu", "p_gain", "kv"};
  const auto extra = [](int k, double lo_k) -> const char* {
    static const char* kNeg[3] = {nullptr, "p_gain must not be negative", "kv must not be negative"};
    return k == 0 ? (lo_k > 1e-5 ? nullptr : "mu must be above 1e-5") : (lo_k < 0.0 ? kNeg[k] : nullptr);
  };
  if (draw_bounds_bad("nm_draw_env_params", env, lo, hi, kCol, 3, extra, false, nullptr)) return 1;
  return env->draw_env_params(lo, hi, (hipStream_t)stream);
}
int nm_set_body_params(nm_env* env, const void* rows_dev, void* stream) {
  NEED_ENV(env);
  return env->set_body_params(rows_dev, (hipStream_t)stream);
}
int nm_get_body_params(nm_env* env, void* out_dev, void* stream) {
  NEED_ENV(env);
  return env->get_body_params(out_dev, (hipStream_t)stream);
}
int nm_draw_payload(nm_env* env, const double lo[4], const double hi[4], void* out_dev, void* stream) {
  static const char* kCol[4] = {"dm", "rx", "ry", "rz"};
  if (draw_bounds_bad("nm_draw_payload", env, lo, hi, kCol, 4, nullptr, true, out_dev)) return 1;
  return env->draw_payload(lo, hi, out_dev, (hipStream_t)stream);
}
int nm_set_action_latency(nm_env* env, const int32_t* substeps_dev, void* stream) {
  NEED_ENV(env);
  return env->set_action_latency(substeps_dev, (hipStream_t)stream);
}
int nm_get_action_latency(nm_env* env, int32_t* out_dev, void* stream) {
  NEED_ENV(env);
  return env->get_action_latency(out_dev, (hipStream_t)stream);
}
int nm_draw_action_latency(nm_env* env, int32_t lo, int32_t hi, void* stream) {
  // the bounds are judged first, so a bad range is named whatever the handle is; the upper limit (history x decimation) needs the env
  if (lo < 0) return fail("nm_draw_action_latency: lo < 0");
  if (lo > hi) return fail("nm_draw_action_latency: lo > hi");
  NEED_ENV(env);
  return env->draw_action_latency(lo, hi, (hipStream_t)stream);
}
int nm_set_action_history(nm_env* env, const float* hist_dev, void* stream) {
  NEED_ENV(env);
  return env->set_action_history(hist_dev, (hipStream_t)stream);
}
int nm_get_action_history(nm_env* env, float* out_dev, void* stream) {
  NEED_ENV(env);
  return env->get_action_history(out_dev, (hipStream_t)stream);
}
int nm_set_gravity(nm_env* env, const void* rows_dev, void* stream) {
  NEED_ENV(env);
  return env->set_gravity(rows_dev, (hipStream_t)stream);
}
int nm_get_gravity(nm_env* env, void* out_dev, void* stream) {
  NEED_ENV(env);
  return env->get_gravity(out_dev, (hipStream_t)stream);
}
int nm_draw_gravity(nm_env* env, const double lo[5], const double hi[5], void* out_dev, void* stream) {
  static const char* kCol[5] = {"offset x", "offset y", "offset z", "tilt", "azimuth"};
  if (draw_bounds_bad("nm_draw_gravity", env, lo, hi, kCol, 5, nullptr, true, out_dev)) return 1;
  return env->draw_gravity(lo, hi, out_dev, (hipStream_t)stream);
}
int nm_set_servo(nm_env* env, const void* rows_dev, void* stream) {
  NEED_ENV(env);
  return env->set_servo(rows_dev, (hipStream_t)stream);
}
int nm_get_servo(nm_env* env, void* out_dev, void* stream) {
  NEED_ENV(env);
  return env->get_servo(out_dev, (hipStream_t)stream);
}
int nm_draw_servo(nm_env* env, const double lo[2], const double hi[2], void* stream) {
  static const char* kCol[2] = {"rate", "d_gain"};
  const auto extra = [](int k, double lo_k) -> const char* {
    return k == 0 ? (lo_k > 0.0 ? nullptr : "rate must be above 0") : (lo_k < 0.0 ? "d_gain must not be negative" : nullptr);
  };
  if (draw_bounds_bad("nm_draw_servo", env, lo, hi, kCol, 2, extra, false, nullptr)) return 1;
  if (env->dtype == NM_DTYPE_F32 && !((float)lo[0] > 0.0f)) return fail("nm_draw_servo: rate must be above 0 in float32");
  return env->draw_servo(lo, hi, (hipStream_t)stream);
}
int nm_get_servo_state(nm_env* env, double* limited) {
  NEED_ENV(env);
  return env->get_servo_state(limited);
}
int nm_set_servo_state(nm_env* env, const double* limited) {
  NEED_ENV(env);
  return env->set_servo_state(limited);
}
// ---- the sensor model (nm_sensor.h): observation latency and bias between the step and whoever reads the observation
static int sensor_draw_bad(const char* who, const int32_t* lo, const int32_t* hi, const double* bias_max) {
  static const char* kGroup[nm::kSensorGroups] = {"imu", "joint"};
  static const char* kKind[nm::kSensorKinds] = {"lin_vel", "ang_vel", "gravity", "dof_pos", "dof_vel"};
  if (!lo || !hi || !bias_max) return fail(std::string(who) + ": NULL bounds");
  for (int g = 0; g < nm::kSensorGroups; g++) {
    if (lo[g] < 0) return fail(std::string(who) + ": lo < 0 for the " + kGroup[g] + " delay");
    if (lo[g] > hi[g]) return fail(std::string(who) + ": lo > hi for the " + kGroup[g] + " delay");
    if (hi[g] > nm::kSensorMaxDelay) return fail(std::string(who) + ": hi above " + std::to_string(nm::kSensorMaxDelay) + " env steps for the " + kGroup[g] + " delay");
  }
  for (int k = 0; k < nm::kSensorKinds; k++)
    if (!(bias_max[k] >= 0.0) || !std::isfinite((float)bias_max[k])) return fail(std::string(who) + ": the maximum of " + kKind[k] + " must be finite and >= 0");
  return 0;
}
int nm_set_sensor(nm_env* env, const int32_t* delays_dev, const float* bias_dev, void* stream) {
  NEED_ENV(env);
  return env->set_sensor(delays_dev, bias_dev, (hipStream_t)stream);
}
int nm_get_sensor(nm_env* env, int32_t* on, int32_t* delays_out_dev, float* bias_out_dev, void* stream) {
  NEED_ENV(env);
  return env->get_sensor(on, delays_out_dev, bias_out_dev, (hipStream_t)stream);
}
int nm_draw_sensor(nm_env* env, const int32_t lo[2], const int32_t hi[2], const double bias_max[5], void* stream) {
  // the bounds are judged first, so a bad range is named whatever the handle is
  if (sensor_draw_bad("nm_draw_sensor", lo, hi, bias_max)) return 1;
  NEED_ENV(env);
  return env->draw_sensor(lo, hi, bias_max, (hipStream_t)stream);
}
int nm_sensor_draw_values(uint64_t seed, int64_t global_env, const int32_t lo[2], const int32_t hi[2], const double bias_max[5], int32_t out_delays[2],
                          float out_bias[NM_NUM_OBS]) {
  if (sensor_draw_bad("nm_sensor_draw_values", lo, hi, bias_max)) return 1;
  if (!out_delays || !out_bias) return fail("nm_sensor_draw_values: NULL output");
  float bmax[nm::kSensorKinds];
  for (int k = 0; k < nm::kSensorKinds; k++) bmax[k] = (float)bias_max[k];
  for (int w = 0; w < nm::kSensorDrawWords; w++)
    nm::sensor_draw(seed, (uint64_t)global_env, lo, hi, bmax, w, out_delays + (w < nm::kNOBS ? 0 : w - nm::kNOBS), out_bias + (w < nm::kNOBS ? w : 0));
  return 0;
}
int nm_get_sensor_state(nm_env* env, float* ring, uint32_t* count) {
  NEED_ENV(env);
  return env->get_sensor_state(ring, count);
}
int nm_set_sensor_state(nm_env* env, const float* ring, const uint32_t* count) {
  NEED_ENV(env);
  return env->set_sensor_state(ring, count);
}
int nm_get_true_obs(nm_env* env, float* out_dev, void* stream) {
  NEED_ENV(env);
  return env->get_true_obs(out_dev, (hipStream_t)stream);
}
// The servo torque limit stands for MuJoCo's actuator forcerange: the clamp of mj_fwdActuation and, in mj_implicit (implicitfast), the
// velocity derivative mjd_actuator_vel leaves out for an actuator whose force sits on its bound (level 6 of the step, nm_core.h stage A)
int nm_set_torque_limit(nm_env* env, const void* rows_dev, void* stream) {      // mj_fwdActuation's clamp + mjd_actuator_vel's mask, per env
  NEED_ENV(env);
  return env->set_torque_limit(rows_dev, (hipStream_t)stream);
}
int nm_get_torque_limit(nm_env* env, void* out_dev, void* stream) {      // the forcerange rows as the stages read them
  NEED_ENV(env);
  return env->get_torque_limit(out_dev, (hipStream_t)stream);
}
int nm_draw_torque_limit(nm_env* env, const double lo[3], const double hi[3], void* stream) {      // forcerange drawn per env and joint type
  static const char* kCol[3] = {"the coxa limit", "the femur limit", "the tibia limit"};
  const auto extra = [](int, double lo_k) -> const char* { return lo_k > 0.0 ? nullptr : "a limit must be above 0"; };
  if (draw_bounds_bad("nm_draw_torque_limit", env, lo, hi, kCol, 3, extra, false, nullptr)) return 1;
  if (env->dtype == NM_DTYPE_F32)
    for (int k = 0; k < 3; k++)
      if (!((float)lo[k] > 0.0f)) return fail("nm_draw_torque_limit: a limit must be above 0 in float32");
  return env->draw_torque_limit(lo, hi, (hipStream_t)stream);
}
// The external wrench on the base stands for MuJoCo's xfrc_applied on the base body (level 7 of the step, nm_core.h stage A)
int nm_set_base_wrench(nm_env* env, const void* rows_dev, void* stream) {      // constant rows, or NULL = off
  NEED_ENV(env);
  if (rows_dev && env->wrench_interval > 0) return fail("nm_set_base_wrench: a wrench schedule is on (nm_set_wrench_schedule with interval_steps = 0 switches it off)");
  if (!rows_dev) { env->wrench_interval = 0; env->wrench_duration = 0; }      // off ends a schedule too
  return env->set_base_wrench(rows_dev, (hipStream_t)stream);
}
int nm_get_base_wrench(nm_env* env, void* out_dev, void* stream) {
  NEED_ENV(env);
  return env->get_base_wrench(out_dev, (hipStream_t)stream);
}
int nm_set_wrench_schedule(nm_env* env, int64_t interval_steps, int64_t duration_steps, const double max_force[3], const double max_torque[3],
                           uint64_t start_step) {
  const std::string w = "nm_set_wrench_schedule: ";
  if (interval_steps < 0) return fail(w + "interval_steps must be >= 0 (0 = no schedule)");
  if (interval_steps >= ((int64_t)1 << 31)) return fail(w + "an interval of 2^31 steps or more is not admitted");
  if (interval_steps > 0) {
    if (!max_force || !max_torque) return fail(w + "max_force / max_torque is NULL");
    for (int k = 0; k < 3; k++) {
      if (!std::isfinite(max_force[k]) || max_force[k] < 0.0) return fail(w + "max_force must be finite and >= 0");
      if (!std::isfinite(max_torque[k]) || max_torque[k] < 0.0) return fail(w + "max_torque must be finite and >= 0");
    }
    if (duration_steps < 1 || duration_steps > interval_steps) return fail(w + "duration_steps must lie in [1, interval_steps]");
  }
  NEED_ENV(env);
  if (interval_steps > 0 && env->dtype == NM_DTYPE_F32)
    for (int k = 0; k < 3; k++)
      if (!std::isfinite((float)max_force[k]) || !std::isfinite((float)max_torque[k])) return fail(w + "the maxima must be finite in float32");
  env->wrench_interval = (int)interval_steps; env->wrench_duration = interval_steps > 0 ? (int)duration_steps : 0; env->wrench_step = start_step;
  for (int k = 0; k < 3; k++) {
    env->wrench_max[k] = interval_steps > 0 ? max_force[k] : 0.0;
    env->wrench_max[3 + k] = interval_steps > 0 ? max_torque[k] : 0.0;
  }
  return env->install_wrench_schedule();
}
int nm_get_wrench_schedule(nm_env* env, int64_t* interval_steps, int64_t* duration_steps, double max_force[3], double max_torque[3], uint64_t* step) {
  NEED_ENV(env);
  if (interval_steps) *interval_steps = env->wrench_interval;
  if (duration_steps) *duration_steps = env->wrench_duration;
  for (int k = 0; k < 3; k++) {
    if (max_force) max_force[k] = env->wrench_max[k];
    if (max_torque) max_torque[k] = env->wrench_max[3 + k];
  }
  if (step) *step = env->wrench_step;
  return 0;
}
int nm_step_tape(nm_env* env, const nm_tape_args* args, void* stream) {
  if (!env) return fail("nm_step_tape: env is NULL");
  if (!args) return fail("nm_step_tape: args is NULL");
  return env->tape(args, (hipStream_t)stream);
}
#ifdef NM_STAMPS
int nm_read_stamps(unsigned long long* out16, int reset) {   // measurement builds only
  (void)hipDeviceSynchronize();
  if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(nm::g_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return fail("nm_read_stamps: copy failed");
  unsigned long long z[16] = {0};
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(nm::g_stamps), z, sizeof z) != hipSuccess) return fail("nm_read_stamps: reset failed");
  return 0;
}
#endif
int nm_set_step_variant(nm_env* env, int32_t mode) {
  NEED(env);
  if (mode != 0 && mode != 1) return fail("nm_set_step_variant: mode must be 0 (choose per launch) or 1 (always the generic kernel)");
  env->step_variant_mode = mode;
  return 0;
}
int nm_get_step_variant(nm_env* env) { return env ? env->step_variant_last : 0; }
int nm_profile(nm_env* env, int32_t enable, double* sum_ms, int64_t* count) { NEED(env); return env->profiling(enable, sum_ms, count); }
}
