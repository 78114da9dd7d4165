// nm_emul.cpp - TEST SCAFFOLDING: compiles the device kernel source (nightmare_rl_amd/csrc/nm_core.h) for the host with
// -DNM_EMUL, where simt.h executes the 64 lanes of a wavefront in lockstep. Lets the exact device algorithm (lane mappings, LDS traffic,
// cross-lane reductions, solver sweeps) be checked against the CPU oracle on a machine without a GPU. Never linked into the product
// library; the product has no CPU path.
//
// -DNM_EMUL_LEVELS=<bitmask> chooses the levels of the step that are compiled in (bit L = level L; a level costs about as much to compile
// as the rest of the file together), default level 0 alone. A step at a level outside the mask runs nothing and returns non-zero. The
// per-env rows behind nm::Args::envp - layout, default rows, admission, on / off state, the level a launch takes - are NOT restated here:
// they are the host object's own (nightmare_rl_amd/csrc/nm_env_rows.h), so a suite that steps this shim tests the host's policy itself.
// With level 0 in the mask the fp32, two-envs-per-wave env has a second step on the lean configuration traits (nm::CfgLean, as in the
// kernel of nm_step_lean.hip), which refuses what the host refuses for the lean kernel (nm::lean_config).
//
// The suite builds levels {0}, {0..4}, {0,5}, {0,6} and {0,7} of it: one small library per feature's suite. A library of all eight levels
// is one -DNM_EMUL_LEVELS=0xffu away and would be the slowest build of the suite.
//
// With -DNM_EMUL_MAIN the file is a stand-alone program (for sanitizer builds, which must not be loaded into Python):
// <program> envp|payload|latency|servo|torque|wrench <states file>; see the end of the file.
#define NM_EMUL 1
#ifndef NM_EMUL_LEVELS
#define NM_EMUL_LEVELS 1u
#endif
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../nightmare_rl_amd/csrc/nm_host_model.h"
#include "../../nightmare_rl_amd/csrc/nm_env_rows.h"

namespace {
constexpr unsigned kMask = NM_EMUL_LEVELS;
constexpr int top_level(unsigned m) { return m > 1 ? 1 + top_level(m >> 1) : 0; }
constexpr int kTop = top_level(kMask);      // its LDS image holds every lower level's: nm::ShWSel
static_assert(kMask != 0 && kMask <= nmrows::kAllLevels, "NM_EMUL_LEVELS: one bit per level 0..7");

// f(D{}) for the descriptor kind (nm_env_rows.h RowKind) of that number; -1 for any other number
template <class F> int with_kind(int kind, F&& f) {
  int r = -1;
  nmrows::for_each_row_kind([&](auto D) { return decltype(D)::kind == kind ? (r = f(D), true) : false; });
  return r;
}

struct Base {
  virtual ~Base() {}
  virtual int step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only,
                   double* dbg, double* stat_sum, int* stat_cnt, int force_level) = 0;
  virtual void array(int what, int set, double* io) = 0;
  virtual void servo_state(int set, double* io) = 0;
  virtual int set_rows(int kind, const void* in) = 0;
  virtual int get_rows(int kind, void* out) = 0;
  virtual int default_row(int kind, double* out) = 0;
  virtual void flags(int* on7, int* levels2, int* carries) = 0;
  virtual bool layout_agrees() = 0;
  virtual float* hist() = 0;
  virtual int64_t* eplen() = 0;
  virtual void set_noise(const double* vec, const double* u) = 0;
  virtual void record(int env, double* out50) = 0;
  virtual void configure(const double* scales, const double* modes6) = 0;
  virtual void feet(int set, double* air, int* flags) = 0;
  virtual void hull_cache(int set, int* hc) = 0;
  virtual int refused_steps() = 0;
};

template <class real> struct Emu : Base {
  int N;
  nmhost::Tables<real> T;
  nm::Model<real> M;
  std::vector<real> qpos, qvel, qwarm, dofpos, dofvel, act, cmd, epsum, feetair, envp;
  std::vector<int64_t> ep;
  std::vector<uint32_t> ctr;
  std::vector<int> hcache, feetflags;
  nmrows::State rows;
  uint64_t seed;
  int64_t off;
  int G;
  bool lean;
  int refused = 0;       // lean steps that did not run because the configuration or the optional inputs are not the lean ones
  std::vector<real> nvec, nu, rec = std::vector<real>(64, 0);
  uint64_t nstep = 0;
  int rec_env = -1;
  Emu(int n, uint64_t s, int64_t o, int g, bool l = false) : N(n), seed(s), off(o), G(g), lean(l) {
    T.build();
    nmhost::EnvConfig cfg;
    T.fill_scalars(M, cfg);
    M.hullv = T.hullv.data(); M.hullnv = T.hullnv.data();
    const size_t n_ = (size_t)N;
    qpos.assign(n_ * 25, 0); qvel.assign(n_ * 24, 0); qwarm.assign(n_ * 24, 0); dofpos.assign(n_ * 18, 0); dofvel.assign(n_ * 18, 0);
    act.assign(n_ * 18, 0); cmd.assign(n_ * 3, 0); epsum.assign(n_ * nm::kNREW, 0); feetair.assign(n_ * 6, 0);
    ep.assign(N, 0); ctr.assign(N, 0); hcache.assign(n_ * 8, 0); feetflags.assign(N, 0);
    for (size_t i = 0; i < n_; i++)
      for (int j = 0; j < 25; j++) qpos[i * 25 + j] = T.qpos0[j];
    // the whole block, as the host allocates it at first use: zero delays, history and limited targets, every kind's defaults (nm_env_rows.h)
    envp.assign(nmrows::wrench_block_reals<real>(n_), 0);
    set_fric(nullptr);
    nmrows::for_each_row_kind([&](auto D) { return set_kind<decltype(D)>(nullptr) != 0; });
  }
  int* delay() { return nmrows::delays(envp.data(), N); }
  float* hist() override { return nmrows::histories(envp.data(), N); }
  real* lim() { return nmrows::servo_state(envp.data(), N); }
  int64_t* eplen() override { return ep.data(); }
  int refused_steps() override { return refused; }

  // ---- the env arrays: 0..7 the state, 8..11 what else a step carries over
  template <class Fn> void with_array(int what, Fn fn) {
    switch (what) {
      case 0: return fn(qpos); case 1: return fn(qvel); case 2: return fn(qwarm); case 3: return fn(dofpos); case 4: return fn(dofvel);
      case 5: return fn(act); case 6: return fn(cmd); case 7: return fn(epsum);
      case 8: return fn(feetair); case 9: return fn(feetflags); case 10: return fn(hcache); case 11: return fn(ctr);
    }
  }
  void array(int what, int set, double* io) override {
    with_array(what, [&](auto& a) {
      for (size_t i = 0; i < a.size(); i++) { if (set) a[i] = (typename std::decay_t<decltype(a)>::value_type)io[i]; else io[i] = (double)a[i]; }
    });
  }
  void servo_state(int set, double* io) override {      // [N,kNU] limited targets: state, like the history in front of them
    for (int i = 0; i < N * nm::kNU; i++) { if (set) lim()[i] = (real)io[i]; else io[i] = (double)lim()[i]; }
  }
  void hull_cache(int set, int* hc) override {
    for (size_t i = 0; i < hcache.size(); i++) { if (set) hcache[i] = hc[i]; else hc[i] = hcache[i]; }
  }
  void feet(int set, double* air, int* flags) override {
    for (size_t i = 0; i < feetair.size(); i++) { if (set) feetair[i] = (real)air[i]; else air[i] = (double)feetair[i]; }
    for (int i = 0; i < N; i++) { if (set) feetflags[i] = flags[i]; else flags[i] = feetflags[i]; }
  }
  void set_noise(const double* vec, const double* u) override {
    nvec.clear(); nu.clear();
    if (vec) nvec.assign(vec, vec + 66);
    if (u) nu.assign(u, u + (size_t)N * 66);
  }
  void record(int env, double* out50) override {
    rec_env = env;
    if (out50) for (int i = 0; i < 50; i++) out50[i] = (double)rec[i];
  }
  void configure(const double* scales, const double* m) override {   // raw reward scales [kNREW] + (tibia mode, max, body mode, max, base height target, max contact force)
    nmhost::EnvConfig cfg;
    for (int k = 0; k < nm::kNREW; k++) cfg.rew_scales[k] = scales[k];
    cfg.tibia_contact_mode = (int)m[0]; cfg.tibia_max_contact_force = m[1]; cfg.body_contact_mode = (int)m[2]; cfg.body_max_contact_force = m[3];
    cfg.base_height_target = m[4]; cfg.max_contact_force = m[5];
    T.fill_scalars(M, cfg);
  }

  // ---- the rows: each setter writes its own region, or with null refills that region's defaults, and looks at no other kind
  void set_fric(const double* in) {   // [N,3] (mu, p_gain, kv) or null = off
    rows.on[nmrows::kFric] = in != nullptr;
    real dflt[3];
    nmrows::fric_default(M, dflt);
    for (int i = 0; i < N; i++) {
      real* r = nmrows::fric_rows(envp.data(), N) + (size_t)i * nm::kEnvP;
      for (int k = 0; k < 3; k++) r[k] = in ? (real)in[i * 3 + k] : dflt[k];
      r[3] = real(0);
    }
  }
  void set_latency(const int* d) {   // [N] substeps or null = off; the history keeps what it holds
    rows.on[nmrows::kLat] = d != nullptr;
    for (int i = 0; i < N; i++) delay()[i] = d ? d[i] : 0;
  }
  // a descriptor kind: [N, D::W] rows or null = off; judged by the host's admission before anything changes (1 = refused)
  template <class D> int set_kind(const double* in) {
    real dflt[D::W];
    D::dflt(M, dflt);
    std::vector<real> r((size_t)N * D::W);
    for (size_t i = 0; i < r.size(); i++) r[i] = in ? (real)in[i] : dflt[i % D::W];
    if (in && !D::fault(r.data(), N).empty()) return 1;
    std::memcpy(D::rows(envp.data(), N), r.data(), r.size() * sizeof(real));
    rows.on[D::kind] = in != nullptr;
    return 0;
  }
  template <class D> int get_kind(double* out) {      // what the region holds, whatever is on
    for (size_t i = 0; i < (size_t)N * D::W; i++) out[i] = (double)D::rows(envp.data(), N)[i];
    return 0;
  }
  int set_rows(int kind, const void* in) override {
    if (kind == nmrows::kFric) return set_fric((const double*)in), 0;
    if (kind == nmrows::kLat) return set_latency((const int*)in), 0;
    return with_kind(kind, [&](auto D) { return set_kind<decltype(D)>((const double*)in); });
  }
  int get_rows(int kind, void* out) override {
    if (kind == nmrows::kFric) {
      for (int i = 0; i < N * 3; i++) ((double*)out)[i] = (double)nmrows::fric_rows(envp.data(), N)[i / 3 * nm::kEnvP + i % 3];
      return 0;
    }
    if (kind == nmrows::kLat) return std::memcpy(out, delay(), (size_t)N * sizeof(int)), 0;
    return with_kind(kind, [&](auto D) { return get_kind<decltype(D)>((double*)out); });
  }
  int default_row(int kind, double* out) override {      // the model's own row in the env's precision: what the host's getter reports while the kind is off
    return with_kind(kind, [&](auto D) {
      real r[decltype(D)::W];
      decltype(D)::dflt(M, r);
      for (int j = 0; j < decltype(D)::W; j++) out[j] = (double)r[j];
      return 0;
    });
  }
  void flags(int* on7, int* levels2, int* carries) override {      // the kinds that are on; the level of a full and of a physics-only launch; nm::Args::envp not null
    for (int k = 0; k < 7; k++) on7[k] = rows.on[k];
    levels2[0] = rows.level(false); levels2[1] = rows.level(true);
    *carries = rows.envp(envp.data()) != nullptr;
  }

  // Every device accessor of nm_core.h ends where the host's layout says, the regions tile the block in order with no gap but the pad
  // behind the histories (less than one real), and the last one ends the block.
  bool layout_agrees() override {
    nm::Args<real> A{};
    A.N = N; A.envp = envp.data();
    const nmrows::Layout L = nmrows::layout<real>((size_t)N);
    const size_t n_ = (size_t)N, R = sizeof(real);
    auto at = [&](const void* p) { return (size_t)((const char*)p - (const char*)envp.data()); };
    real* b = envp.data();
    const bool device = at(nm::lat_delay(A)) == L.delays && at(nm::lat_hist(A)) == L.hist && at(nm::grav_rows_of(A)) == L.grav &&
                        at(nm::servo_rows_of(A)) == L.servo && at(nm::servo_state_of(A)) == L.servo_state && at(nm::torque_rows_of(A)) == L.torque &&
                        at(nm::wrench_rows_of(A)) == L.wrench && at(nm::wrench_args_of(A)) == L.wrench_args;
    const bool host = at(nmrows::fric_rows(b, N)) == L.fric && at(nmrows::body_rows(b, N)) == L.body && at(delay()) == L.delays && at(hist()) == L.hist &&
                      at(nmrows::grav_rows(b, N)) == L.grav && at(nmrows::servo_rows(b, N)) == L.servo && at(lim()) == L.servo_state &&
                      at(nmrows::torque_rows(b, N)) == L.torque && at(nmrows::wrench_rows(b, N)) == L.wrench && at(nmrows::wrench_args(b, N)) == L.wrench_args;
    const bool tiles = L.fric == 0 && L.body == L.fric + n_ * nm::kEnvP * R && L.delays == L.body + n_ * nm::kBodyP * R && L.hist == L.delays + n_ * 4 &&
                       L.pad == L.hist + nmrows::hist_words(n_) * 4 && L.grav >= L.pad && L.grav - L.pad < R && L.grav % R == 0 &&
                       L.servo == L.grav + n_ * nm::kGravP * R && L.servo_state == L.servo + n_ * nm::kServoP * R &&
                       L.torque == L.servo_state + n_ * nm::kNU * R && L.wrench == L.torque + n_ * nm::kTorqueP * R &&
                       L.wrench_args == L.wrench + n_ * nm::kWrenchP * R && L.total == L.wrench_args + nm::kWrenchArgBytes;
    const bool prefixes = nmrows::block_reals<real>(n_) * R == L.servo && nmrows::servo_block_reals<real>(n_) * R == L.torque &&
                          nmrows::torque_block_reals<real>(n_) * R == L.wrench && nmrows::wrench_block_reals<real>(n_) * R == L.total;
    return device && host && tiles && prefixes && L.total == envp.size() * R;
  }

  // ---- stepping, at the level that is the host's own choice from what is on (force_level -1), or at force_level: whatever is on, the
  // block holds every other kind's defaults, so a forced level runs default rows through that level's code. Non-zero, with nothing run,
  // for a level that is not compiled in.
  template <int GG> bool waves(const nm::Args<real>& A, int level) {
    static thread_local typename nm::ShWSel<real, GG, kTop>::type sh;
    nm::ShW<real, GG>& w = nm::ShWSel<real, GG, kTop>::images(sh);
    return nmrows::with_level<kMask>(level, [&](auto L) {
      for (int wv = 0; wv * GG < N; wv++) nm::wave_step<real, GG, decltype(L)::value>(w, M, A, wv);
    });
  }
  nm::Args<real> args(const float* actions, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, real* ssum, int* scnt) {
    nm::Args<real> A{};
    A.N = N; A.seed = seed; A.env_offset = off;
    A.qpos = qpos.data(); A.qvel = qvel.data(); A.qwarm = qwarm.data(); A.dofpos = dofpos.data(); A.dofvel = dofvel.data();
    A.act = act.data(); A.cmd = cmd.data(); A.epsum = epsum.data(); A.feetair = feetair.data(); A.feetflags = feetflags.data();
    A.eplen = ep.data(); A.rngctr = ctr.data(); A.hullcache = hcache.data();
    A.actions = actions; A.obs = obs; A.rew = rew; A.timeout_now = to; A.done = done; A.stat_sum = ssum; A.stat_cnt = scnt;
    A.nsub = nsub; A.physics_only = physics_only;
    return A;
  }
  int step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only,
           double* dbg, double* stat_sum, int* stat_cnt, int force_level) override {
    std::vector<real> cu, dbgr(dbg ? (size_t)N * nm::kDbgN : 0, 0), ssum(nm::kNREW, 0);
    int scnt[4] = {0, 0, 0, 0};
    nm::Args<real> A = args(actions, obs, rew, done, to, nsub, physics_only, ssum.data(), scnt);
    if (lean) {
      if (cmd_u || dbg || !nvec.empty() || rec_env >= 0 || rows.level() || force_level > 0 || !step_lean(A)) { refused++; return 0; }
    } else {
      const int level = force_level >= 0 ? force_level : rows.level(physics_only != 0);
      if (cmd_u) { cu.resize((size_t)N * 4); for (size_t i = 0; i < cu.size(); i++) cu[i] = (real)cmd_u[i]; }
      A.cmd_u = cmd_u ? cu.data() : nullptr;
      A.dbg = dbg ? dbgr.data() : nullptr;
      A.envp = level ? envp.data() : nullptr;      // as nmrows::State::envp, and for a forced level too: level 0 never looks
      if (!physics_only) {
        A.noise_vec = nvec.empty() ? nullptr : nvec.data(); A.noise_u = nu.empty() ? nullptr : nu.data(); A.noise_step = nstep;
        A.rec = rec_env >= 0 ? rec.data() : nullptr; A.rec_env = rec_env;
      }
      if (!(G == 1 ? waves<1>(A, level) : waves<2>(A, level))) return 1;
      if (!physics_only) nstep++;
      if (dbg) for (size_t i = 0; i < dbgr.size(); i++) dbg[i] = (double)dbgr[i];
    }
    if (stat_sum) for (int k = 0; k < nm::kNREW; k++) stat_sum[k] = (double)ssum[k];
    if (stat_cnt) { stat_cnt[0] = scnt[0]; stat_cnt[1] = scnt[1]; }
    return 0;
  }
  // wave_step on nm::CfgLean: fp32, two envs per wave, level 0; false where the host would not launch the lean kernel
  bool step_lean(const nm::Args<real>& A) {
    if constexpr (std::is_same<real, float>::value && (kMask & 1u)) {
      if (G != 2 || !nm::lean_config(M, A)) return false;
      nstep++;
      static thread_local nm::ShW<float, 2> sh;
      for (int wv = 0; wv * 2 < N; wv++) nm::wave_step<float, 2, 0, nm::NoMid, nm::NoMid, nm::Args<float>, nm::CfgLean>(sh, M, A, wv);
      return true;
    }
    return false;
  }
};
}  // namespace

#ifndef NM_EMUL_MAIN
extern "C" {
void* emu_create(int N, int use_double, uint64_t seed, int64_t env_off, int envs_per_wave, int lean) {
  if (use_double) return new Emu<double>(N, seed, env_off, envs_per_wave, lean != 0);
  return new Emu<float>(N, seed, env_off, envs_per_wave, lean != 0);
}
void emu_destroy(void* h) { delete (Base*)h; }
int emu_step(void* h, const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only,
             double* dbg, double* stat_sum, int* stat_cnt, int force_level) {
  return ((Base*)h)->step(actions, cmd_u, obs, rew, done, to, nsub, physics_only, dbg, stat_sum, stat_cnt, force_level);
}
void emu_array(void* h, int what, int set, double* io) { ((Base*)h)->array(what, set, io); }
void emu_servo_state(void* h, int set, double* io) { ((Base*)h)->servo_state(set, io); }
int emu_set_rows(void* h, int kind, const void* in) { return ((Base*)h)->set_rows(kind, in); }
int emu_get_rows(void* h, int kind, void* out) { return ((Base*)h)->get_rows(kind, out); }
int emu_default_row(void* h, int kind, double* out) { return ((Base*)h)->default_row(kind, out); }
void emu_flags(void* h, int* on7, int* levels2, int* carries) { ((Base*)h)->flags(on7, levels2, carries); }
int emu_layout_agrees(void* h) { return ((Base*)h)->layout_agrees(); }
float* emu_hist(void* h) { return ((Base*)h)->hist(); }
int64_t* emu_eplen(void* h) { return ((Base*)h)->eplen(); }
void emu_set_noise(void* h, const double* vec, const double* u) { ((Base*)h)->set_noise(vec, u); }
void emu_record(void* h, int env, double* out50) { ((Base*)h)->record(env, out50); }
void emu_configure(void* h, const double* scales, const double* modes6) { ((Base*)h)->configure(scales, modes6); }
void emu_feet(void* h, int set, double* air, int* flags) { ((Base*)h)->feet(set, air, flags); }
void emu_hull_cache(void* h, int set, int* hc) { ((Base*)h)->hull_cache(set, hc); }
int emu_refused(void* h) { return ((Base*)h)->refused_steps(); }
long emu_together_count() { return nm::nm_emul_together(); }
unsigned emu_levels() { return kMask; }
// what the binding's shapes and columns assume: kNREW, kDbgN, kLatH; the widths of the friction (the 3 words of kEnvP in use), body,
// gravity, servo, torque and wrench rows; EP_KV, SV_RATE, SV_DGAIN, WP_F, WP_T
void emu_sizes(int* out14) {
  const int s[14] = {nm::kNREW,   nm::kDbgN,    nm::kLatH, 3,           nm::kBodyP,   nm::kGravP, nm::kServoP,
                     nm::kTorqueP, nm::kWrenchP, nm::EP_KV, nm::SV_RATE, nm::SV_DGAIN, nm::WP_F,   nm::WP_T};
  std::memcpy(out14, s, sizeof s);
}
}
#else
// ---- the stand-alone program:  <program> envp|payload|latency|servo|torque|wrench <states file>
// It steps one mixed batch of N = 8 envs per population of that feature's fixture, two envs per wave, fp32 and fp64, from start states it
// reads from the file, and prints what ran. Exit status 0 = every result finite, the two-env constraint pass taken, and the mode's own
// condition: the matrix-free layout taken (envp, payload), every history shifted (latency), no limited target moved faster than its
// env's rate (servo). The file holds raw doubles, which the feature's test writes from its fixture: `head` doubles first (payload: the
// body rows of the four payload sets), then per population the state record
//   qpos[N*25] qvel[N*24] qacc_warmstart[N*24] dof_pos[N*18] dof_vel[N*18] previous actions[N*18] commands[N*3] actions[N*18]
// and behind it `tail` doubles per env: latency history[N*3*18]; servo history[N*3*18] limited targets[N*18]; torque limits[N*3] kv[N];
// wrench wrench rows[N*8] body rows[N*20]. Build it with the mode's level alone in NM_EMUL_LEVELS.
constexpr int kN = 8, kState = 25 + 24 + 24 + 18 + 18 + 18 + 3 + 18, kHist = nm::kLatH * 18;
struct Mode { const char* name; int level, pops, head, tail; uint64_t seed; const char* also; };      // also: what the mode counts besides, null = nothing
const Mode kModes[6] = {{"envp", 1, 3, 0, 0, 3, "envs in the matrix-free layout"},
                        {"payload", 2, 3, 4 * nm::kBodyP, 0, 3, "envs in the matrix-free layout"},
                        {"latency", 3, 2, 0, kHist, 3, "histories not shifted"},
                        {"servo", 5, 2, 0, kHist + 18, 5, "limited targets that moved faster than their rate"},
                        {"torque", 6, 2, 0, 3 + 1, 5, nullptr},
                        {"wrench", 7, 2, 0, nm::kWrenchP + nm::kBodyP, 5, nullptr}};

template <class real> int run(const char* tag, const Mode& m, const std::vector<double>& file) {
  const int N = kN;
  static const double sets[4][3] = {{1.0, 20.0, 0.8}, {0.4, 20.0, 0.5}, {1.6, 14.0, 0.8}, {0.7, 26.0, 1.1}};
  const double inf = INFINITY;
  const double servo[16] = {inf, 0, 0.03, 0, 0.02, 0.05, 0.08, 0.05, 0.04, 0.2, inf, 0.2, 0.02, 0, 0.08, 0.1};      // (rate, d_gain) per env
  const int delays[8] = {0, 1, 2, 3, 4, 5, 6, 0};
  std::vector<float> a((size_t)N * 18), obs((size_t)N * 66), rew(N), to(N), h0((size_t)N * kHist);
  std::vector<real> l0((size_t)N * 18);
  std::vector<int64_t> done(N);
  std::vector<double> dbg((size_t)N * nm::kDbgN);
  int bad = 0, also = 0;
  const long tog0 = nm::nm_emul_together();
  for (int pop = 0; pop < m.pops; pop++) {
    Emu<real> e(N, m.seed, 0, 2);
    const double* p = file.data() + m.head + (size_t)pop * kN * (kState + m.tail);
    auto take = [&](std::vector<real>& dst) { for (auto& x : dst) x = (real)*p++; };
    take(e.qpos); take(e.qvel); take(e.qwarm); take(e.dofpos); take(e.dofvel); take(e.act); take(e.cmd);
    for (auto& x : a) x = (float)*p++;
    // the mode's rows: N rows of W doubles, zero but for what put(env, row) gives
    int refused = 0;
    auto rows_of = [&](int kind, int W, auto put) {
      std::vector<double> r((size_t)N * W, 0);
      for (int i = 0; i < N; i++) put(i, r.data() + (size_t)i * W);
      refused |= e.set_rows(kind, r.data());
    };
    auto file_rows = [&](int kind, int W, int w) {      // the file's next N rows of w doubles, in front of rows of W
      rows_of(kind, W, [&](int i, double* r) { std::memcpy(r, p + (size_t)i * w, sizeof(double) * w); });
      p += (size_t)N * w;
    };
    if (m.level == 1) rows_of(nmrows::kFric, 3, [&](int i, double* r) { for (int k = 0; k < 3; k++) r[k] = sets[(i + i / 4) % 4][k]; });      // neighbours in a wave always hold different sets
    if (m.level == 2) rows_of(nmrows::kBody, nm::kBodyP, [&](int i, double* r) { std::memcpy(r, file.data() + ((i + i / 4) % 4) * nm::kBodyP, sizeof(double) * nm::kBodyP); });
    if (m.level == 3 || m.level == 5) {
      e.set_latency(delays);
      for (auto& x : h0) x = (float)*p++;
      std::memcpy(e.hist(), h0.data(), sizeof(float) * h0.size());
    }
    if (m.level == 5) {
      rows_of(nmrows::kServo, nm::kServoP, [&](int i, double* r) { r[nm::SV_RATE] = servo[i * 2]; r[nm::SV_DGAIN] = servo[i * 2 + 1]; });
      take(l0);
      std::memcpy(e.lim(), l0.data(), l0.size() * sizeof(real));
    }
    if (m.level == 6) {      // the limits, and the default friction / gain rows with the file's kv
      file_rows(nmrows::kTorque, nm::kTorqueP, 3);
      real f[3];
      nmrows::fric_default(e.M, f);
      rows_of(nmrows::kFric, 3, [&](int i, double* r) { for (int k = 0; k < 3; k++) r[k] = k == nm::EP_KV ? p[i] : (double)f[k]; });
    }
    if (m.level == 7) { file_rows(nmrows::kWrench, nm::kWrenchP, nm::kWrenchP); file_rows(nmrows::kBody, nm::kBodyP, nm::kBodyP); }
    if (refused || e.step(a.data(), nullptr, obs.data(), rew.data(), done.data(), to.data(), 2, 0, dbg.data(), nullptr, nullptr, -1)) return 1;
    for (float x : obs) bad += !std::isfinite(x);
    for (float x : rew) bad += !std::isfinite(x);
    for (real x : e.qpos) bad += !std::isfinite((double)x);
    for (real x : e.qvel) bad += !std::isfinite((double)x);
    for (int i = 0; i < N; i++) {
      if (m.level <= 2) also += dbg[(size_t)i * nm::kDbgN + 160] > nm::kMaxCon;
      if (m.level == 3)      // rows 1 and 2 of the new history are rows 0 and 1 of the old one
        also += std::memcmp(e.hist() + i * kHist + 18, h0.data() + i * kHist, sizeof(float) * 36) != 0;
      if (m.level == 5)      // a finite rate bounds the move of every limited target (1e-6: float32 roundings of a target below 1 rad)
        for (int j = 0; j < 18; j++)
          also += std::isfinite(servo[i * 2]) && std::fabs((double)e.lim()[i * 18 + j] - (double)l0[i * 18 + j]) > servo[i * 2] + 1e-6;
    }
  }
  const long tog = nm::nm_emul_together() - tog0;
  std::printf("%s: non-finite values %d, two-env constraint passes %ld", tag, bad, tog);
  if (m.also) std::printf(", %s %d", m.also, also);
  std::printf("\n");
  return bad != 0 || tog == 0 || (m.also && (m.level <= 2 ? also == 0 : also != 0));
}
int main(int argc, char** argv) {
  const Mode* m = nullptr;
  for (const Mode& k : kModes) if (argc > 1 && !std::strcmp(argv[1], k.name)) m = &k;
  FILE* f = m && argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  const size_t want = m ? m->head + (size_t)m->pops * kN * (kState + m->tail) : 0;
  std::vector<double> file(want);
  if (!f || std::fread(file.data(), sizeof(double), want, f) != want) { std::fprintf(stderr, "usage: %s envp|payload|latency|servo|torque|wrench <states file>\n", argv[0]); return 2; }
  std::fclose(f);
  const int r32 = run<float>("fp32", *m, file), r64 = run<double>("fp64", *m, file);
  return r32 | r64;
}
#endif
