// nm_emul_grav.cpp - TEST SCAFFOLDING: the host emulation of the device kernel source (see nm_emul.cpp) with ALL per-env rows of
// nm::Args::envp exposed, the gravity rows (level 4 of the step) included. nm_emul_rows.cpp, which stops at level 3, stays as it is; this
// shim declares the level-4 LDS image (nm::ShWG), so every level can run in it. Layout, default rows, admission, the on / off state and
// the level of a launch are the host object's own (nightmare_rl_amd/csrc/nm_env_rows.h). Never linked into the product library.
#define NM_EMUL 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../nightmare_rl_amd/csrc/nm_host_model.h"
#include "../../nightmare_rl_amd/csrc/nm_env_rows.h"

namespace {
struct Base {
  virtual ~Base() {}
  virtual void get(int what, double* out) = 0;
  virtual void set(int what, const double* in) = 0;
  virtual void set_envp(const double* rows) = 0;
  virtual void set_body(const double* rows) = 0;
  virtual void set_latency(const int* d) = 0;
  virtual int set_gravity(const double* rows) = 0;
  virtual void get_gravity(double* rows8) = 0;
  virtual void get_rows(double* envp3, double* body20, int* delays) = 0;
  virtual int carries_block() = 0;
  virtual void default_body_row(double* out) = 0;
  virtual void on_flags(int* on4) = 0;
  virtual int level(int physics_only) = 0;
  virtual bool device_layout_agrees() = 0;
  virtual float* hist() = 0;
  virtual int64_t* eplen() = 0;
  virtual void step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) = 0;
};

template <class real> struct EmuG : Base {
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
  EmuG(int n, uint64_t s, int64_t o, int g) : N(n), seed(s), off(o), G(g) {
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
    envp.assign(nmrows::block_reals<real>(n_), 0);      // every kind that is off holds its defaults from here on
    set_envp(nullptr); set_body(nullptr); set_gravity(nullptr);
  }
  template <class Fn> void array(int what, Fn fn) {
    switch (what) {
      case 0: return fn(qpos); case 1: return fn(qvel); case 2: return fn(qwarm); case 3: return fn(dofpos); case 4: return fn(dofvel);
      case 5: return fn(act); case 6: return fn(cmd); case 7: return fn(epsum);
      case 8: return fn(feetair); case 9: return fn(feetflags); case 10: return fn(hcache); case 11: return fn(ctr);      // what else a step carries over
    }
  }
  void get(int what, double* out) override { array(what, [&](auto& a) { for (size_t i = 0; i < a.size(); i++) out[i] = (double)a[i]; }); }
  void set(int what, const double* in) override {
    array(what, [&](auto& a) { for (size_t i = 0; i < a.size(); i++) a[i] = (typename std::decay_t<decltype(a)>::value_type)in[i]; });
  }
  void set_envp(const double* in) override {
    rows.on[nmrows::kFric] = in != nullptr;
    real dflt[3];
    nmrows::fric_default(M, dflt);
    for (int i = 0; i < N; i++) {
      real* r = nmrows::fric_rows(envp.data(), N) + (size_t)i * nm::kEnvP;
      for (int k = 0; k < 3; k++) r[k] = in ? (real)in[i * 3 + k] : dflt[k];
      r[3] = real(0);
    }
  }
  void set_body(const double* in) override {
    rows.on[nmrows::kBody] = in != nullptr;
    real dflt[nm::kBodyP];
    nmrows::body_default(M, dflt);
    real* b = nmrows::body_rows(envp.data(), N);
    for (size_t i = 0; i < (size_t)N * nm::kBodyP; i++) b[i] = in ? (real)in[i] : dflt[i % nm::kBodyP];
  }
  void set_latency(const int* d) override {
    rows.on[nmrows::kLat] = d != nullptr;
    for (int i = 0; i < N; i++) nmrows::delays(envp.data(), N)[i] = d ? d[i] : 0;
  }
  int set_gravity(const double* in) override {      // [N,8] rows or null = off; judged by the host's admission before anything changes
    real dflt[nm::kGravP];
    nmrows::grav_default(M, dflt);
    std::vector<real> r((size_t)N * nm::kGravP);
    for (size_t i = 0; i < r.size(); i++) r[i] = in ? (real)in[i] : dflt[i % nm::kGravP];
    if (in && !nmrows::grav_rows_fault(r.data(), N).empty()) return 1;
    std::memcpy(nmrows::grav_rows(envp.data(), N), r.data(), r.size() * sizeof(real));
    rows.on[nmrows::kGrav] = in != nullptr;
    return 0;
  }
  void get_gravity(double* out) override {
    const real* g = nmrows::grav_rows(envp.data(), N);
    for (size_t i = 0; i < (size_t)N * nm::kGravP; i++) out[i] = (double)g[i];
  }
  void get_rows(double* envp3, double* body20, int* d) override {      // what the first three regions hold, whatever is on
    for (int i = 0; i < N; i++) {
      for (int k = 0; k < 3; k++) envp3[i * 3 + k] = (double)nmrows::fric_rows(envp.data(), N)[i * nm::kEnvP + k];
      for (int k = 0; k < nm::kBodyP; k++) body20[i * nm::kBodyP + k] = (double)nmrows::body_rows(envp.data(), N)[i * nm::kBodyP + k];
      d[i] = nmrows::delays(envp.data(), N)[i];
    }
  }
  int carries_block() override { return rows.envp(envp.data()) != nullptr; }
  void default_body_row(double* out) override {
    real r[nm::kBodyP];
    nmrows::body_default(M, r);
    for (int j = 0; j < nm::kBodyP; j++) out[j] = (double)r[j];
  }
  void on_flags(int* on4) override { for (int k = 0; k < 4; k++) on4[k] = rows.on[k]; }
  int level(int physics_only) override { return rows.level(physics_only != 0); }
  // the device's own way to the words behind the body rows ends where the host's layout says, inside the block
  bool device_layout_agrees() override {
    nm::Args<real> A{};
    A.N = N; A.envp = envp.data();
    const real* g = nmrows::grav_rows(envp.data(), N);
    return nm::lat_delay(A) == nmrows::delays(envp.data(), N) && nm::lat_hist(A) == nmrows::histories(envp.data(), N) && nm::grav_rows_of(A) == g &&
           reinterpret_cast<const char*>(nmrows::histories(envp.data(), N) + nmrows::hist_words((size_t)N)) <= reinterpret_cast<const char*>(g) &&
           g + (size_t)N * nm::kGravP == envp.data() + envp.size();
  }
  float* hist() override { return nmrows::histories(envp.data(), N); }
  int64_t* eplen() override { return ep.data(); }
  template <int GG> void waves(const nm::Args<real>& A, int lvl) {
    static thread_local nm::ShWG<real, GG> sh;      // the largest LDS image: every level addresses its rows by offset from the wave's images
    nm::ShW<real, GG>& w = nm::ShWSel<real, GG, 4>::images(sh);
    for (int wv = 0; wv * GG < N; wv++)
      nmrows::with_level(lvl, [&](auto L) { nm::wave_step<real, GG, decltype(L)::value>(w, M, A, wv); });
  }
  void step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) override {
    std::vector<real> cu, dbgr(dbg ? (size_t)N * nm::kDbgN : 0, 0), ssum(nm::kNREW, 0);
    if (cmd_u) { cu.resize((size_t)N * 4); for (size_t i = 0; i < cu.size(); i++) cu[i] = (real)cmd_u[i]; }
    int scnt[4] = {0, 0, 0, 0};
    nm::Args<real> A{};
    A.N = N; A.seed = seed; A.env_offset = off;
    A.qpos = qpos.data(); A.qvel = qvel.data(); A.qwarm = qwarm.data(); A.dofpos = dofpos.data(); A.dofvel = dofvel.data();
    A.act = act.data(); A.cmd = cmd.data(); A.epsum = epsum.data(); A.feetair = feetair.data(); A.feetflags = feetflags.data();
    A.eplen = ep.data(); A.rngctr = ctr.data(); A.hullcache = hcache.data();
    A.actions = actions; A.cmd_u = cmd_u ? cu.data() : nullptr;
    A.obs = obs; A.rew = rew; A.timeout_now = to; A.done = done; A.stat_sum = ssum.data(); A.stat_cnt = scnt;
    A.dbg = dbg ? dbgr.data() : nullptr; A.nsub = nsub; A.physics_only = physics_only;
    const int lvl = level(physics_only);
    A.envp = rows.envp(envp.data());
    if (G == 1) waves<1>(A, lvl);
    else waves<2>(A, lvl);
    if (dbg) for (size_t i = 0; i < dbgr.size(); i++) dbg[i] = (double)dbgr[i];
  }
};
}  // namespace

extern "C" {
void* emug_create(int N, int use_double, uint64_t seed, int64_t env_off, int envs_per_wave) {
  if (use_double) return new EmuG<double>(N, seed, env_off, envs_per_wave);
  return new EmuG<float>(N, seed, env_off, envs_per_wave);
}
void emug_destroy(void* h) { delete (Base*)h; }
void emug_step(void* h, const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) {
  ((Base*)h)->step(actions, cmd_u, obs, rew, done, to, nsub, physics_only, dbg);
}
void emug_get(void* h, int what, double* out) { ((Base*)h)->get(what, out); }
void emug_set(void* h, int what, const double* in) { ((Base*)h)->set(what, in); }
void emug_set_envp(void* h, const double* rows3) { ((Base*)h)->set_envp(rows3); }
void emug_set_body(void* h, const double* rows20) { ((Base*)h)->set_body(rows20); }
void emug_set_latency(void* h, const int* d) { ((Base*)h)->set_latency(d); }
int emug_set_gravity(void* h, const double* rows8) { return ((Base*)h)->set_gravity(rows8); }
void emug_get_gravity(void* h, double* rows8) { ((Base*)h)->get_gravity(rows8); }
void emug_get_rows(void* h, double* envp3, double* body20, int* delays) { ((Base*)h)->get_rows(envp3, body20, delays); }
int emug_carries_block(void* h) { return ((Base*)h)->carries_block(); }
void emug_default_body_row(void* h, double* out20) { ((Base*)h)->default_body_row(out20); }
void emug_on_flags(void* h, int* on4) { ((Base*)h)->on_flags(on4); }
int emug_level(void* h, int physics_only) { return ((Base*)h)->level(physics_only); }
int emug_device_layout_agrees(void* h) { return ((Base*)h)->device_layout_agrees(); }
float* emug_hist(void* h) { return ((Base*)h)->hist(); }
int64_t* emug_eplen(void* h) { return ((Base*)h)->eplen(); }
long emug_together_count() { return nm::nm_emul_together(); }
int emug_grav_p() { return nm::kGravP; }
}
