// nm_emul_rows.cpp - TEST SCAFFOLDING: the host emulation of the device kernel source (see nm_emul.cpp) with ALL per-env rows of
// nm::Args::envp exposed - friction / gain rows, the body rows of a base payload, actuation delays and the action history behind them,
// gravity rows - and the level-4 LDS image (nm::ShWG), so every level of the step can run in it. Layout, default rows, admission, the
// on / off state and the level of the step a launch takes are NOT restated here: they are the host object's own
// (nightmare_rl_amd/csrc/nm_env_rows.h), so a suite that steps this shim tests the host's policy itself. Never linked into the product library.
//
// With -DNM_EMUL_ROWS_MAIN the file is a stand-alone program (for sanitizer builds, which must not be loaded into Python):
// <program> envp|payload|latency <states file> steps one mixed batch of eight envs per population of that feature's fixture, from start
// states it reads from the file, fp32 and fp64, and prints what ran; exit status 0 = every result finite, the two-env constraint pass
// taken, and the matrix-free layout taken (envp, payload) or every history shifted (latency).
#define NM_EMUL 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../nightmare_rl_amd/csrc/nm_host_model.h"
#include "../../nightmare_rl_amd/csrc/nm_env_rows.h"

template <class real> struct EmuR {
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
  EmuR(int n, uint64_t s, int64_t o, int g) : N(n), seed(s), off(o), G(g) {
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
    envp.assign(nmrows::block_reals<real>(n_), 0);      // the host allocates at first use; from then on, like here, every kind that is off holds its defaults
    set_envp(nullptr); set_body(nullptr); set_gravity(nullptr);
  }
  int* delay() { return nmrows::delays(envp.data(), N); }
  float* hist() { return nmrows::histories(envp.data(), N); }
  template <class Fn> void array(int what, Fn fn) {      // fn(the env array of that number): 0..7 what every shim exposes, 8..11 what else a step carries over
    switch (what) {
      case 0: return fn(qpos); case 1: return fn(qvel); case 2: return fn(qwarm); case 3: return fn(dofpos); case 4: return fn(dofvel);
      case 5: return fn(act); case 6: return fn(cmd); case 7: return fn(epsum);
      case 8: return fn(feetair); case 9: return fn(feetflags); case 10: return fn(hcache); case 11: return fn(ctr);
    }
  }
  // each setter writes its own region, or with null refills that region's defaults, and looks at no other kind (nm_env_rows.h)
  void set_envp(const double* in) {   // [N,3] (mu, p_gain, kv) or null = off
    rows.on[nmrows::kFric] = in != nullptr;
    real dflt[3];
    nmrows::fric_default(M, dflt);
    for (int i = 0; i < N; i++) {
      real* r = nmrows::fric_rows(envp.data(), N) + (size_t)i * nm::kEnvP;
      for (int k = 0; k < 3; k++) r[k] = in ? (real)in[i * 3 + k] : dflt[k];
      r[3] = real(0);
    }
  }
  // the kinds with a descriptor D (nm_env_rows.h RowKind): [N, D::W] rows or null = off; judged by the host's admission before anything
  // changes (1 = refused)
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
  int set_body(const double* in) { return set_kind<nmrows::BodyKind>(in); }      // [N,20] body rows
  int set_gravity(const double* in) { return set_kind<nmrows::GravKind>(in); }      // [N,8] rows (g[3], pad, gravity_vec[3], pad)
  void set_latency(const int* d) {   // [N] substeps or null = off; the history keeps what it holds
    rows.on[nmrows::kLat] = d != nullptr;
    for (int i = 0; i < N; i++) delay()[i] = d ? d[i] : 0;
  }
  void default_body_row(double* out) const {   // what nm_get_body_params reports while the feature is off
    real r[nm::kBodyP];
    nmrows::body_default(M, r);
    for (int j = 0; j < nm::kBodyP; j++) out[j] = (double)r[j];
  }
  // the device's own way to the words behind the body rows (nm_core.h lat_delay / lat_hist / grav_rows_of) ends where the host's layout
  // says: the history ends in front of the gravity rows, and those end the block
  bool device_layout_agrees() {
    nm::Args<real> A{};
    A.N = N; A.envp = envp.data();
    const real* g = nmrows::grav_rows(envp.data(), N);
    return nm::lat_delay(A) == delay() && nm::lat_hist(A) == hist() && nm::grav_rows_of(A) == g &&
           reinterpret_cast<const char*>(hist() + nmrows::hist_words((size_t)N)) <= reinterpret_cast<const char*>(g) &&
           g + (size_t)N * nm::kGravP == envp.data() + envp.size();
  }
  template <int GG> void waves(const nm::Args<real>& A, int level) {
    // the largest LDS image for every level: body_rows() / lat_rows() / grav_rows() (nm_core.h) address by offset from the wave's images
    static thread_local nm::ShWG<real, GG> sh;
    nm::ShW<real, GG>& w = nm::ShWSel<real, GG, 4>::images(sh);
    for (int wv = 0; wv * GG < N; wv++)
      nmrows::with_level(level, [&](auto L) { nm::wave_step<real, GG, decltype(L)::value>(w, M, A, wv); });
  }
  void step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) {
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
    A.envp = rows.envp(envp.data());
    if (G == 1) waves<1>(A, rows.level(physics_only != 0));
    else waves<2>(A, rows.level(physics_only != 0));
    if (dbg) for (size_t i = 0; i < dbgr.size(); i++) dbg[i] = (double)dbgr[i];
  }
};

#ifndef NM_EMUL_ROWS_MAIN
namespace {
struct Base {
  virtual ~Base() {}
  virtual void get(int what, double* out) = 0;
  virtual void set(int what, const double* in) = 0;
  virtual void set_envp(const double* rows) = 0;
  virtual int set_body(const double* rows) = 0;
  virtual void set_latency(const int* d) = 0;
  virtual int set_gravity(const double* rows) = 0;
  virtual void default_body_row(double* out) = 0;
  virtual void get_rows(double* envp3, double* body20, int* delays, double* grav8) = 0;
  virtual void on_flags(int* on4) = 0;
  virtual int level(int physics_only) = 0;
  virtual int carries_block() = 0;
  virtual bool device_layout_agrees() = 0;
  virtual float* hist() = 0;
  virtual int64_t* eplen() = 0;
  virtual void step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) = 0;
};
template <class real> struct Impl : Base {
  EmuR<real> e;
  Impl(int n, uint64_t s, int64_t o, int g) : e(n, s, o, g) {}
  void get(int what, double* out) override { e.array(what, [&](auto& a) { for (size_t i = 0; i < a.size(); i++) out[i] = (double)a[i]; }); }
  void set(int what, const double* in) override {
    e.array(what, [&](auto& a) { for (size_t i = 0; i < a.size(); i++) a[i] = (typename std::decay_t<decltype(a)>::value_type)in[i]; });
  }
  void set_envp(const double* rows) override { e.set_envp(rows); }
  int set_body(const double* rows) override { return e.set_body(rows); }
  void set_latency(const int* d) override { e.set_latency(d); }
  int set_gravity(const double* rows) override { return e.set_gravity(rows); }
  void default_body_row(double* out) override { e.default_body_row(out); }
  void get_rows(double* envp3, double* body20, int* delays, double* grav8) override {      // what the block holds, whatever is on
    for (int i = 0; i < e.N; i++) {
      for (int k = 0; k < 3; k++) envp3[i * 3 + k] = (double)nmrows::fric_rows(e.envp.data(), e.N)[i * nm::kEnvP + k];
      for (int k = 0; k < nm::kBodyP; k++) body20[i * nm::kBodyP + k] = (double)nmrows::body_rows(e.envp.data(), e.N)[i * nm::kBodyP + k];
      for (int k = 0; k < nm::kGravP; k++) grav8[i * nm::kGravP + k] = (double)nmrows::grav_rows(e.envp.data(), e.N)[i * nm::kGravP + k];
      delays[i] = e.delay()[i];
    }
  }
  void on_flags(int* on4) override { for (int k = 0; k < 4; k++) on4[k] = e.rows.on[k]; }
  int level(int physics_only) override { return e.rows.level(physics_only != 0); }
  int carries_block() override { return e.rows.envp(e.envp.data()) != nullptr; }      // nm::Args::envp of a launch is not null
  bool device_layout_agrees() override { return e.device_layout_agrees(); }
  float* hist() override { return e.hist(); }
  int64_t* eplen() override { return e.ep.data(); }
  void step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) override {
    e.step(actions, cmd_u, obs, rew, done, to, nsub, physics_only, dbg);
  }
};
}  // namespace

extern "C" {
void* emur_create(int N, int use_double, uint64_t seed, int64_t env_off, int envs_per_wave) {
  if (use_double) return new Impl<double>(N, seed, env_off, envs_per_wave);
  return new Impl<float>(N, seed, env_off, envs_per_wave);
}
void emur_destroy(void* h) { delete (Base*)h; }
void emur_step(void* h, const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) {
  ((Base*)h)->step(actions, cmd_u, obs, rew, done, to, nsub, physics_only, dbg);
}
void emur_get(void* h, int what, double* out) { ((Base*)h)->get(what, out); }
void emur_set(void* h, int what, const double* in) { ((Base*)h)->set(what, in); }
void emur_set_envp(void* h, const double* rows3) { ((Base*)h)->set_envp(rows3); }
int emur_set_body(void* h, const double* rows20) { return ((Base*)h)->set_body(rows20); }
void emur_set_latency(void* h, const int* d) { ((Base*)h)->set_latency(d); }
int emur_set_gravity(void* h, const double* rows8) { return ((Base*)h)->set_gravity(rows8); }
void emur_default_body_row(void* h, double* out20) { ((Base*)h)->default_body_row(out20); }
void emur_get_rows(void* h, double* envp3, double* body20, int* delays, double* grav8) { ((Base*)h)->get_rows(envp3, body20, delays, grav8); }
void emur_on_flags(void* h, int* on4) { ((Base*)h)->on_flags(on4); }
int emur_level(void* h, int physics_only) { return ((Base*)h)->level(physics_only); }
int emur_carries_block(void* h) { return ((Base*)h)->carries_block(); }
int emur_device_layout_agrees(void* h) { return ((Base*)h)->device_layout_agrees(); }
float* emur_hist(void* h) { return ((Base*)h)->hist(); }
int64_t* emur_eplen(void* h) { return ((Base*)h)->eplen(); }
long emur_together_count() { return nm::nm_emul_together(); }
int emur_dbg_n() { return nm::kDbgN; }
int emur_lat_h() { return nm::kLatH; }
int emur_grav_p() { return nm::kGravP; }
}
#else
// ---- the stand-alone program:  <program> envp|payload|latency <states file>
// The file holds raw doubles (the feature's test writes it from its fixture): for payload the body rows of the four payload sets [4*20]
// first; then per population (envp, payload: dropped, standing, flat on the belly; latency: dropped, standing) one start state of N = 8 envs:
// qpos[N*25] qvel[N*24] qacc_warmstart[N*24] dof_pos[N*18] dof_vel[N*18] previous actions[N*18] commands[N*3] actions[N*18]
// and, for latency, history[N*3*18]. One mixed-batch step of each population, fp32 and fp64.
enum Mode { kEnvp, kPayload, kLatency };
constexpr int kN = 8, kState = 25 + 24 + 24 + 18 + 18 + 18 + 3 + 18, kHist = nm::kLatH * 18;
static int pops(Mode m) { return m == kLatency ? 2 : 3; }
static size_t head(Mode m) { return m == kPayload ? 4 * nm::kBodyP : 0; }
static size_t per_pop(Mode m) { return (size_t)kN * (kState + (m == kLatency ? kHist : 0)); }

template <class real> static int run(const char* tag, Mode mode, const std::vector<double>& file) {
  const int N = kN;
  static const double sets[4][3] = {{1.0, 20.0, 0.8}, {0.4, 20.0, 0.5}, {1.6, 14.0, 0.8}, {0.7, 26.0, 1.1}};
  const int delays[8] = {0, 1, 2, 3, 4, 5, 6, 0};
  std::vector<double> envp((size_t)N * 3), body((size_t)N * nm::kBodyP);
  for (int i = 0; i < N; i++) {      // neighbours in a wave always hold different sets
    for (int k = 0; k < 3; k++) envp[i * 3 + k] = sets[(i + i / 4) % 4][k];
    if (mode == kPayload)
      for (int k = 0; k < nm::kBodyP; k++) body[i * nm::kBodyP + k] = file[((i + i / 4) % 4) * nm::kBodyP + k];
  }
  std::vector<float> a((size_t)N * 18), obs((size_t)N * 66), rew(N), to(N);
  std::vector<int64_t> done(N);
  std::vector<double> dbg((size_t)N * nm::kDbgN);
  int bad = 0, big = 0, unshifted = 0;
  const long tog0 = nm::nm_emul_together();
  for (int pop = 0; pop < pops(mode); pop++) {
    EmuR<real> e(N, 3, 0, 2);
    if (mode == kEnvp) e.set_envp(envp.data());
    if (mode == kPayload) e.set_body(body.data());
    if (mode == kLatency) e.set_latency(delays);
    const double* p = file.data() + head(mode) + (size_t)pop * per_pop(mode);
    auto take = [&](std::vector<real>& dst) { for (auto& x : dst) x = (real)*p++; };
    take(e.qpos); take(e.qvel); take(e.qwarm); take(e.dofpos); take(e.dofvel); take(e.act); take(e.cmd);
    for (auto& x : a) x = (float)*p++;
    std::vector<float> h0((size_t)N * kHist);
    if (mode == kLatency) {
      for (auto& x : h0) x = (float)*p++;
      std::memcpy(e.hist(), h0.data(), sizeof(float) * h0.size());
    }
    e.step(a.data(), nullptr, obs.data(), rew.data(), done.data(), to.data(), 2, 0, dbg.data());
    for (float x : obs) bad += !std::isfinite(x);
    for (float x : rew) bad += !std::isfinite(x);
    for (real x : e.qpos) bad += !std::isfinite((double)x);
    for (real x : e.qvel) bad += !std::isfinite((double)x);
    for (int i = 0; i < N; i++) big += dbg[(size_t)i * nm::kDbgN + 160] > nm::kMaxCon;
    if (mode == kLatency)
      for (int i = 0; i < N; i++)      // rows 1 and 2 of the new history are rows 0 and 1 of the old one
        unshifted += std::memcmp(e.hist() + i * kHist + 18, h0.data() + i * kHist, sizeof(float) * 36) != 0;
  }
  const long tog = nm::nm_emul_together() - tog0;
  if (mode == kLatency) {
    std::printf("%s: non-finite values %d, two-env constraint passes %ld, histories not shifted %d\n", tag, bad, tog, unshifted);
    return bad != 0 || tog == 0 || unshifted != 0;
  }
  std::printf("%s: non-finite values %d, two-env constraint passes %ld, envs in the matrix-free layout %d\n", tag, bad, tog, big);
  return bad != 0 || tog == 0 || big == 0;
}
int main(int argc, char** argv) {
  int mode = -1;
  static const char* kNames[3] = {"envp", "payload", "latency"};
  for (int m = 0; m < 3 && argc > 1; m++) if (!std::strcmp(argv[1], kNames[m])) mode = m;
  FILE* f = mode >= 0 && argc > 2 ? std::fopen(argv[2], "rb") : nullptr;
  const size_t want = mode < 0 ? 0 : head((Mode)mode) + pops((Mode)mode) * per_pop((Mode)mode);
  std::vector<double> file(want);
  if (!f || std::fread(file.data(), sizeof(double), want, f) != want) { std::fprintf(stderr, "usage: %s envp|payload|latency <states file>\n", argv[0]); return 2; }
  std::fclose(f);
  const int r32 = run<float>("fp32", (Mode)mode, file), r64 = run<double>("fp64", (Mode)mode, file);
  return r32 | r64;
}
#endif
