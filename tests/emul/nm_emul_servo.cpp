// nm_emul_servo.cpp - TEST SCAFFOLDING: the host emulation of the device kernel source (see nm_emul.cpp) for the servo target model
// (level 5 of the step): the servo rows and the limited targets behind the gravity rows of nm::Args::envp, with actuation delays and the
// action history in front of them. It runs levels 0 and 5 only, to keep its build short: every other kind stays at its defaults, which the
// host's invariant (nightmare_rl_amd/csrc/nm_env_rows.h) puts into the block. Layout, defaults and admission are the host object's own.
// Never linked into the product library.
//
// With -DNM_EMUL_SERVO_MAIN the file is a stand-alone program (for sanitizer builds, which must not be loaded into Python):
// <program> <states file> steps one mixed batch of eight envs per population of the servo fixture, fp32 and fp64, and prints what ran;
// exit status 0 = every result finite, the two-env constraint pass taken, every limited target moved by no more than its env's rate.
#define NM_EMUL 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../nightmare_rl_amd/csrc/nm_host_model.h"
#include "../../nightmare_rl_amd/csrc/nm_env_rows.h"

template <class real> struct EmuS {
  int N;
  nmhost::Tables<real> T;
  nm::Model<real> M;
  std::vector<real> qpos, qvel, qwarm, dofpos, dofvel, act, cmd, epsum, feetair, envp;
  std::vector<int64_t> ep;
  std::vector<uint32_t> ctr;
  std::vector<int> hcache, feetflags;
  nmrows::State rows;
  uint64_t seed;
  int G;
  EmuS(int n, int g, uint64_t s = 0) : N(n), seed(s), G(g) {
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
    envp.assign(nmrows::servo_block_reals<real>(n_), 0);      // zero delays, zero history, zero limited targets; every kind's defaults
    fill<nmrows::BodyKind>(); fill<nmrows::GravKind>(); fill<nmrows::ServoKind>();
    real f[3];
    nmrows::fric_default(M, f);
    for (int i = 0; i < N; i++)
      for (int k = 0; k < 3; k++) nmrows::fric_rows(envp.data(), N)[(size_t)i * nm::kEnvP + k] = f[k];
  }
  template <class D> void fill() {
    real d[D::W];
    D::dflt(M, d);
    for (int i = 0; i < N; i++) std::memcpy(D::rows(envp.data(), N) + (size_t)i * D::W, d, sizeof d);
  }
  int* delay() { return nmrows::delays(envp.data(), N); }
  float* hist() { return nmrows::histories(envp.data(), N); }
  real* lim() { return nmrows::servo_state(envp.data(), N); }
  template <class Fn> void array(int what, Fn fn) {
    switch (what) {
      case 0: return fn(qpos); case 1: return fn(qvel); case 2: return fn(qwarm); case 3: return fn(dofpos); case 4: return fn(dofvel);
      case 5: return fn(act); case 6: return fn(cmd); case 7: return fn(epsum);
    }
  }
  int set_servo(const double* in) {      // [N,2] (rate, d_gain) or null = off; judged by the host's admission before anything changes
    typedef nmrows::ServoKind D;
    if (!in) { fill<D>(); rows.on[D::kind] = false; return 0; }
    std::vector<real> r((size_t)N * D::W, real(0));
    for (int i = 0; i < N; i++) { r[(size_t)i * D::W + nm::SV_RATE] = (real)in[i * 2]; r[(size_t)i * D::W + nm::SV_DGAIN] = (real)in[i * 2 + 1]; }
    if (!D::fault(r.data(), N).empty()) return 1;
    std::memcpy(D::rows(envp.data(), N), r.data(), r.size() * sizeof(real));
    rows.on[D::kind] = true;
    return 0;
  }
  void set_latency(const int* d) {   // [N] substeps or null = off
    rows.on[nmrows::kLat] = d != nullptr;
    for (int i = 0; i < N; i++) delay()[i] = d ? d[i] : 0;
  }
  // the device's own way to the servo regions ends where the host's layout says, and they end the block
  bool device_layout_agrees() {
    nm::Args<real> A{};
    A.N = N; A.envp = envp.data();
    return nm::servo_rows_of(A) == nmrows::servo_rows(envp.data(), N) && nm::servo_state_of(A) == lim() &&
           nm::grav_rows_of(A) + (size_t)N * nm::kGravP == nm::servo_rows_of(A) && lim() + (size_t)N * nm::kNU == envp.data() + envp.size();
  }
  template <int GG> void waves(const nm::Args<real>& A, int level) {
    static thread_local nm::ShWG<real, GG> sh;
    nm::ShW<real, GG>& w = nm::ShWSel<real, GG, 5>::images(sh);
    for (int wv = 0; wv * GG < N; wv++) {
      if (level == 5) nm::wave_step<real, GG, 5>(w, M, A, wv);
      else nm::wave_step<real, GG, 0>(w, M, A, wv);
    }
  }
  // level 5 while the servo rows are on, level 0 otherwise (the shim runs no other level: with latency alone it refuses)
  int step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only) {
    const int level = rows.level(physics_only != 0);
    if (level != 0 && level != 5) return 1;
    std::vector<real> cu, ssum(nm::kNREW, 0);
    if (cmd_u) { cu.resize((size_t)N * 4); for (size_t i = 0; i < cu.size(); i++) cu[i] = (real)cmd_u[i]; }
    int scnt[4] = {0, 0, 0, 0};
    nm::Args<real> A{};
    A.N = N; A.seed = seed; A.env_offset = 0;
    A.qpos = qpos.data(); A.qvel = qvel.data(); A.qwarm = qwarm.data(); A.dofpos = dofpos.data(); A.dofvel = dofvel.data();
    A.act = act.data(); A.cmd = cmd.data(); A.epsum = epsum.data(); A.feetair = feetair.data(); A.feetflags = feetflags.data();
    A.eplen = ep.data(); A.rngctr = ctr.data(); A.hullcache = hcache.data();
    A.actions = actions; A.cmd_u = cmd_u ? cu.data() : nullptr;
    A.obs = obs; A.rew = rew; A.timeout_now = to; A.done = done; A.stat_sum = ssum.data(); A.stat_cnt = scnt;
    A.nsub = nsub; A.physics_only = physics_only;
    A.envp = rows.envp(envp.data());
    if (G == 1) waves<1>(A, level);
    else waves<2>(A, level);
    return 0;
  }
};

#ifndef NM_EMUL_SERVO_MAIN
namespace {
struct Base {
  virtual ~Base() {}
  virtual void get(int what, double* out) = 0;
  virtual void set(int what, const double* in) = 0;
  virtual int set_servo(const double* rows2) = 0;
  virtual void get_servo(double* rows2) = 0;
  virtual void set_latency(const int* d) = 0;
  virtual void get_lim(double* out) = 0;
  virtual void set_lim(const double* in) = 0;
  virtual int level(int physics_only) = 0;
  virtual bool device_layout_agrees() = 0;
  virtual float* hist() = 0;
  virtual int64_t* eplen() = 0;
  virtual int step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only) = 0;
};
template <class real> struct Impl : Base {
  EmuS<real> e;
  Impl(int n, int g, uint64_t s) : e(n, g, s) {}
  void get(int what, double* out) override { e.array(what, [&](auto& a) { for (size_t i = 0; i < a.size(); i++) out[i] = (double)a[i]; }); }
  void set(int what, const double* in) override { e.array(what, [&](auto& a) { for (size_t i = 0; i < a.size(); i++) a[i] = (real)in[i]; }); }
  int set_servo(const double* rows2) override { return e.set_servo(rows2); }
  void get_servo(double* rows2) override {
    const real* r = nmrows::servo_rows(e.envp.data(), e.N);
    for (int i = 0; i < e.N; i++) { rows2[i * 2] = (double)r[i * nm::kServoP + nm::SV_RATE]; rows2[i * 2 + 1] = (double)r[i * nm::kServoP + nm::SV_DGAIN]; }
  }
  void set_latency(const int* d) override { e.set_latency(d); }
  void get_lim(double* out) override { for (int i = 0; i < e.N * nm::kNU; i++) out[i] = (double)e.lim()[i]; }
  void set_lim(const double* in) override { for (int i = 0; i < e.N * nm::kNU; i++) e.lim()[i] = (real)in[i]; }
  int level(int physics_only) override { return e.rows.level(physics_only != 0); }
  bool device_layout_agrees() override { return e.device_layout_agrees(); }
  float* hist() override { return e.hist(); }
  int64_t* eplen() override { return e.ep.data(); }
  int step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only) override {
    return e.step(actions, cmd_u, obs, rew, done, to, nsub, physics_only);
  }
};
}  // namespace

extern "C" {
void* emus_create(int N, int use_double, uint64_t seed, int envs_per_wave) {
  if (use_double) return new Impl<double>(N, envs_per_wave, seed);
  return new Impl<float>(N, envs_per_wave, seed);
}
void emus_destroy(void* h) { delete (Base*)h; }
int emus_step(void* h, const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only) {
  return ((Base*)h)->step(actions, cmd_u, obs, rew, done, to, nsub, physics_only);
}
void emus_get(void* h, int what, double* out) { ((Base*)h)->get(what, out); }
void emus_set(void* h, int what, const double* in) { ((Base*)h)->set(what, in); }
int emus_set_servo(void* h, const double* rows2) { return ((Base*)h)->set_servo(rows2); }
void emus_get_servo(void* h, double* rows2) { ((Base*)h)->get_servo(rows2); }
void emus_set_latency(void* h, const int* d) { ((Base*)h)->set_latency(d); }
void emus_get_lim(void* h, double* out) { ((Base*)h)->get_lim(out); }
void emus_set_lim(void* h, const double* in) { ((Base*)h)->set_lim(in); }
int emus_level(void* h, int physics_only) { return ((Base*)h)->level(physics_only); }
int emus_device_layout_agrees(void* h) { return ((Base*)h)->device_layout_agrees(); }
float* emus_hist(void* h) { return ((Base*)h)->hist(); }
int64_t* emus_eplen(void* h) { return ((Base*)h)->eplen(); }
long emus_together_count() { return nm::nm_emul_together(); }
int emus_lat_h() { return nm::kLatH; }
}
#else
// ---- the stand-alone program:  <program> <states file>
// The file holds raw doubles (tests/test_servo_emulated.py writes it from the fixture's SL recording): per population (dropped, standing) one
// start state of N = 8 envs: qpos[N*25] qvel[N*24] qacc_warmstart[N*24] dof_pos[N*18] dof_vel[N*18] previous actions[N*18] commands[N*3]
// actions[N*18] history[N*3*18] limited targets[N*18]. One mixed-batch step of each population, fp32 and fp64, under the fixture's rows and delays.
constexpr int kN = 8, kHist = nm::kLatH * 18, kState = 25 + 24 + 24 + 18 + 18 + 18 + 3 + 18 + kHist + 18, kPops = 2;

template <class real> static int run(const char* tag, const std::vector<double>& file) {
  const int N = kN;
  const double inf = INFINITY;
  const double rows[16] = {inf, 0, 0.03, 0, 0.02, 0.05, 0.08, 0.05, 0.04, 0.2, inf, 0.2, 0.02, 0, 0.08, 0.1};
  const int delays[8] = {0, 1, 2, 3, 4, 5, 6, 0};
  std::vector<float> a((size_t)N * 18), obs((size_t)N * 66), rew(N), to(N);
  std::vector<int64_t> done(N);
  int bad = 0, fast = 0;
  const long tog0 = nm::nm_emul_together();
  for (int pop = 0; pop < kPops; pop++) {
    EmuS<real> e(N, 2, 5);
    if (e.set_servo(rows)) return 1;
    e.set_latency(delays);
    const double* p = file.data() + (size_t)pop * kN * kState;
    auto take = [&](std::vector<real>& dst) { for (auto& x : dst) x = (real)*p++; };
    take(e.qpos); take(e.qvel); take(e.qwarm); take(e.dofpos); take(e.dofvel); take(e.act); take(e.cmd);
    for (auto& x : a) x = (float)*p++;
    for (int i = 0; i < N * kHist; i++) e.hist()[i] = (float)*p++;
    std::vector<real> l0((size_t)N * 18);
    for (auto& x : l0) x = (real)*p++;
    std::memcpy(e.lim(), l0.data(), l0.size() * sizeof(real));
    if (e.step(a.data(), nullptr, obs.data(), rew.data(), done.data(), to.data(), 2, 0)) return 1;
    for (float x : obs) bad += !std::isfinite(x);
    for (float x : rew) bad += !std::isfinite(x);
    for (real x : e.qpos) bad += !std::isfinite((double)x);
    for (real x : e.qvel) bad += !std::isfinite((double)x);
    for (int i = 0; i < N; i++)      // a finite rate bounds the move of every limited target (1e-6: float32 roundings of a target below 1 rad)
      for (int j = 0; j < 18; j++)
        fast += std::isfinite(rows[i * 2]) && std::fabs((double)e.lim()[i * 18 + j] - (double)l0[i * 18 + j]) > rows[i * 2] + 1e-6;
  }
  const long tog = nm::nm_emul_together() - tog0;
  std::printf("%s: non-finite values %d, two-env constraint passes %ld, limited targets that moved faster than their rate %d\n", tag, bad, tog, fast);
  return bad != 0 || tog == 0 || fast != 0;
}
int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
  const size_t want = (size_t)kPops * kN * kState;
  std::vector<double> file(want);
  if (!f || std::fread(file.data(), sizeof(double), want, f) != want) { std::fprintf(stderr, "usage: %s <states file>\n", argv[0]); return 2; }
  std::fclose(f);
  const int r32 = run<float>("fp32", file), r64 = run<double>("fp64", file);
  return r32 | r64;
}
#endif
