// nm_emul_wrench.cpp - TEST SCAFFOLDING: the host emulation of the device kernel source (see nm_emul.cpp) for the external wrench on the
// base (level 7 of the step): the wrench rows behind the torque rows of nm::Args::envp. It runs levels 0 and 7 only, to keep its build
// short: every other kind stays at its defaults, which the host's invariant (nightmare_rl_amd/csrc/nm_env_rows.h) puts into the block -
// but for the body rows, which the fixture's set 3 (a payload with a displaced COM) needs per env. Layout, defaults and admission are the
// host object's own. Never linked into the product library.
//
// With -DNM_EMUL_WRENCH_MAIN the file is a stand-alone program (for sanitizer builds, which must not be loaded into Python):
// <program> <states file> steps one mixed batch of eight envs per population of the wrench fixture, fp32 and fp64, and prints what ran;
// exit status 0 = every result finite and the two-env constraint pass taken.
#define NM_EMUL 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../nightmare_rl_amd/csrc/nm_host_model.h"
#include "../../nightmare_rl_amd/csrc/nm_env_rows.h"

template <class real> struct EmuX {
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
  EmuX(int n, int g, uint64_t s = 0) : N(n), seed(s), G(g) {
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
    envp.assign(nmrows::wrench_block_reals<real>(n_), 0);      // zero delays, zero history, zero limited targets; every kind's defaults
    real f[3];
    nmrows::fric_default(M, f);
    for (int i = 0; i < N; i++)
      for (int k = 0; k < 3; k++) nmrows::fric_rows(envp.data(), N)[(size_t)i * nm::kEnvP + k] = f[k];
    fill<nmrows::BodyKind>(); fill<nmrows::GravKind>(); fill<nmrows::ServoKind>(); fill<nmrows::TorqueKind>(); fill<nmrows::WrenchKind>();
  }
  template <class D> void fill() {
    real d[D::W];
    D::dflt(M, d);
    for (int i = 0; i < N; i++) std::memcpy(D::rows(envp.data(), N) + (size_t)i * D::W, d, sizeof d);
  }
  template <class Fn> void array(int what, Fn fn) {
    switch (what) {
      case 0: return fn(qpos); case 1: return fn(qvel); case 2: return fn(qwarm); case 3: return fn(dofpos); case 4: return fn(dofvel);
      case 5: return fn(act); case 6: return fn(cmd); case 7: return fn(epsum);
    }
  }
  // a descriptor kind: [N, D::W] rows or null = off; judged by the host's admission before anything changes
  template <class D> int set_kind(const double* in) {
    if (!in) { fill<D>(); rows.on[D::kind] = false; return 0; }
    std::vector<real> r((size_t)N * D::W);
    for (size_t i = 0; i < r.size(); i++) r[i] = (real)in[i];
    if (!D::fault(r.data(), N).empty()) return 1;
    std::memcpy(D::rows(envp.data(), N), r.data(), r.size() * sizeof(real));
    rows.on[D::kind] = true;
    return 0;
  }
  // the device's own way to the wrench rows ends where the host's layout says, and the launch arguments behind them end the block
  bool device_layout_agrees() {
    nm::Args<real> A{};
    A.N = N; A.envp = envp.data();
    return nm::wrench_rows_of(A) == nmrows::wrench_rows(envp.data(), N) && nm::torque_rows_of(A) + (size_t)N * nm::kTorqueP == nm::wrench_rows_of(A) &&
           (const real*)nm::wrench_args_of(A) + nm::kWrenchArgBytes / sizeof(real) == envp.data() + envp.size() &&
           nm::wrench_args_of(A) == nmrows::wrench_args(envp.data(), N) && nm::wrench_args_of(A) == nm::wrench_rows_of(A) + (size_t)N * nm::kWrenchP &&
           nmrows::wrench_block_reals<real>((size_t)N) == nmrows::torque_block_reals<real>((size_t)N) + (size_t)N * nm::kWrenchP + nm::kWrenchArgBytes / sizeof(real) &&
           nm::torque_rows_of(A) == nmrows::torque_rows(envp.data(), N);
  }
  template <int GG> void waves(const nm::Args<real>& A, int level) {
    static thread_local nm::ShWX<real, GG> sh;
    nm::ShW<real, GG>& w = nm::ShWSel<real, GG, 7>::images(sh);
    for (int wv = 0; wv * GG < N; wv++) {
      if (level == 7) nm::wave_step<real, GG, 7>(w, M, A, wv);
      else nm::wave_step<real, GG, 0>(w, M, A, wv);
    }
  }
  // level 7 while the wrench rows are on, level 0 otherwise (the shim runs no other level: with body rows alone it refuses).
  // force_level 7: default rows through the level-7 code (the block holds them whatever is on)
  int step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, int force_level) {
    const int level = force_level >= 0 ? force_level : rows.level(physics_only != 0);
    if (level != 0 && level != 7) return 1;
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
    A.envp = level ? envp.data() : nullptr;
    if (G == 1) waves<1>(A, level);
    else waves<2>(A, level);
    return 0;
  }
};

#ifndef NM_EMUL_WRENCH_MAIN
namespace {
struct Base {
  virtual ~Base() {}
  virtual void get(int what, double* out) = 0;
  virtual void set(int what, const double* in) = 0;
  virtual int set_wrench(const double* rows8) = 0;
  virtual void get_wrench(double* rows8) = 0;
  virtual int set_body(const double* rows20) = 0;
  virtual int level(int physics_only) = 0;
  virtual bool device_layout_agrees() = 0;
  virtual int64_t* eplen() = 0;
  virtual int step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, int force_level) = 0;
};
template <class real> struct Impl : Base {
  EmuX<real> e;
  Impl(int n, int g, uint64_t s) : e(n, g, s) {}
  void get(int what, double* out) override { e.array(what, [&](auto& a) { for (size_t i = 0; i < a.size(); i++) out[i] = (double)a[i]; }); }
  void set(int what, const double* in) override { e.array(what, [&](auto& a) { for (size_t i = 0; i < a.size(); i++) a[i] = (real)in[i]; }); }
  int set_wrench(const double* rows8) override { return e.template set_kind<nmrows::WrenchKind>(rows8); }
  void get_wrench(double* rows8) override {
    const real* r = nmrows::wrench_rows(e.envp.data(), e.N);
    for (int i = 0; i < e.N * nm::kWrenchP; i++) rows8[i] = (double)r[i];
  }
  int set_body(const double* rows20) override { return e.template set_kind<nmrows::BodyKind>(rows20); }
  int level(int physics_only) override { return e.rows.level(physics_only != 0); }
  bool device_layout_agrees() override { return e.device_layout_agrees(); }
  int64_t* eplen() override { return e.ep.data(); }
  int step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, int force_level) override {
    return e.step(actions, cmd_u, obs, rew, done, to, nsub, physics_only, force_level);
  }
};
}  // namespace

extern "C" {
void* emux_create(int N, int use_double, uint64_t seed, int envs_per_wave) {
  if (use_double) return new Impl<double>(N, envs_per_wave, seed);
  return new Impl<float>(N, envs_per_wave, seed);
}
void emux_destroy(void* h) { delete (Base*)h; }
int emux_step(void* h, const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, int force_level) {
  return ((Base*)h)->step(actions, cmd_u, obs, rew, done, to, nsub, physics_only, force_level);
}
void emux_get(void* h, int what, double* out) { ((Base*)h)->get(what, out); }
void emux_set(void* h, int what, const double* in) { ((Base*)h)->set(what, in); }
int emux_set_wrench(void* h, const double* rows8) { return ((Base*)h)->set_wrench(rows8); }
void emux_get_wrench(void* h, double* rows8) { ((Base*)h)->get_wrench(rows8); }
int emux_set_body(void* h, const double* rows20) { return ((Base*)h)->set_body(rows20); }
int emux_level(void* h, int physics_only) { return ((Base*)h)->level(physics_only); }
int emux_device_layout_agrees(void* h) { return ((Base*)h)->device_layout_agrees(); }
int64_t* emux_eplen(void* h) { return ((Base*)h)->eplen(); }
long emux_together_count() { return nm::nm_emul_together(); }
}
#else
// ---- the stand-alone program:  <program> <states file>
// The file holds raw doubles (tests/test_wrench_emulated.py writes it from the fixture): per population (dropped, standing) one start
// state of N = 8 envs: qpos[N*25] qvel[N*24] qacc_warmstart[N*24] dof_pos[N*18] dof_vel[N*18] previous actions[N*18] commands[N*3]
// actions[N*18] wrench rows[N*8] body rows[N*20]. One mixed-batch step of each population, fp32 and fp64.
constexpr int kN = 8, kState = 25 + 24 + 24 + 18 + 18 + 18 + 3 + 18 + 8 + 20, kPops = 2;

template <class real> static int run(const char* tag, const std::vector<double>& file) {
  const int N = kN;
  std::vector<float> a((size_t)N * 18), obs((size_t)N * 66), rew(N), to(N);
  std::vector<int64_t> done(N);
  int bad = 0;
  const long tog0 = nm::nm_emul_together();
  for (int pop = 0; pop < kPops; pop++) {
    EmuX<real> e(N, 2, 5);
    const double* p = file.data() + (size_t)pop * kN * kState;
    auto take = [&](std::vector<real>& dst) { for (auto& x : dst) x = (real)*p++; };
    take(e.qpos); take(e.qvel); take(e.qwarm); take(e.dofpos); take(e.dofvel); take(e.act); take(e.cmd);
    for (auto& x : a) x = (float)*p++;
    if (e.template set_kind<nmrows::WrenchKind>(p)) return 1;
    p += N * 8;
    if (e.template set_kind<nmrows::BodyKind>(p)) return 1;
    if (e.step(a.data(), nullptr, obs.data(), rew.data(), done.data(), to.data(), 2, 0, -1)) return 1;
    for (float x : obs) bad += !std::isfinite(x);
    for (float x : rew) bad += !std::isfinite(x);
    for (real x : e.qpos) bad += !std::isfinite((double)x);
    for (real x : e.qvel) bad += !std::isfinite((double)x);
  }
  const long tog = nm::nm_emul_together() - tog0;
  std::printf("%s: non-finite values %d, two-env constraint passes %ld\n", tag, bad, tog);
  return bad != 0 || tog == 0;
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
