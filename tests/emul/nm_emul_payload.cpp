// nm_emul_payload.cpp - TEST SCAFFOLDING: the host emulation of the device kernel source (see nm_emul.cpp) with the per-env body rows
// of a base payload exposed (level 2 of the step, nm_core.h env_mu): [N,20] rows behind the N friction / gain rows of nm::Args::envp, as
// the host object lays them out, or none. A shim of its own, so that nm_emul.cpp and nm_emul_envp.cpp stay what they were. Never linked
// into the product library.
//
// With -DNM_EMUL_PAYLOAD_MAIN the file is a stand-alone program (for sanitizer builds, which must not be loaded into Python): it steps a
// mixed batch of the three populations the payload tests use - dropped with random actions, standing, flat on the belly - from start
// states and body rows it reads from a file, and prints what ran; exit status 0 = every result finite, the two-env constraint pass and
// the matrix-free layout both taken.
#define NM_EMUL 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../nightmare_rl_amd/csrc/nm_host_model.h"

template <class real> struct EmuP {
  int N;
  nmhost::Tables<real> T;
  nm::Model<real> M;
  std::vector<real> qpos, qvel, qwarm, dofpos, dofvel, act, cmd, epsum, feetair, envp;
  std::vector<int64_t> ep;
  std::vector<uint32_t> ctr;
  std::vector<int> hcache, feetflags;
  bool envp_on = false, body_on = false;
  uint64_t seed;
  int64_t off;
  int G;
  EmuP(int n, uint64_t s, int64_t o, int g) : N(n), seed(s), off(o), G(g) {
    T.build();
    nmhost::EnvConfig cfg;
    T.fill_scalars(M, cfg);
    M.hullv = T.hullv.data(); M.hullnv = T.hullnv.data();
    const size_t n_ = (size_t)N;
    qpos.assign(n_ * 25, 0); qvel.assign(n_ * 24, 0); qwarm.assign(n_ * 24, 0); dofpos.assign(n_ * 18, 0); dofvel.assign(n_ * 18, 0);
    act.assign(n_ * 18, 0); cmd.assign(n_ * 3, 0); epsum.assign(n_ * nm::kNREW, 0); feetair.assign(n_ * 6, 0); envp.assign(n_ * (nm::kEnvP + nm::kBodyP), 0);
    ep.assign(N, 0); ctr.assign(N, 0); hcache.assign(n_ * 8, 0); feetflags.assign(N, 0);
    for (size_t i = 0; i < n_; i++)
      for (int j = 0; j < 25; j++) qpos[i * 25 + j] = T.qpos0[j];
  }
  std::vector<real>* arr(int what) {
    switch (what) {
      case 0: return &qpos; case 1: return &qvel; case 2: return &qwarm; case 3: return &dofpos; case 4: return &dofvel;
      case 5: return &act; case 6: return &cmd; case 7: return &epsum;
    }
    return nullptr;
  }
  void set_envp(const double* rows) {   // [N,3] (mu, p_gain, kv) or null = the model's values in every row
    envp_on = rows != nullptr;
    const double dflt[3] = {(double)M.mu, (double)M.p_gain, (double)M.kv};
    for (int i = 0; i < N; i++) {
      for (int k = 0; k < 3; k++) envp[(size_t)i * nm::kEnvP + k] = rows ? (real)rows[i * 3 + k] : (real)dflt[k];
      envp[(size_t)i * nm::kEnvP + 3] = real(0);
    }
  }
  void set_body(const double* rows) {   // [N,20] body rows or null = off
    body_on = rows != nullptr;
    if (!envp_on) set_envp(nullptr);
    if (rows)
      for (size_t i = 0; i < (size_t)N * nm::kBodyP; i++) envp[(size_t)N * nm::kEnvP + i] = (real)rows[i];
  }
  void default_row(double* out) const {   // what nm_get_body_params reports while the feature is off
    for (int j = 0; j < nm::kBodyP; j++) out[j] = 0;
    for (int j = 0; j < 10; j++) out[nm::BP_IPOS + j] = (double)M.basec[j];
    out[nm::BP_TOTAL] = (double)M.total_mass;
    for (int g = 0; g < nm::kNCOL; g++) out[nm::BP_INVW + g] = (double)M.colc[g * nm::kColN + 4];
    out[nm::BP_PGS] = (double)M.pgs_scale;
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
    A.envp = envp_on || body_on ? envp.data() : nullptr;
    // as the host does: level 2 of the step while body rows are set, level 1 while only friction / gain rows are, the default otherwise
    const int level = body_on ? 2 : (A.envp ? 1 : 0);
    if (G == 1) {
      static thread_local nm::ShWB<real, 1> sh;
      for (int wv = 0; wv < N; wv++) {
        if (level == 2) nm::wave_step<real, 1, 2>(sh.w, M, A, wv);
        else if (level == 1) nm::wave_step<real, 1, 1>(sh.w, M, A, wv);
        else nm::wave_step<real, 1>(sh.w, M, A, wv);
      }
    } else {
      static thread_local nm::ShWB<real, 2> sh;
      for (int wv = 0; wv * 2 < N; wv++) {
        if (level == 2) nm::wave_step<real, 2, 2>(sh.w, M, A, wv);
        else if (level == 1) nm::wave_step<real, 2, 1>(sh.w, M, A, wv);
        else nm::wave_step<real, 2>(sh.w, M, A, wv);
      }
    }
    if (dbg) for (size_t i = 0; i < dbgr.size(); i++) dbg[i] = (double)dbgr[i];
  }
};

#ifndef NM_EMUL_PAYLOAD_MAIN
namespace {
struct Base {
  virtual ~Base() {}
  virtual void get(int what, double* out) = 0;
  virtual void set(int what, const double* in) = 0;
  virtual void set_envp(const double* rows) = 0;
  virtual void set_body(const double* rows) = 0;
  virtual void default_row(double* out) = 0;
  virtual int64_t* eplen() = 0;
  virtual void step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) = 0;
};
template <class real> struct Impl : Base {
  EmuP<real> e;
  Impl(int n, uint64_t s, int64_t o, int g) : e(n, s, o, g) {}
  void get(int what, double* out) override { auto* a = e.arr(what); for (size_t i = 0; i < a->size(); i++) out[i] = (double)(*a)[i]; }
  void set(int what, const double* in) override { auto* a = e.arr(what); for (size_t i = 0; i < a->size(); i++) (*a)[i] = (real)in[i]; }
  void set_envp(const double* rows) override { e.set_envp(rows); }
  void set_body(const double* rows) override { e.set_body(rows); }
  void default_row(double* out) override { e.default_row(out); }
  int64_t* eplen() override { return e.ep.data(); }
  void step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) override {
    e.step(actions, cmd_u, obs, rew, done, to, nsub, physics_only, dbg);
  }
};
}  // namespace

extern "C" {
void* emub_create(int N, int use_double, uint64_t seed, int64_t env_off, int envs_per_wave) {
  if (use_double) return new Impl<double>(N, seed, env_off, envs_per_wave);
  return new Impl<float>(N, seed, env_off, envs_per_wave);
}
void emub_destroy(void* h) { delete (Base*)h; }
void emub_step(void* h, const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only, double* dbg) {
  ((Base*)h)->step(actions, cmd_u, obs, rew, done, to, nsub, physics_only, dbg);
}
void emub_get(void* h, int what, double* out) { ((Base*)h)->get(what, out); }
void emub_set(void* h, int what, const double* in) { ((Base*)h)->set(what, in); }
void emub_set_envp(void* h, const double* rows3) { ((Base*)h)->set_envp(rows3); }
void emub_set_body(void* h, const double* rows20) { ((Base*)h)->set_body(rows20); }
void emub_default_row(void* h, double* out20) { ((Base*)h)->default_row(out20); }
int64_t* emub_eplen(void* h) { return ((Base*)h)->eplen(); }
long emub_together_count() { return nm::nm_emul_together(); }
int emub_dbg_n() { return nm::kDbgN; }
}
#else
// ---- the stand-alone program:  <program> <states file>
// The file holds raw doubles: the body rows of the four payload sets [4*20], then per population (three of them: dropped, standing, flat
// on the belly) one start state of N = 8 envs:
// qpos[N*25] qvel[N*24] qacc_warmstart[N*24] dof_pos[N*18] dof_vel[N*18] previous actions[N*18] commands[N*3] actions[N*18]
// (the test writes it from its fixture). One mixed-batch step of each population, fp32 and fp64.
template <class real> static int run(const char* tag, const std::vector<double>& file) {
  const int N = 8, kPer = N * (25 + 24 + 24 + 18 + 18 + 18 + 3 + 18);
  std::vector<double> rows((size_t)N * nm::kBodyP);
  for (int i = 0; i < N; i++)
    for (int k = 0; k < nm::kBodyP; k++) rows[i * nm::kBodyP + k] = file[((i + i / 4) % 4) * nm::kBodyP + k];   // neighbours in a wave always hold different sets
  std::vector<float> a((size_t)N * 18), obs((size_t)N * 66), rew(N), to(N);
  std::vector<int64_t> done(N);
  std::vector<double> dbg((size_t)N * nm::kDbgN);
  int bad = 0, big = 0;
  const long tog0 = nm::nm_emul_together();
  for (int pop = 0; pop < 3; pop++) {
    EmuP<real> e(N, 3, 0, 2);
    e.set_body(rows.data());
    const double* p = file.data() + 4 * nm::kBodyP + (size_t)pop * kPer;
    auto take = [&](std::vector<real>& dst) { for (auto& x : dst) x = (real)*p++; };
    take(e.qpos); take(e.qvel); take(e.qwarm); take(e.dofpos); take(e.dofvel); take(e.act); take(e.cmd);
    for (auto& x : a) x = (float)*p++;
    e.step(a.data(), nullptr, obs.data(), rew.data(), done.data(), to.data(), 2, 0, dbg.data());
    for (float x : obs) bad += !std::isfinite(x);
    for (float x : rew) bad += !std::isfinite(x);
    for (real x : e.qpos) bad += !std::isfinite((double)x);
    for (real x : e.qvel) bad += !std::isfinite((double)x);
    for (int i = 0; i < N; i++) big += dbg[(size_t)i * nm::kDbgN + 160] > nm::kMaxCon;
  }
  const long tog = nm::nm_emul_together() - tog0;
  std::printf("%s: non-finite values %d, two-env constraint passes %ld, envs in the matrix-free layout %d\n", tag, bad, tog, big);
  return bad != 0 || tog == 0 || big == 0;
}
int main(int argc, char** argv) {
  const size_t want = 4 * nm::kBodyP + 3 * 8 * (25 + 24 + 24 + 18 + 18 + 18 + 3 + 18);
  std::vector<double> file(want);
  FILE* f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
  if (!f || std::fread(file.data(), sizeof(double), want, f) != want) { std::fprintf(stderr, "usage: %s <states file>\n", argv[0]); return 2; }
  std::fclose(f);
  const int r32 = run<float>("fp32", file), r64 = run<double>("fp64", file);
  return r32 | r64;
}
#endif
