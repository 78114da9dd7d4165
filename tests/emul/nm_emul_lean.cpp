// nm_emul_lean.cpp - TEST SCAFFOLDING: the host SIMT emulation of nm_emul.cpp with one more env type whose step runs nm::wave_step on
// the lean configuration traits (nm::CfgLean: every question about the configuration answered at compile time, as in the kernel of
// nightmare_rl_amd/csrc/nm_step_lean.hip). The generic emulation is the included file's, unchanged, so one library steps both and a
// test can hold them against each other. A lean step refuses what the host refuses for the lean kernel (nm::lean_config).
#include "nm_emul.cpp"

namespace {
struct EmuLean : Emu<float> {
  int refused = 0;       // steps that did not run because the configuration or the optional inputs are not the lean ones
  EmuLean(int n, uint64_t s, int64_t o) : Emu<float>(n, s, o, 2) {}
  void step(const float* actions, const double* cmd_u, float* obs, float* rew, int64_t* done, float* to, int nsub, int physics_only,
            double* dbg, double* stat_sum, int* stat_cnt) override {
    std::vector<float> ssum(nm::kNREW, 0);
    int scnt[4] = {0, 0, 0, 0};
    nm::Args<float> A{};
    A.N = N; A.seed = seed; A.env_offset = off;
    A.qpos = qpos.data(); A.qvel = qvel.data(); A.qwarm = qwarm.data(); A.dofpos = dofpos.data(); A.dofvel = dofvel.data();
    A.act = act.data(); A.cmd = cmd.data(); A.epsum = epsum.data(); A.feetair = feetair.data(); A.feetflags = feetflags.data(); A.eplen = ep.data(); A.rngctr = ctr.data(); A.hullcache = hcache.data();
    A.actions = actions;
    A.obs = obs; A.rew = rew; A.timeout_now = to; A.done = done; A.stat_sum = ssum.data(); A.stat_cnt = scnt;
    A.nsub = nsub; A.physics_only = physics_only;
    if (cmd_u || dbg || !nvec.empty() || rec_env >= 0 || !nm::lean_config(M, A)) { refused++; return; }
    nstep++;
    static thread_local nm::ShW<float, 2> sh;
    for (int wv = 0; wv * 2 < N; wv++) nm::wave_step<float, 2, 0, nm::NoMid, nm::NoMid, nm::Args<float>, nm::CfgLean>(sh, M, A, wv);
    if (stat_sum) for (int k = 0; k < nm::kNREW; k++) stat_sum[k] = (double)ssum[k];
    if (stat_cnt) { stat_cnt[0] = scnt[0]; stat_cnt[1] = scnt[1]; }
  }
};
}  // namespace

extern "C" {
void* emul_create(int N, uint64_t seed, int64_t env_off) { return new EmuLean(N, seed, env_off); }
int emul_refused(void* h) { return ((EmuLean*)h)->refused; }
}
