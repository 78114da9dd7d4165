// nm_step_kernel.h - k_env_step, the kernel of nm_step, and the closing wave's step_tail. A header, because the kernel is compiled in two
// translation units: nm_hip.hip holds the generic instantiations (every level of per-env rows, both dtypes, configuration asked at run
// time - nm::CfgAsk) and launches them; nm_step_lean.hip holds the one instantiation for the shipped default configuration
// (nm::CfgLean) behind nm_launch_step_lean(). Two units for the reason the K-step kernels have their own: a further kernel around
// nm::wave_step in one unit changes the register allocation of the others.
#pragma once
#include <hip/hip_runtime.h>

#include "nm_core.h"
#include "nm_env_loop.h"

// ------------------------------------------------------------------------------------------------ kernels
// One 64-lane wavefront per NM_ENVS_PER_WAVE (2) envs, one wave per workgroup: LDS image private to the wave, no inter-wave sync.
#ifndef NM_WAVES_PER_SIMD
#define NM_WAVES_PER_SIMD 2  /* the step kernel needs ~250 VGPRs (row-per-lane A matrix): 2 waves per SIMD; a 4-wave budget spills */
#endif
#ifndef NM_ENVS_PER_WAVE
#define NM_ENVS_PER_WAVE 2
#endif
// extras: like the reference, 'episode' and 'time_outs' are refreshed only by a step in which >= 1 env reset (env.py:344-371);
// then the per-step accumulators are cleared for the next launch. One wave, after all others have published.
// (`src` by value: one pointer in registers, nothing through the stack)
template <class real, class Src> __device__ __noinline__ void step_tail(Src src, real ep_len_s) {
  const nm::Args<real>& A = nm::launch_args(nm::scalar_src(src));
  const int lane = NM_TID;
  // This runs behind the launch's last wave, alone: every global access is a full round trip that nothing hides. So the reads are
  // issued in two batches - everything that is addressed by the lane alone, then the two lists those counts index - not one by one.
#define TAIL_LD(p) __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
  const int cnt = TAIL_LD(A.stat_cnt);
  const int c1 = TAIL_LD(A.stat_cnt + 1), c2 = TAIL_LD(A.stat_cnt + 2);
  const real ssum = TAIL_LD(A.stat_sum + (lane < nm::kNREW ? lane : 0));
  const int n = TAIL_LD(A.nto);
  const int np = TAIL_LD(A.nprev);
  // decided on the device, so that it also holds for a launch replayed from a graph: is this the buffer the last refresh wrote?
  const bool to_full = A.time_outs && TAIL_LD(A.to_owner) != (unsigned long long)(uintptr_t)A.time_outs;
  const long long k0 = lane == 0 ? A.counters[0] : 0, k1 = lane == 0 ? A.counters[1] : 0;
  if (cnt > 0) {
    if (lane < nm::kNREW && A.ep_stats) A.ep_stats[lane] = (float)(ssum / (real)cnt / ep_len_s);
    if (A.time_outs) {
      // extras['time_outs'] = this step's time-out flags (a subset of the resets). The buffer still holds what the last refresh
      // wrote, so only the entries that were 1 are cleared and the new ones set: O(time-outs) instead of N stores.
      // A buffer other than the one the last refresh wrote (to_full) is rewritten completely.
      const int e_new = lane < n ? TAIL_LD(A.to_list + lane) : -1;
      const int e_old = (!to_full && lane < np) ? A.to_prev[lane] : -1;
      if (to_full) {
        for (int i = lane; i < A.N; i += 64) A.time_outs[i] = 0.f;
      } else {
        if (e_old >= 0) A.time_outs[e_old] = 0.f;
        for (int j = lane + 64; j < np; j += 64) A.time_outs[A.to_prev[j]] = 0.f;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the zeros have reached L2 before a one goes to the same address
      if (e_new >= 0) { A.time_outs[e_new] = 1.f; A.to_prev[lane] = e_new; }
      for (int j = lane + 64; j < n; j += 64) {
        const int e = TAIL_LD(A.to_list + j);
        A.time_outs[e] = 1.f;
        A.to_prev[j] = e;
      }
      if (lane == 0) { *A.nprev = n; *A.to_owner = (unsigned long long)(uintptr_t)A.time_outs; }
    }
  }
#undef TAIL_LD
  if (lane < nm::kNREW) A.stat_sum[lane] = real(0);
  if (lane == 0) {
    A.counters[0] = k0 + c1;
    A.counters[1] = k1 + c2;
    A.stat_cnt[0] = 0; A.stat_cnt[1] = 0; A.stat_cnt[2] = 0; A.stat_cnt[3] = 0;
    *A.nto = 0;
    A.wave_done[nm::kTicketTop] = 0;
  }
}

// Waves per workgroup: 1 by default (LDS image private to the wave, no inter-wave synchronisation at all). -DNM_WG_WAVES=w (measurement,
// DESIGN.md 6.1) packs w waves into one workgroup - w times fewer workgroups for the dispatcher to start - with wave-private env images and
// ONE shared copy of the model constants and of the launch arguments; the two barriers of the start-up are then real workgroup barriers.
#ifdef NM_WG_WAVES
constexpr int kWG = NM_WG_WAVES;
#else
constexpr int kWG = 1;
#endif
// EP: level of per-env physics parameters (nm_core.h env_mu): 0 none, 1 friction / gain rows (nm::Args::envp), 2 those and body rows, 3 those
// and actuation latency, 4 those and gravity rows, 5 those and the servo target model, 6 those and the servo torque
// limit, 7 those and the external wrench on the base - the host launches a level above 0 only while its rows are set
//
// The launch arguments are read where they are used, by scalar loads from the kernel's own kernarg segment (nm::KernArgs): the wave's
// first instructions are the loads of the base pointers and then the env rows' HBM reads, the epilogue fetches its pointers again from
// the scalar cache, and nothing of them is live across the physics. (Until DESIGN.md 6.13 the kernel copied them into LDS first, like
// the K-step kernels, which edit their copy between steps: ~150 issue slots, a barrier and two LDS round trips in front of the first
// HBM request.) `A` is the second explicit argument, so it starts at byte 8 of the segment.
struct NoArgsCopy {};
template <class real> __device__ __forceinline__ nm::KernArgs<real, 8> step_src(NoArgsCopy&) { return {(nm::kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr()}; }
template <class real> __device__ __forceinline__ const nm::Args<real>& step_src(nm::Args<real>& a) { return a; }
// Cfg: who answers the stages' questions about the env's configuration (nm_core.h): nm::CfgAsk at run time, nm::CfgLean at compile time.
template <class real, int G, int EP, class Cfg = nm::CfgAsk>
__global__ void __launch_bounds__(64 * (sizeof(real) == 8 ? 1 : kWG), NM_WAVES_PER_SIMD) k_env_step(const nm::Model<real>* __restrict__ Mp, nm::Args<real> A) {
  constexpr int kWG = sizeof(real) == 8 ? 1 : ::kWG;     // the fp64 verification build keeps one wave per workgroup
  static_assert(sizeof(Mp) == 8 && alignof(nm::Args<real>) == 8, "k_env_step: Args starts at byte 8 of the kernarg segment");
  __shared__ typename nm::ShWSel<real, G, EP>::type shs[kWG];
  __shared__ nm::ModelBlock<real> Mb;   // this workgroup's copy of the model constants
  const nm::Model<real>& Ms = Mb.m;
  // The fp64 verification build keeps the copy in LDS: read from the kernarg segment its kernels spill 14 more scalar registers (71 for 57).
  constexpr bool kKern = sizeof(real) == 4;
  __shared__ std::conditional_t<kKern, NoArgsCopy, nm::Args<real>> As;
  decltype(auto) KA = step_src<real>(As);
  nm::ShW<real, G>& sh = nm::ShWSel<real, G, EP>::images(shs[kWG == 1 ? 0 : (int)(threadIdx.x >> 6)]);
  if constexpr (kKern) nm::launch_args_touch(KA);
  else { As = A; __syncthreads(); }
  int wave;
  unsigned long long t_start = 0ull;
  {  // what the kernel's own first lines need, in one batch of scalar loads; nothing of it but `wave` and the debug clock lives on
    const nm::Args<real>& A0 = nm::launch_args(KA);
    const int N = A0.N, nxcd = A0.nxcd;
    const bool dbg_on = nm::cfg_opt<Cfg>(A0.dbg) != nullptr;
#ifdef NM_MEASURE
    if (A0.ablate & 512) return;      // measurement only: the empty launch
#endif
    wave = nmr::wave_index(nxcd);      // XCD-aware block -> wave mapping (nm_env_loop.h)
    if (kWG > 1) wave = wave * kWG + (int)(threadIdx.x >> 6);
    if (dbg_on) t_start = __builtin_amdgcn_s_memtime();
    if (wave * G >= N) return;       // (a wave that has left does not count for the barrier of the model copy below; only -DNM_WG_WAVES has one)
  }
  // the model copy (L2 -> LDS) runs inside the load stage, after the env rows' HBM reads have been issued: one start-up round trip, not two.
  // The block is padded to whole rounds of 64 lanes x 16 bytes on both sides (nm::ModelBlock), so every lane moves 16 bytes per round
  // and no round tests a bound.
  auto copy_model = [&]() {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    constexpr int kRounds = (int)(sizeof(nm::ModelBlock<real>) / (64 * 16));
    const NM_GLOBAL(u4)* src = (const NM_GLOBAL(u4)*)Mp;
    u4* dst = reinterpret_cast<u4*>(&Mb);
    u4 tmp[kRounds];
#pragma unroll
    for (int k = 0; k < kRounds; k++) tmp[k] = src[NM_TID + 64 * k];
    if (kWG == 1 || threadIdx.x < 64) {     // one wave fills the workgroup's copy
#pragma unroll
      for (int k = 0; k < kRounds; k++) dst[NM_TID + 64 * k] = tmp[k];
    }
    if (kWG == 1) nm::wave_sync(); else __syncthreads();
  };
  // Two-level ticket for "which wave closes the step": waves draw from their group's counter, the last wave of a group from the top
  // counter - at most 64 + 32 same-address atomics in a row instead of gridDim.x. A wave draws its group ticket as soon as everything
  // it contributes to the bookkeeping is published (inside the epilogue, before rewards and observation), so the round trip of that
  // atomic is off the critical path of the wave that finishes last.
  const int grp = wave / nm::kTicketGroup;
  int ticket = 0, top = 0;
  int stage = 0;                       // 0: nothing drawn, 1: group ticket drawn, 2: group ticket resolved (and the top one drawn if this wave closes its group)
  bool closes_group = false;
  auto draw = [&](int phase) {
#ifdef NM_NO_TICKETS   // measurement only (results without extras): what the end-of-step tickets cost
    stage = 2; (void)phase; return;
#endif
    const nm::Args<real>& Ad = nm::launch_args(KA);
    int* wave_done = Ad.wave_done;
    if (phase == 0) {
      if (NM_TID == 0) ticket = atomicAdd(wave_done + (grp + 1) * nm::kTicketStride, 1);
      stage = 1;
    } else {
      const int nw = (Ad.N + G - 1) / G, gsize = min(nm::kTicketGroup, nw - grp * nm::kTicketGroup);
      closes_group = __builtin_amdgcn_readfirstlane(ticket) == gsize - 1;
      if (closes_group && NM_TID == 0) {
        wave_done[(grp + 1) * nm::kTicketStride] = 0;     // every member has drawn: re-arm for the next launch
        top = atomicAdd(wave_done + nm::kTicketTop, 1);
      }
      stage = 2;
    }
  };
  nm::wave_step<real, G, EP>(sh, Ms, KA, wave, copy_model, draw, Cfg());
  const nm::Args<real>& A1 = nm::launch_args(KA);
  if (nm::cfg_opt<Cfg>(A1.dbg) && NM_TID == 0) {   // debug buffer only: start / end clock of this wave as exact 24-bit pieces (scripts/wavetimes.py)
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    real* d = A1.dbg + (size_t)(wave * G) * nm::kDbgN + 250;
    d[0] = (real)(unsigned)(t_start & 0xFFFFFF); d[1] = (real)(unsigned)((t_start >> 24) & 0xFFFFFF);
    d[2] = (real)(unsigned)(t_end & 0xFFFFFF); d[3] = (real)(unsigned)((t_end >> 24) & 0xFFFFFF);
    // where the wave ran: HW_ID (hwreg 4: wave[3:0] simd[5:4] pipe[7:6] cu[11:8] sh[12] se[15:13]) and XCC_ID (hwreg 20)
    d[4] = (real)(__builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11)) & 0xFFFF);
    d[5] = (real)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 0xF);
  }
  if (nm::cfg_flag<Cfg>(A1.physics_only)) return;
  // The wave that finishes last closes the step (what used to be a second launch). What it needs from the others went through
  // device-scope atomics whose results each wave has already consumed (nm_consume), so the tickets need no fence.
  if (stage < 1) draw(0);              // paths that do not run the two-env epilogue draw here
  if (stage < 2) draw(1);
  if (!closes_group) return;
  const int ngrp = ((A1.N + G - 1) / G + nm::kTicketGroup - 1) / nm::kTicketGroup;
  if (__builtin_amdgcn_readfirstlane(top) != ngrp - 1) return;
#ifndef NM_SKIP_TAIL2
  if constexpr (kKern) step_tail<real>(KA, Ms.ep_len_s);
  else step_tail<real>(&As, Ms.ep_len_s);
#endif
}

// The lean instantiation k_env_step<float, 2, 0, nm::CfgLean> (nm_step_lean.hip), one wave per workgroup: launched by nm_step for
// level 0 of the per-env rows while nm::lean_config() holds for the launch. Returns what hipGetLastError() gives after the launch.
hipError_t nm_launch_step_lean(int N, hipStream_t s, const nm::Model<float>* M_dev, const nm::Args<float>& a);
