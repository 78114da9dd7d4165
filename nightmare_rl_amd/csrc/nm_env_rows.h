// nm_env_rows.h - host side, plain C++17, no HIP header: the one owner of what the host decides about the per-env rows behind
// nm::Args::envp - layout, default rows, admission, which kinds are on and which level of the step a launch takes. Used by the env object
// (nm_hip.hip), the K-step launchers and the host emulation (tests/emul, -DNM_EMUL).
//
// The invariant every owner of a block keeps: ONCE THE BLOCK IS ALLOCATED, EVERY REGION WHOSE KIND IS OFF HOLDS THAT KIND'S DEFAULTS -
// default friction / gain rows, default body rows, zero delays, default gravity, servo and torque rows, zero wrench rows - so a transition
// writes or refills its own region and looks at no other kind's flag. The action history and the servo's limited targets are exempt: they
// are state, not parameters, and keep what they hold.
#pragma once
#include <cmath>
#include <cstddef>
#include <string>
#include <type_traits>

#include "nm_core.h"

namespace nmrows {

enum Kind { kFric = 0, kBody = 1, kLat = 2, kGrav = 3, kServo = 4, kTorque = 5, kWrench = 6 };      // kWrench lies outside the pooled range [0, kKinds)

// ---- layout: ONE block, the regions below in this order, as byte offsets from the base. The device walks it through nm::lat_delay /
// lat_hist / grav_rows_of / servo_rows_of / servo_state_of / torque_rows_of / wrench_rows_of / wrench_args_of (nm_core.h); tests/emul
// checks every one of them, and that the regions tile the block.
constexpr size_t hist_words(size_t N) { return N * nm::kLatH * nm::kNU; }
struct Layout { size_t fric, body, delays, hist, pad, grav, servo, servo_state, torque, wrench, wrench_args, total; };
template <class real> constexpr Layout layout(size_t N) {
  constexpr size_t R = sizeof(real);
  static_assert(nm::kLatP == 1 + nm::kLatH * nm::kNU && nm::kWrenchArgBytes % R == 0, "the latency words and the wrench arguments as the device counts them");
  Layout L{};                                         // fric: N friction / gain rows of kEnvP reals
  L.body = L.fric + N * nm::kEnvP * R;                // N body rows of kBodyP reals (base payload)
  L.delays = L.body + N * nm::kBodyP * R;             // N ints: actuation latency in substeps
  L.hist = L.delays + N * sizeof(int);                // N x kLatH x kNU floats: the action history (state)
  L.pad = L.hist + hist_words(N) * sizeof(float);     // up to the next multiple of sizeof(real): 4 bytes in fp64 with an odd N, else empty
  L.grav = (L.pad + R - 1) / R * R;                   // N gravity rows of kGravP reals
  L.servo = L.grav + N * nm::kGravP * R;              // N servo rows of kServoP reals
  L.servo_state = L.servo + N * nm::kServoP * R;      // N x kNU reals: the servo's limited targets (state)
  L.torque = L.servo_state + N * nm::kNU * R;         // N torque rows of kTorqueP reals
  L.wrench = L.torque + N * nm::kTorqueP * R;         // N wrench rows of kWrenchP reals
  L.wrench_args = L.wrench + N * nm::kWrenchP * R;    // kWrenchArgBytes: the schedule parameters of a K-step launch (zero = no schedule)
  L.total = L.wrench_args + nm::kWrenchArgBytes;
  return L;
}
// the block sizes, in reals: the whole block (wrench_block_reals, what every owner allocates) and its prefixes that end in front of the
// servo, the torque and the wrench regions. No owner allocates a prefix any more: the three prefix sizes are named only by the emulation
// shims of earlier commits and by layout_agrees() (tests/emul), and are to be deleted together with that clause
template <class real> constexpr size_t block_reals(size_t N) { return layout<real>(N).servo / sizeof(real); }
template <class real> constexpr size_t servo_block_reals(size_t N) { return layout<real>(N).torque / sizeof(real); }
template <class real> constexpr size_t torque_block_reals(size_t N) { return layout<real>(N).wrench / sizeof(real); }
template <class real> constexpr size_t wrench_block_reals(size_t N) { return layout<real>(N).total / sizeof(real); }
template <class T, class real> inline T* region(real* base, size_t bytes) { return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + bytes); }
template <class real> inline real* fric_rows(real* base, int N) { return region<real>(base, layout<real>(N).fric); }
template <class real> inline real* body_rows(real* base, int N) { return region<real>(base, layout<real>(N).body); }
template <class real> inline int* delays(real* base, int N) { return region<int>(base, layout<real>(N).delays); }
template <class real> inline float* histories(real* base, int N) { return region<float>(base, layout<real>(N).hist); }
template <class real> inline real* grav_rows(real* base, int N) { return region<real>(base, layout<real>(N).grav); }
template <class real> inline real* servo_rows(real* base, int N) { return region<real>(base, layout<real>(N).servo); }
template <class real> inline real* servo_state(real* base, int N) { return region<real>(base, layout<real>(N).servo_state); }
template <class real> inline real* torque_rows(real* base, int N) { return region<real>(base, layout<real>(N).torque); }
template <class real> inline real* wrench_rows(real* base, int N) { return region<real>(base, layout<real>(N).wrench); }
template <class real> inline void* wrench_args(real* base, int N) { return region<void>(base, layout<real>(N).wrench_args); }

// ---- default rows: the model's own values (the fourth word of a friction / gain row is padding, zero)
template <class real> inline void fric_default(const nm::Model<real>& M, real out[3]) {
  out[nm::EP_MU] = M.mu; out[nm::EP_PGAIN] = M.p_gain; out[nm::EP_KV] = M.kv;
}
template <class real> inline void body_default(const nm::Model<real>& M, real out[nm::kBodyP]) {
  for (int j = 0; j < nm::kBodyP; j++) out[j] = real(0);
  for (int j = 0; j < 10; j++) out[nm::BP_IPOS + j] = M.basec[j];
  out[nm::BP_TOTAL] = M.total_mass;
  for (int g = 0; g < nm::kNCOL; g++) out[nm::BP_INVW + g] = M.colc[g * nm::kColN + 4];
  out[nm::BP_PGS] = M.pgs_scale;
}

// g and gravity_vec both the model's (0, 0, -gravity); the pads zero
template <class real> inline void grav_default(const nm::Model<real>& M, real out[nm::kGravP]) {
  for (int j = 0; j < nm::kGravP; j++) out[j] = real(0);
  out[nm::GP_G + 2] = -M.grav; out[nm::GP_VEC + 2] = -M.grav;
}

// no limit, no damping: level 5 then commands as level 4 does
template <class real> inline void servo_default(const nm::Model<real>&, real out[nm::kServoP]) {
  for (int j = 0; j < nm::kServoP; j++) out[j] = real(0);
  out[nm::SV_RATE] = (real)INFINITY;
}

// no limit on any joint: level 6 then computes what level 5 does
template <class real> inline void torque_default(const nm::Model<real>&, real out[nm::kTorqueP]) {
  for (int j = 0; j < 3; j++) out[j] = (real)INFINITY;
  out[3] = real(0);
}

// no force, no torque: level 7 then computes what level 6 does
template <class real> inline void wrench_default(const nm::Model<real>&, real out[nm::kWrenchP]) {
  for (int j = 0; j < nm::kWrenchP; j++) out[j] = real(0);
}

// ---- admission: pure functions of the caller's rows; empty = admitted, otherwise what the entry point reports behind its own name
template <class real> inline std::string body_rows_fault(const real* rows, int N) {
  for (int e = 0; e < N; e++) {
    const real* r = rows + (size_t)e * nm::kBodyP;
    const char* why = nullptr;
    for (int j = 0; j < nm::kBodyP; j++) if (!std::isfinite((double)r[j])) why = "a non-finite value";
    if (!why && !(r[nm::BP_MASS] > 0)) why = "mass <= 0";
    if (!why && r[nm::BP_TOTAL] < r[nm::BP_MASS]) why = "total_mass < mass";
    if (!why && !(r[nm::BP_I6] > 0 && r[nm::BP_I6 + 1] > 0 && r[nm::BP_I6 + 2] > 0)) why = "a non-positive inertia diagonal";
    for (int g = 0; g < nm::kNCOL && !why; g++) if (!(r[nm::BP_INVW + g] > 0)) why = "a non-positive invweight0";
    if (!why && !(r[nm::BP_PGS] > 0)) why = "a non-positive pgs_scale";
    if (why) return "row " + std::to_string(e) + ": " + why;
  }
  return std::string();
}
// a zero g is admitted (free float); a zero gravity_vec is not: the termination divides by its norm
template <class real> inline std::string grav_rows_fault(const real* rows, int N) {
  for (int e = 0; e < N; e++) {
    const real* r = rows + (size_t)e * nm::kGravP;
    const char* why = nullptr;
    for (int j = 0; j < nm::kGravP; j++) if (!std::isfinite((double)r[j])) why = "a non-finite value";
    if (!why && r[nm::GP_VEC] == real(0) && r[nm::GP_VEC + 1] == real(0) && r[nm::GP_VEC + 2] == real(0)) why = "a zero gravity_vec";
    if (why) return "row " + std::to_string(e) + ": " + why;
  }
  return std::string();
}
// rate > 0 (+inf = no limit) and not NaN; d_gain finite and >= 0
template <class real> inline std::string servo_rows_fault(const real* rows, int N) {
  for (int e = 0; e < N; e++) {
    const real* r = rows + (size_t)e * nm::kServoP;
    const char* why = nullptr;
    if (!(r[nm::SV_RATE] > 0)) why = "rate not > 0";
    if (!why && !(std::isfinite((double)r[nm::SV_DGAIN]) && r[nm::SV_DGAIN] >= 0)) why = "d_gain not finite and >= 0";
    if (why) return "row " + std::to_string(e) + ": " + why;
  }
  return std::string();
}
// each of the three limits > 0 (+inf = no limit) and not NaN; the pad is not judged
template <class real> inline std::string torque_rows_fault(const real* rows, int N) {
  for (int e = 0; e < N; e++) {
    const real* r = rows + (size_t)e * nm::kTorqueP;
    for (int j = 0; j < 3; j++)
      if (!(r[j] > 0)) return "row " + std::to_string(e) + ": limit " + std::to_string(j) + " not > 0";
  }
  return std::string();
}
// the force and the torque finite; the pads are not judged
template <class real> inline std::string wrench_rows_fault(const real* rows, int N) {
  for (int e = 0; e < N; e++) {
    const real* r = rows + (size_t)e * nm::kWrenchP;
    for (int j = 0; j < 3; j++)
      if (!std::isfinite((double)r[nm::WP_F + j]) || !std::isfinite((double)r[nm::WP_T + j])) return "row " + std::to_string(e) + ": a non-finite value";
  }
  return std::string();
}
inline int delay_max(int nsub) { return nm::kLatH * nsub; }     // the history holds kLatH steps of nsub substeps
inline std::string delays_fault(const int* d, int N, int nsub) {
  for (int e = 0; e < N; e++)
    if (d[e] < 0 || d[e] > delay_max(nsub))
      return "env " + std::to_string(e) + ": delay " + std::to_string(d[e]) + " outside [0, " + std::to_string(delay_max(nsub)) + "] substeps";
  return std::string();
}

// friction / gain rows as envp_write and nm_draw_env_params admit them: finite, mu > 1e-5, gains >= 0; the pad is not judged
template <class real> inline std::string fric_rows_fault(const real* rows, int N) {
  for (int e = 0; e < N; e++) {
    const real* r = rows + (size_t)e * nm::kEnvP;
    const char* why = nullptr;
    for (int j = 0; j < nm::kEnvPS; j++) if (!std::isfinite((double)r[j])) why = "a non-finite value";
    if (!why && !(r[nm::EP_MU] > real(1e-5))) why = "mu must be above 1e-5";
    if (!why && r[nm::EP_PGAIN] < 0) why = "p_gain must not be negative";
    if (!why && r[nm::EP_KV] < 0) why = "kv must not be negative";
    if (why) return "row " + std::to_string(e) + ": " + why;
  }
  return std::string();
}

// ---- descriptors: the kinds that are "N rows of W reals in the env's dtype, set whole, judged on the host" - body, gravity, servo, torque
// and wrench rows - differ in nothing but this. Every owner of a block (the env object, the emulation) has ONE set / get / fill for them,
// written over a descriptor D: D::kind, D::W, D::rows(base, N), D::dflt(M, out[W]), D::fault(rows, N). A new kind of that shape supplies
// its descriptor, its region in the layout above, its place in for_each_row_kind, its entry points, and the device's reads.
template <Kind K> struct RowKind;
template <> struct RowKind<kBody> {
  static constexpr Kind kind = kBody;
  static constexpr int W = nm::kBodyP;
  template <class real> static real* rows(real* base, int N) { return body_rows(base, N); }
  template <class real> static void dflt(const nm::Model<real>& M, real* out) { body_default(M, out); }
  template <class real> static std::string fault(const real* r, int N) { return body_rows_fault(r, N); }
};
template <> struct RowKind<kGrav> {
  static constexpr Kind kind = kGrav;
  static constexpr int W = nm::kGravP;
  template <class real> static real* rows(real* base, int N) { return grav_rows(base, N); }
  template <class real> static void dflt(const nm::Model<real>& M, real* out) { grav_default(M, out); }
  template <class real> static std::string fault(const real* r, int N) { return grav_rows_fault(r, N); }
};
template <> struct RowKind<kServo> {
  static constexpr Kind kind = kServo;
  static constexpr int W = nm::kServoP;
  template <class real> static real* rows(real* base, int N) { return servo_rows(base, N); }
  template <class real> static void dflt(const nm::Model<real>& M, real* out) { servo_default(M, out); }
  template <class real> static std::string fault(const real* r, int N) { return servo_rows_fault(r, N); }
};
template <> struct RowKind<kTorque> {
  static constexpr Kind kind = kTorque;
  static constexpr int W = nm::kTorqueP;
  template <class real> static real* rows(real* base, int N) { return torque_rows(base, N); }
  template <class real> static void dflt(const nm::Model<real>& M, real* out) { torque_default(M, out); }
  template <class real> static std::string fault(const real* r, int N) { return torque_rows_fault(r, N); }
};
template <> struct RowKind<kWrench> {
  static constexpr Kind kind = kWrench;
  static constexpr int W = nm::kWrenchP;
  template <class real> static real* rows(real* base, int N) { return wrench_rows(base, N); }
  template <class real> static void dflt(const nm::Model<real>& M, real* out) { wrench_default(M, out); }
  template <class real> static std::string fault(const real* r, int N) { return wrench_rows_fault(r, N); }
};
typedef RowKind<kBody> BodyKind;
typedef RowKind<kGrav> GravKind;
typedef RowKind<kServo> ServoKind;
typedef RowKind<kTorque> TorqueKind;
typedef RowKind<kWrench> WrenchKind;
// f(D{}) for every descriptor kind in block order, until one returns true (= failed); what an owner fills a new block's defaults through
template <class F> inline bool for_each_row_kind(F&& f) { return f(BodyKind{}) || f(GravKind{}) || f(ServoKind{}) || f(TorqueKind{}) || f(WrenchKind{}); }

// the rows of a reset pool (nm_reset_rows.h) of P rows of `kind`, judged by the rule the kind's own setter applies: `rows` holds P rows of
// the kind's width in `real` - for kLat, P ints. The pooled kinds are the first six: the base wrench (kWrench) has no pool
constexpr int kKinds = 6;
constexpr int kind_width(int kind) {
  return kind == kFric ? nm::kEnvP : kind == kBody ? nm::kBodyP : kind == kLat ? 1 : kind == kGrav ? nm::kGravP : kind == kServo ? nm::kServoP : nm::kTorqueP;
}
template <class real> inline std::string pool_rows_fault(int kind, const void* rows, int P, int nsub) {
  const real* r = static_cast<const real*>(rows);
  switch (kind) {
    case kFric: return fric_rows_fault<real>(r, P);
    case kBody: return BodyKind::fault<real>(r, P);
    case kLat: return delays_fault(static_cast<const int*>(rows), P, nsub);
    case kGrav: return GravKind::fault<real>(r, P);
    case kServo: return ServoKind::fault<real>(r, P);
    default: return TorqueKind::fault<real>(r, P);
  }
}

// ---- state: which kinds are on, and what follows from that for a launch
struct State {
  bool on[7] = {false, false, false, false, false, false, false};
  // the level of the step a launch takes: the highest kind that is on. Latency and the servo target model are not physics: a physics-only
  // launch with latency as the highest kind drops to level 2 (the rows level 3 reads), and at levels 4..7, which physics-only launches
  // take too, the kernel skips the delay, the servo row and its state at run time (nm::Args::physics_only)
  int level(bool physics_only = false) const {
    return on[kWrench] ? 7 : on[kTorque] ? 6 : on[kServo] ? 5 : on[kGrav] ? 4 : (on[kLat] ? (physics_only ? 2 : 3) : (on[kBody] ? 2 : (on[kFric] ? 1 : 0)));
  }
  // nm::Args::envp of a launch: the block while any kind is on, null (level 0 never looks) otherwise
  template <class real> real* envp(real* base) const { return level() ? base : nullptr; }
};

// ---- level dispatch: f(std::integral_constant<int, L>{}) for the level, the one place a run-time level becomes a template argument. Mask
// holds one bit per level that the caller compiles in: f is instantiated for those alone, and a level outside the mask returns false with
// nothing run. A level that is no level at all is taken as level 0. The product passes no mask: every level.
constexpr int kLevels = 8;
constexpr unsigned kAllLevels = (1u << kLevels) - 1;
template <unsigned Mask, int L, class F> inline bool at_level(int level, F& f) {
  if constexpr ((Mask >> L) & 1u)
    if (level == L) { f(std::integral_constant<int, L>{}); return true; }
  return false;
}
template <unsigned Mask = kAllLevels, class F> inline bool with_level(int level, F&& f) {
  if (level < 0 || level >= kLevels) level = 0;
  return at_level<Mask, 7>(level, f) || at_level<Mask, 6>(level, f) || at_level<Mask, 5>(level, f) || at_level<Mask, 4>(level, f) ||
         at_level<Mask, 3>(level, f) || at_level<Mask, 2>(level, f) || at_level<Mask, 1>(level, f) || at_level<Mask, 0>(level, f);
}

}  // namespace nmrows
