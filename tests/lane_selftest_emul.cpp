// The lane self-test of the lean kernel's helper forms (nightmare_rl_amd/csrc/nm_lane_selftest.h) on the host SIMT emulation of simt.h:
// the same lines the device kernel k_lane_selftest runs, 64 values per wave, zeros behind n. Built by tests/test_lane_helpers.py.
#define NM_EMUL
#include "../nightmare_rl_amd/csrc/nm_lane_selftest.h"

extern "C" int lane_selftest_emul(const float* x, const float* a, const float* g, const uint64_t* masks, int n, float* out) {
  using namespace nm;
  for (int w = 0; w * NM_WAVE < n; w++) {
    V<float> xv(0.f), av(0.f), gv(0.f), o0[kLaneSlots], o1[kLaneSlots];
    for (int l = 0; l < NM_WAVE; l++) {
      const int i = w * NM_WAVE + l;
      if (i < n) { xv.v[l] = x[i]; av.v[l] = a[i]; gv.v[l] = g[i]; }
    }
    lane_selftest_wave<float>(xv, av, gv, masks, o0, o1);
    for (int s = 0; s < kLaneSlots; s++)
      for (int l = 0; l < NM_WAVE; l++) {
        const int i = w * NM_WAVE + l;
        if (i < n) { out[(size_t)s * n + i] = o0[s].v[l]; out[(size_t)(kLaneSlots + s) * n + i] = o1[s].v[l]; }
      }
  }
  return 0;
}
