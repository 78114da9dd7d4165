// The sensor model's one definition (nightmare_rl_amd/csrc/nm_sensor.h: nm::sensor_apply) on the host build of simt.h, run over a sequence
// of true observations the way k_sensor runs it behind every step: per env the count is read first, then every column is applied.
// Built by tests/test_sensor_emulated.py.
#define NM_EMUL
#include "../nightmare_rl_amd/csrc/nm_sensor.h"

#include <cstring>
#include <vector>

// y [T,N,66], done [T,N], delay [N,2], bias [N,66] -> out [T,N,66]; ring [N,4,66] and count [N] are the history, in and out
extern "C" int sensor_emul(const float* y, const unsigned char* done, const int32_t* delay, const float* bias, float clip_obs, int T, int N,
                           float* out, float* ring, uint32_t* count) {
  using namespace nm;
  std::vector<float> truth((size_t)N * kNOBS);
  SensorDesc D{};
  D.delay = delay; D.bias = bias; D.ring = ring; D.count = count; D.true_obs = truth.data(); D.out = nullptr; D.clip_obs = clip_obs;
  for (int t = 0; t < T; t++) {
    std::memcpy(truth.data(), y + (size_t)t * N * kNOBS, truth.size() * sizeof(float));
    for (int e = 0; e < N; e++) {
      const uint32_t n = count[e];
      for (int c = 0; c < kNOBS; c++) sensor_apply(D, (size_t)e, c, n, done[(size_t)t * N + e] != 0, out + (size_t)t * N * kNOBS);
    }
  }
  return 0;
}
