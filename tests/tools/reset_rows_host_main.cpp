// reset_rows_host_main.cpp - the host functions of nightmare_rl_amd/csrc/nm_reset_rows.h and the pool admission of nm_env_rows.h as a
// stand-alone program (its own main; built with -DNM_EMUL by tests/test_reset_rows_host.py, with -fsanitize=address,undefined): never
// loaded into Python. It prints
//   pick <seed> <genv> <k> <sizes x6> : <index x6>      for the argument sets of the test
//   fault <kind> <dtype> <case> : <text or "ok">        for one admissible and the inadmissible pool rows of every kind
//   map <41 kinds> / first <7 values>                   the lane map
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../nightmare_rl_amd/csrc/nm_env_rows.h"
#include "../../nightmare_rl_amd/csrc/nm_reset_rows.h"

template <class real> static std::vector<real> good_rows(int kind, int P) {
  const int W = nmrows::kind_width(kind);
  std::vector<real> r((size_t)P * W, real(0));
  for (int e = 0; e < P; e++) {
    real* x = r.data() + (size_t)e * W;
    switch (kind) {
      case nmrows::kFric: x[0] = real(0.8); x[1] = real(25); x[2] = real(0.8); break;
      case nmrows::kBody:
        for (int j = 0; j < W; j++) x[j] = real(0.01);
        x[nm::BP_MASS] = real(1.5); x[nm::BP_TOTAL] = real(4); x[nm::BP_PGS] = real(1);
        break;
      case nmrows::kGrav: x[nm::GP_G + 2] = real(-9.81); x[nm::GP_VEC + 2] = real(-9.81); break;
      case nmrows::kServo: x[nm::SV_RATE] = real(0.3); x[nm::SV_DGAIN] = real(0.1); break;
      default: x[0] = x[1] = x[2] = real(3); break;
    }
  }
  return r;
}

template <class real> static void faults(const char* dt) {
  const int P = 3, nsub = 2;
  const real nan = (real)NAN;
  for (int kind = 0; kind < nmrows::kKinds; kind++) {
    if (kind == nmrows::kLat) continue;
    const int W = nmrows::kind_width(kind);
    auto say = [&](const char* name, const std::vector<real>& r) {
      const std::string why = nmrows::pool_rows_fault<real>(kind, r.data(), P, nsub);
      printf("fault %d %s %s : %s\n", kind, dt, name, why.empty() ? "ok" : why.c_str());
    };
    say("good", good_rows<real>(kind, P));
    auto bad = [&](const char* name, int word, real v) {
      std::vector<real> r = good_rows<real>(kind, P);
      r[(size_t)(P - 1) * W + word] = v;          // the last row: every row is looked at
      say(name, r);
    };
    switch (kind) {
      case nmrows::kFric: bad("mu", 0, real(1e-6)); bad("p_gain", 1, real(-1)); bad("kv", 2, real(-0.5)); bad("nan", 1, nan); break;
      case nmrows::kBody: bad("mass", nm::BP_MASS, real(0)); bad("total", nm::BP_TOTAL, real(1)); bad("nan", 0, nan); bad("pgs", nm::BP_PGS, real(0)); break;
      case nmrows::kGrav: bad("zero_vec", nm::GP_VEC + 2, real(0)); bad("nan", nm::GP_G, nan); break;
      case nmrows::kServo: bad("rate", nm::SV_RATE, real(0)); bad("d_gain", nm::SV_DGAIN, real(-1)); bad("nan", nm::SV_RATE, nan); break;
      default: bad("limit", 1, real(0)); bad("nan", 2, nan); break;
    }
  }
}

int main() {
  printf("first");
  for (int k = 0; k <= nm::kResetRowKinds; k++) printf(" %d", nm::reset_rows_first(k));
  printf("\nmap");
  for (int l = 0; l < nm::kResetRowWords; l++) printf(" %d", nm::reset_rows_kind(l));
  printf("\n");
  const uint32_t size_sets[4][6] = {{1, 1, 1, 1, 1, 1}, {5, 5, 5, 5, 5, 5}, {65536, 65536, 65536, 65536, 65536, 65536}, {5, 0, 4, 2, 0, 7}};
  const uint32_t ks[3] = {0u, 1u, 1u << 29};
  for (int s = 0; s < 4; s++)
    for (int64_t genv : {(int64_t)0, (int64_t)62, (int64_t)4097})
      for (uint32_t k : ks) {
        uint32_t out[6];
        nm::nm_reset_rows_pick(11, (uint64_t)genv, k, size_sets[s], out);
        printf("pick 11 %lld %u %u %u %u %u %u %u : %u %u %u %u %u %u\n", (long long)genv, k, size_sets[s][0], size_sets[s][1], size_sets[s][2],
               size_sets[s][3], size_sets[s][4], size_sets[s][5], out[0], out[1], out[2], out[3], out[4], out[5]);
      }
  faults<float>("f32");
  faults<double>("f64");
  {
    const int good[3] = {0, 3, 6}, bad_hi[3] = {0, 7, 1}, bad_lo[3] = {0, -1, 1};
    for (const int* d : {good, bad_hi, bad_lo}) {
      const std::string why = nmrows::pool_rows_fault<float>(nmrows::kLat, d, 3, 2);
      printf("fault 2 i32 %s : %s\n", d == good ? "good" : d == bad_hi ? "above" : "below", why.empty() ? "ok" : why.c_str());
    }
  }
  return 0;
}
