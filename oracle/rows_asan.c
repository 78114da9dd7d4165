/* rows_asan.c - host-only sanitizer run of the oracle's per-env rows (make -C oracle rows_asan).
 *
 * TEST INFRASTRUCTURE ONLY (see nm_oracle.h). Two env objects with different non-default rows of every kind, 20 steps with 4 threads,
 * half of the envs reset, both destroyed: built with -fsanitize=address,undefined, it must end with "rows_asan: ok" and nothing else.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nm_oracle.h"

#define N 6
#define DECIMATION 2

static nmo_env* make(int which) {
  nmo_env* e = nmo_env_create(N, 5, 0, 4);
  double g[N][3], vec[N][3], envp[N][3], servo[N][2], fmax[N][3], wrench[N][6];
  int32_t delay[N];
  for (int i = 0; i < N; i++) {
    const double s = which ? -1.0 : 1.0;
    g[i][0] = 0.3 * s * i; g[i][1] = -0.2 * s; g[i][2] = -9.81 + 0.1 * i;
    vec[i][0] = which ? g[i][0] : 0; vec[i][1] = which ? g[i][1] : 0; vec[i][2] = which ? g[i][2] : -9.81;
    envp[i][0] = 0.4 + 0.2 * i; envp[i][1] = which ? 14.0 : 26.0; envp[i][2] = 0.5 + 0.1 * i;
    delay[i] = which ? i : NMO_NHIST * DECIMATION - i; /* 0 .. 6: every switch substep and the deepest history slot */
    servo[i][0] = i % 2 ? 0.02 * (i + which) : INFINITY; servo[i][1] = 0.05 * i;
    fmax[i][0] = i % 3 ? 3.2 : INFINITY; fmax[i][1] = 0.3 + 0.5 * i; fmax[i][2] = which ? 2.0 : INFINITY;
    for (int k = 0; k < 6; k++) wrench[i][k] = s * (k < 3 ? 1.0 + i : 0.1 * (k - 2));
  }
  nmo_env_set_gravity(e, &g[0][0], &vec[0][0]);
  nmo_env_set_env_params(e, &envp[0][0]);
  nmo_env_set_action_latency(e, delay, NULL);
  nmo_env_set_servo(e, &servo[0][0], NULL);
  nmo_env_set_torque_limit(e, &fmax[0][0], which);
  nmo_env_set_base_wrench(e, &wrench[0][0]);
  nmo_env_reset_idx(e, NULL, 0, NULL);
  return e;
}

int main(void) {
  nmo_env* env[2] = {make(0), make(1)};
  float actions[N * 18], obs[N * 66], rew[N];
  int64_t done[N];
  double margin[N], lim[N][18], checksum = 0;
  for (int t = 0; t < 20; t++)
    for (int w = 0; w < 2; w++) {
      for (int k = 0; k < N * 18; k++) actions[k] = (float)sin(0.37 * k + 0.9 * t + w);
      nmo_env_step(env[w], actions, NULL, obs, rew, done, NULL, NULL, NULL);
      if (t == 9) {
        const int32_t ids[N / 2] = {0, 2, 4};
        nmo_env_reset_idx(env[w], ids, N / 2, NULL);
      }
      nmo_env_step_physics(env[w], actions);
      nmo_env_get_torque_limit(env[w], NULL, margin);
      nmo_env_get_servo(env[w], NULL, &lim[0][0]);
      for (int i = 0; i < N; i++) checksum += rew[i] + obs[i * 66 + 12] + lim[i][1];
    }
  /* a data block without rows: the physics alone, under the defaults */
  nmo_data* d = (nmo_data*)calloc(1, sizeof *d);
  nmo_scratch* s = (nmo_scratch*)calloc(1, sizeof *s);
  nmo_reset_data(d);
  nmo_step(d, s, 3);
  checksum += d->qpos[2];
  free(d); free(s);
  nmo_env_destroy(env[0]);
  nmo_env_destroy(env[1]);
  if (!isfinite(checksum)) { printf("rows_asan: checksum %g\n", checksum); return 1; }
  printf("rows_asan: ok\n");
  return 0;
}
