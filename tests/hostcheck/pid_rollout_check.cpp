// Test-only host program (tests/test_pid_rollout_host.py): balance()'s per-step accumulation
// (csrc/bb_pid.h: pid_summary_step, the code the kernel of bb_pid_rollout runs per env and step)
// built for the CPU and run over T recorded steps of n envs.  Built with -O2 -ffp-contract=off.
// Never shipped.
//
//   pid_rollout_check IN OUT
// IN : int32[4] = n, T, 0, 0;  double[T] weights;  float[T][n] reward;  uint8[T][n] done flags;
//      float[T][n] angle_deg;  float[T][n][2] pos2d.
// OUT: uint8[n] alive;  uint8[n] failed;  int64[n] steps;  float[n] max_angle;  double[n] g_tau;
//      float[n][2] pos2d.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "bb_pid.h"

static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: pid_rollout_check IN OUT\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int32_t hd[4];
  if (!rd(f, hd, sizeof hd)) return fprintf(stderr, "short header\n"), 2;
  const int n = hd[0], T = hd[1];
  if (n < 1 || T < 1) return fprintf(stderr, "bad header\n"), 2;
  const size_t rows = size_t(T) * size_t(n);
  std::vector<double> w(T);
  std::vector<float> rew(rows), deg(rows), p2(rows * 2);
  std::vector<uint8_t> flags(rows);
  if (!rd(f, w.data(), w.size() * 8) || !rd(f, rew.data(), rows * 4) || !rd(f, flags.data(), rows) ||
      !rd(f, deg.data(), rows * 4) || !rd(f, p2.data(), rows * 8))
    return fprintf(stderr, "short input\n"), 2;
  fclose(f);
  std::vector<bb::PidSummary> s(n);
  for (auto& x : s) x = bb::PidSummary{1, 0, 0, 0.f, 0.0, {0.f, 0.f}};
  for (int t = 0; t < T; t++)
    for (int e = 0; e < n; e++) {
      const size_t r = size_t(t) * n + e;
      bb::pid_summary_step(s[e], deg[r], rew[r], flags[r], &p2[2 * r], w[t]);
    }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return fprintf(stderr, "cannot open %s\n", argv[2]), 2;
  for (auto& x : s) fwrite(&x.alive, 1, 1, o);
  for (auto& x : s) fwrite(&x.failed, 1, 1, o);
  for (auto& x : s) fwrite(&x.steps, 8, 1, o);
  for (auto& x : s) fwrite(&x.max_angle, 4, 1, o);
  for (auto& x : s) fwrite(&x.g_tau, 8, 1, o);
  for (auto& x : s) fwrite(x.pos, 4, 2, o);
  fclose(o);
  return 0;
}
