// Test-only host program (tests/test_pid_host.py): the balance controller's row function
// (csrc/bb_pid.h: pid_row, the code the kernel of bb_pid_act runs per env) built for the CPU and run
// over T steps of n rows.  Built with -O2 -ffp-contract=off.  Never shipped.
//
//   pid_check IN OUT
// IN : int32[8] = orient_kind, space, n, T, stride (floats per orientation row), has_setpoint,
//      has_reset, 0;  float[5] = dt, k_p, k_i, k_d, limit;  float[T][n][stride] orientations;
//      float[T][n][2] setpoints if has_setpoint;  uint8[T][n] reset flags if has_reset.
// OUT: float[T][n][w] commands (w = 3 motor space, 2 pitch/roll space);  float[T][n] angle_deg;
//      float[T][n][4] the state after each step.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "bb_pid.h"

static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: pid_check IN OUT\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int32_t hd[8];
  float g[5];
  if (!rd(f, hd, sizeof hd) || !rd(f, g, sizeof g)) return fprintf(stderr, "short header\n"), 2;
  const int kind = hd[0], space = hd[1], n = hd[2], T = hd[3], stride = hd[4];
  if (n < 1 || T < 1 || stride < (kind == bb::PID_ROTMAT ? 9 : 3)) return fprintf(stderr, "bad header\n"), 2;
  const int w = space == bb::PID_PITCH_ROLL ? 2 : 3;
  const size_t rows = size_t(T) * size_t(n);
  std::vector<float> orient(rows * stride), sp(hd[5] ? rows * 2 : 0);
  std::vector<uint8_t> reset(hd[6] ? rows : 0);
  if (!rd(f, orient.data(), orient.size() * 4) || !rd(f, sp.data(), sp.size() * 4) || !rd(f, reset.data(), reset.size()))
    return fprintf(stderr, "short input\n"), 2;
  fclose(f);
  const bb::PidCfg cfg{g[0], g[1], g[2], g[3], g[4], kind, space};
  std::vector<float> out(rows * w), angle(rows), hist(rows * 4), state(size_t(n) * 4, 0.f);
  for (int t = 0; t < T; t++)
    for (int e = 0; e < n; e++) {
      const size_t r = size_t(t) * n + e;
      bb::pid_row(cfg, &orient[r * stride], hd[5] ? &sp[2 * r] : nullptr, hd[6] && reset[r] != 0, &state[4 * size_t(e)],
                  &out[w * r], &angle[r]);
      for (int i = 0; i < 4; i++) hist[4 * r + i] = state[4 * size_t(e) + i];
    }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return fprintf(stderr, "cannot open %s\n", argv[2]), 2;
  fwrite(out.data(), 4, out.size(), o);
  fwrite(angle.data(), 4, angle.size(), o);
  fwrite(hist.data(), 4, hist.size(), o);
  fclose(o);
  return 0;
}
