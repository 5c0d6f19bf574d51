// bb_pid_rollout.hip -- pid_rollout_kernel and its launch (bb_pid_rollout) as their own
// translation unit: bb_kernels.hip compiled with BB_PID_TU (everything but the C-ABI), with the
// product's flags, so that the kernels of bb_kernels.hip's own unit are compiled exactly as they
// were before this kernel existed (see bb_pid_rollout_launch_tu in bb_kernels.hip).
#define BB_PID_TU
// no batched pre-phase reads in this unit (bb_physics.h; the same bits either way): its fp64 fast
// kernel is at the 512-register limit with scratch, so its forward keeps the serial text
#ifndef BB_NO_PRE_BATCH
#define BB_NO_PRE_BATCH
#endif
// for the same reason its solve keeps its operands where they were and its three sums apart
// (bb_solve.h, bb_team16.h; the same bits either way): no square rows, no workspace growth here
#ifndef BB_NO_HROW_SQUARE
#define BB_NO_HROW_SQUARE
#endif
#ifndef BB_NO_GROUND_RECORD
#define BB_NO_GROUND_RECORD
#endif
#ifndef BB_NO_SUM3
#define BB_NO_SUM3
#endif
// and its factorisation and sweeps keep the parent's text (bb_team16.h; the same bits either way):
// with the lean forms pid_rollout_kernel<double, false> goes from 20 to 28 B of scratch
#ifndef BB_NO_LEAN_SOLVE
#define BB_NO_LEAN_SOLVE
#endif
#ifdef BB_PHASE_CLOCKS  // diagnostic builds: this unit's counters under their own name
#define bb_phase_cycles bb_phase_cycles_pid
#endif
#include "bb_kernels.hip"
