// Host build of csrc/bb_eval.h for tests/test_eval_track_host.py: eval_track_serial, the statement of
// bb_eval_track's accounting and staging that the kernel is held to, behind a C entry point whose
// argument struct is bb_eval_args (include/ballbot_mi355x.h) field for field.
#include <stdint.h>

#include "ballbot_mi355x.h"
#include "bb_eval.h"

static_assert(sizeof(bb_eval_args) == sizeof(bb::EvalArgs), "EvalArgs mirrors bb_eval_args");

extern "C" int ec_eval_track(const bb_eval_args* a) {
  if (!a || a->n < 1) return -1;
  const bb::EvalArgs e{a->n, a->cap, a->reward, a->flags, a->obs, a->rel_ts, a->targets, a->ep_ret, a->ep_len,
                       a->counts, a->tab_ret, a->tab_len, a->tab_env, a->tab_step, a->book, a->feats, a->fresh};
  bb::eval_track_serial(e);
  return 0;
}
