// call_common.h -- the frame of a call that scans or looks up the snapshot and hands out YIELD rows
// (fetch.hip, find.hip; included after row_gather.h, every definition translation-unit local):
//   begin_call     the call's Timing and its first event
//   run_guarded    no launch or copy outlives a block the call frees when it throws
//   hand_out_call  yield_rows' columns -> the caller (hand_out_rows), the call's last event
#pragma once
#include <memory>

#include "engine.h"
#include "query_common.h"
#include "row_gather.h"
#include "rows.h"

namespace nbg {
namespace {

void begin_call(Ctx& c) {
  c.timing = Timing{};
  timing_reset(c);
  c.total_pending = false;
  if (c.host_stage_used) NBG_HIP(hipStreamSynchronize(c.stream));  // a failed query's copies
  c.host_stage_used = 0;
  NBG_HIP(hipEventRecord(c.ev[0], c.stream));
}

void hand_out_call(Ctx& c, YieldOut& y, int64_t n_rows, bool keep_on_device, nbg_rows* out) {
  NBG_HIP(hipEventRecord(c.ev[1], c.stream));
  c.total_pending = true;
  auto h = std::make_unique<HostRows>();
  h->types = y.types;
  h->dev = std::move(y.dev);
  hand_out_rows(c, std::move(h), y.off, y.str_bytes, n_rows, keep_on_device, out);
  out->edges_scanned = c.timing.edges_scanned;
}

template <typename F>
int32_t run_guarded(Ctx& c, F f) {
  try {
    return f();
  } catch (...) {
    // no launch or copy may still use a block this call frees on the way out
    (void)hipStreamSynchronize(c.stream);
    throw;
  }
}

}  // namespace
}  // namespace nbg
