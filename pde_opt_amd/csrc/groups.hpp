// The environment-group schedule shared by the substep pipelines (explicit integrators, fused Strang, fused IMEX).
//
// Environments are independent, so n substeps may run group by group: a group whose working set fits the Infinity
// Cache keeps every pass on-die instead of streaming the whole batch through HBM once per pass.  Optionally two groups
// run side by side, the first on the ctx stream and the second on the ctx's second stream.  WHEN to group and when
// to go side by side is the callers' policy; this file is the mechanism, and the only place that touches the second
// stream and its fork / join events.
#pragma once

#include <algorithm>

#include "common.hpp"

namespace pdeopt {

// largest balanced group of environments whose working set (bytes_per_env each) fits the cache budget; the whole
// batch when that fits.  even: groups of an even number of environments (two real fields per complex transform)
inline int cache_group(int batch, size_t bytes_per_env, size_t budget, bool even) {
  int64_t fit = (int64_t)(budget / bytes_per_env);
  fit = even ? std::max<int64_t>(2, fit & ~1LL) : std::max<int64_t>(1, fit);
  if (fit >= batch) return batch;
  const int ngroups = (int)((batch + fit - 1) / fit);
  const int group = (batch + ngroups - 1) / ngroups;
  return even ? (group + 1) & ~1 : group;
}

// Substeps [s0, n) of every group of `group` environments: first(w) once per group (may be a no-op), then
// step(w, s, took) per substep; a step that advanced two substeps sets took = 2 (it is preset to 1, and both groups
// of a pair must agree).  two_streams: groups run in pairs, and the host issues substep s of the first group on the
// ctx stream, then substep s of the second on the second stream, then s + 1 -- that order is what overlaps one
// group's ramp and tail with the other group's work.  Otherwise group after group on the ctx stream.
// Returns the first error, after the join has been queued: later work on the ctx stream sees both groups' results
// and the second stream is idle again whatever happened.
template <typename First, typename Step>
int run_groups(pdeopt_ctx* ctx, int group, bool two_streams, int64_t s0, int64_t n, First&& first, Step&& step) {
  const int batch = ctx->prob.batch;
  ctx->last_groups = (batch + group - 1) / group;
  const int lanes = two_streams && ctx->last_groups >= 2 ? 2 : 1;
  int rc = PDEOPT_OK;
  if (lanes == 2) {
    ctx->last_group_streams = 2;
    if ((rc = ensure_stream2(ctx))) return rc;
    // the second stream starts after everything already queued on the ctx stream (the state upload, the previous call)
    PDEOPT_HIP_CHECK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
  }
  for (int lo = 0; lo < batch && !rc; lo += lanes * group) {
    Window w[2];
    int nw = 0;
    for (int l = lo; nw < lanes && l < batch; l += group, ++nw)
      w[nw] = Window{l, std::min(group, batch - l), nw ? ctx->stream2 : ctx->stream};
    for (int k = 0; k < nw && !rc; ++k) rc = first(w[k]);
    for (int64_t s = s0; s < n && !rc;) {
      int took = 1;
      for (int k = 0; k < nw && !rc; ++k) rc = step(w[k], s, took);
      s += took;
    }
  }
  if (lanes == 2) {
    const hipError_t e1 = hipEventRecord(ctx->ev_join, ctx->stream2);
    const hipError_t e2 = hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
    if (rc) return rc;
    PDEOPT_HIP_CHECK(ctx, e1);
    PDEOPT_HIP_CHECK(ctx, e2);
  }
  return rc;
}

}  // namespace pdeopt
