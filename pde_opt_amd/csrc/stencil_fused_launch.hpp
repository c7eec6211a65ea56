// Host-side dispatch of the fused stage-pair kernels (included after every kernel header so that the
// kernel templates are defined before their launch sites are instantiated).
#pragma once

#include "stencil_fused.hpp"
#include "stencil_fused_ac.hpp"

namespace pdeopt {

template <typename T>
int launch_pair(pdeopt_ctx* ctx, const Window& w, const HaloIo& io, int pair, const void* in, const void* y, const void* acc, void* out,
                void* acc_out, double aA, double bA, double aB, double bB) {
  const pdeopt_problem& p = ctx->prob;
  PairArgs<T> s{};
  s.g = make_geo(ctx);
  const int64_t woff = (int64_t)w.lo * s.g.bstride;
  s.in = static_cast<const T*>(in) + woff;
  s.y = y ? static_cast<const T*>(y) + woff : nullptr;
  s.acc = acc ? static_cast<const T*>(acc) + woff : nullptr;
  s.out = static_cast<T*>(out) + woff;
  s.acc_out = acc_out ? static_cast<T*>(acc_out) + woff : nullptr;
  s.aA = T(aA); s.bA = T(bA); s.aB = T(aB); s.bB = T(bB);
  const GridRecip r = grid_recip(p);
  set_recip_halved(s, r.rx2, r.ry2);
  set_closures<T>(s, ctx, w.lo);
  s.dbg = (int)ctx->opt_debug_ablate;
  s.part = io.part;
  // halo-8 layout of a decomposed field: PAIR_12 on the tile + 4 ring, PAIR_34 with the fused pack
  int ext = 0;
  if (ctx->halo == 8) {
    if (p.equation != PDEOPT_EQ_CAHN_HILLIARD) return fail(ctx, PDEOPT_EINVAL, "the halo-8 layout runs the fused Cahn-Hilliard stage pairs only");
    if (pair == PAIR_12) {
      ext = io.ext;
      const int64_t shift = (int64_t)ext * s.g.ld + ext;
      s.in -= shift; s.out -= shift; s.acc_out -= shift;
      s.ext = ext;
      // fused unpack: halo cells straight from the neighbours' strips
      s.strip_env = 2LL * 8 * p.ny + 2LL * p.nx * 8 + 4LL * 64;
      fill_neighbour_strips<T>(io, s.strip_env * p.batch, s.nbase);
    } else if (io.strip) {
      s.strip = static_cast<T*>(io.strip);
      s.strip_env = 2LL * 8 * p.ny + 2LL * p.nx * 8 + 4LL * 64;
    }
  }
  ctx->n_stage_launches++;
  const int cl = classify_closures(p.mu, p.mob);
  // tile height of the pair kernels.  CH: 32 rows (512-thread workgroups) where they divide the grid --
  // less redundant ring work at the same VGPR count, +4.5 % on 1024^2 same-box once the kernel sat at
  // 78 / 88 VGPRs -- otherwise 16; PDEOPT_OPT_TILE_ROWS overrides.  AC follows the per-stage kernels.
  int rpt = tiled_rpt(ctx);
  if (p.equation == PDEOPT_EQ_CAHN_HILLIARD && ctx->opt_tile_rows == 0) rpt = (p.nx % 32 == 0) ? 4 : 2;
  char name[96];
  snprintf(name, sizeof(name), "stage_pair<%s,%s,%s,rows%d>", dtype_name<T>(), p.equation == PDEOPT_EQ_ALLEN_CAHN ? "AC" : "CH",
           closure_class_name(cl), 8 * rpt);
  ctx->last_kernel = name;
  // CH with a linear polynomial part: the shorter closure (same bits, see closures.hpp); ext is 0 outside PAIR_12
  const int cl1 = p.equation == PDEOPT_EQ_CAHN_HILLIARD ? narrow_logit1(cl, p.mu) : cl;
  return with_closure_class<CL_POLY, CL_LOGIT, CL_LOGIT1>(cl1, [&](auto c) {
    constexpr int CL = decltype(c)::value;
    auto go = [&](auto pr, auto rows) {
      constexpr int PAIR = decltype(pr)::value, RPT = decltype(rows)::value;
      if constexpr (CL == CL_LOGIT1) return launch_pair_ch_inst<T, CL, PAIR, RPT>(ctx, w, s, ext);
      else return launch_pair_inst<T, CL, PAIR, RPT>(ctx, w, s, ext);
    };
    if (pair == PAIR_12) return rpt == 2 ? go(int_c<PAIR_12>{}, int_c<2>{}) : go(int_c<PAIR_12>{}, int_c<4>{});
    return rpt == 2 ? go(int_c<PAIR_34>{}, int_c<2>{}) : go(int_c<PAIR_34>{}, int_c<4>{});
  });
}

// out = f(in) for every environment of the window through the stage-B half of the fused kernel
// (PAIR_K): the slope launch of the IMEX step.  Same arithmetic as launch_pair's stages (including the
// folded mu form of the linear-logit class), so it may differ from the per-stage kernels' k by rounding;
// pdeopt_rhs and the explicit integrators do not come here.
template <typename T>
bool slope_pair_supported(const pdeopt_ctx* ctx) {
  return ctx->prob.equation == PDEOPT_EQ_CAHN_HILLIARD && !ctx->halo && ctx->opt_fuse_stages >= 0 &&
         ctx->opt_kernel_path != 1 && fused_supported<T>(ctx);
}
template <typename T>
int launch_slope_pair(pdeopt_ctx* ctx, const Window& w, const void* in, void* out) {
  const pdeopt_problem& p = ctx->prob;
  PairArgs<T> s{};
  s.g = make_geo(ctx);
  const int64_t woff = (int64_t)w.lo * s.g.bstride;
  s.in = static_cast<const T*>(in) + woff;
  s.out = static_cast<T*>(out) + woff;
  const GridRecip r = grid_recip(p);
  set_recip_halved(s, r.rx2, r.ry2);
  set_closures<T>(s, ctx, w.lo);
  ctx->n_stage_launches++;
  const int cl = classify_closures(p.mu, p.mob);
  const bool rows32 = ctx->opt_tile_rows == 32 || (ctx->opt_tile_rows == 0 && p.nx % 32 == 0);
  ctx->last_kernel = rows32 ? "slope_pair<CH,rows32>" : "slope_pair<CH,rows16>";
  return with_closure_class<CL_POLY, CL_LOGIT, CL_LOGIT1>(narrow_logit1(cl, p.mu), [&](auto c) {
    constexpr int CL = decltype(c)::value;
    return rows32 ? launch_pair_ch_inst<T, CL, PAIR_K, 4>(ctx, w, s, 0) : launch_pair_ch_inst<T, CL, PAIR_K, 2>(ctx, w, s, 0);
  });
}

}  // namespace pdeopt
