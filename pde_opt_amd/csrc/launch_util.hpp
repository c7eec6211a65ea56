// Host-side helpers every kernel launcher shares: kernel-argument setup (closures, environment parameters, grid
// reciprocals), dispatch of the run-time dtype and closure class to template arguments, and the pieces of the
// last_kernel names.  Included at the end of common.hpp.
#pragma once

#include <type_traits>

namespace pdeopt {

inline ClosureSpec closure_spec(const pdeopt_closure& c) { return ClosureSpec{c.kind, c.flags, c.n}; }

// parameters of the environments from first_env on, in the arithmetic type of the path
template <typename T>
inline const EnvParams<T>* env_params(const pdeopt_ctx* ctx, int first_env) {
  return ctx->env_params_dev.as<const EnvParams<T>>() + first_env;
}
// the three members every argument struct sets the same way
template <typename T, typename Args>
inline void set_closures(Args& s, const pdeopt_ctx* ctx, int first_env) {
  s.ep = env_params<T>(ctx, first_env);
  s.mu = closure_spec(ctx->prob.mu);
  s.mob = closure_spec(ctx->prob.mob);
}

// Reciprocals of the grid spacings, in double; every fill site casts to its T from these.  The argument structs
// name their reciprocal fields alike (rhx, rhy, rhx2, rhy2) under TWO conventions:
//   plain  (set_recip_plain):  rhx = 1 / hx,       rhx2 = 1 / hx^2  -- StageArgs, CoopArgs, SensArgs, Sens3Args
//   halved (set_recip_halved): rhx = 0.5 / hx^2,   rhx2 = 1 / hx^2  -- PairArgs, Quad4Args, SmallArgs, SmallTsit5Args
//                              (the folded flux constant of face_flux, stencil_fused.hpp)
// The halved form is T(0.5 * rx2): scaling a double by 0.5 is exact, so it has the bits of T(0.5 / (hx * hx)).
// (QuadArgs of the Allen-Cahn single-pass kernel has rhx2 / rhy2 only.)  rz / rz2 are meaningful for nz > 1 only.
struct GridRecip {
  double rx, ry, rz, rx2, ry2, rz2;
};
inline GridRecip grid_recip(const pdeopt_problem& p) {
  return {1.0 / p.hx, 1.0 / p.hy, 1.0 / p.hz, 1.0 / (p.hx * p.hx), 1.0 / (p.hy * p.hy), 1.0 / (p.hz * p.hz)};
}
template <typename Args>
inline void set_recip_plain(Args& s, const GridRecip& r) {
  using T = decltype(s.rhx);
  s.rhx = T(r.rx); s.rhy = T(r.ry);
  s.rhx2 = T(r.rx2); s.rhy2 = T(r.ry2);
}
template <typename Args>
inline void set_recip_halved(Args& s, double rx2, double ry2) {
  using T = decltype(s.rhx);
  s.rhx = T(0.5 * rx2); s.rhy = T(0.5 * ry2);
  s.rhx2 = T(rx2); s.rhy2 = T(ry2);
}

// f(T{}) for the arithmetic type T of a dtype: the tag is a value, decltype(tag) is float or double.
//   with_dtype(ctx, [&](auto t) { return launch_x<decltype(t)>(ctx, ...); })
template <typename F>
inline auto with_dtype(int dtype, F&& f) {
  return dtype == PDEOPT_F32 ? f(float{}) : f(double{});
}
template <typename F>
inline auto with_dtype(const pdeopt_ctx* ctx, F&& f) {
  return with_dtype(ctx->prob.dtype, f);
}

template <int V>
using int_c = std::integral_constant<int, V>;

// f(int_c<CL>{}) for the closure class cl.  The classes a site may see are part of the call
// and are exactly what it instantiates: cl among Others... runs that class, anything else runs Default.
//   with_closure_class<CL_POLY, CL_LOGIT>(cl, [&](auto c) { return launch_x<T, decltype(c)::value>(...); })
template <int Default, int... Others, typename F>
inline int with_closure_class(int cl, F&& f) {
  int rc = 0;
  const bool hit = ((cl == Others ? (rc = f(int_c<Others>{}), true) : false) || ...);
  return hit ? rc : f(int_c<Default>{});
}
// sites with a CL_LOGIT1 kernel opt into it: a logit class whose polynomial part is linear
inline int narrow_logit1(int cl, const pdeopt_closure& mu) { return cl == CL_LOGIT && mu.n <= 2 ? CL_LOGIT1 : cl; }

// pieces of the last_kernel names (next to equation_short_name)
template <typename T>
inline const char* dtype_name() { return sizeof(T) == 4 ? "f32" : "f64"; }
inline const char* closure_class_name(int cl) {
  return cl == CL_GENERIC ? "generic" : cl == CL_LOGIT || cl == CL_LOGIT1 ? "logit" : "poly";
}

}  // namespace pdeopt
