// Host side of a network inside the library, once for its families (cnn.hip, mixer.hip): the fields every handle has and
// the steps of its life that do not depend on the kernels.  Its rules are stated here and nowhere else: grad is zeroed on
// the ctx stream, the one the kernels run on; set_params or another problem dtype makes the next call pack the parameters
// again; the stream is synchronised before a workspace or a packed block is freed and before the handle is deleted; a
// handle that cannot be opened owns nothing.  A family F is a struct of static functions over its handle (CnnFamily,
// MixerFamily): the last_kernel strings forward_kernels and vjp_kernels, refuse (the problems it does not run),
// keyed_for / rekey (is the workspace this problem's; free it and record the problem's key), size_workspace, and in the
// problem dtype pack (the parameters as a staging vector, handed to net_upload), forward and backward.
#pragma once

#include <initializer_list>

#include "common.hpp"

namespace pdeopt {

inline int pad16(int c) { return (c + 15) / 16 * 16; }

struct NativeNet {
  pdeopt_ctx* ctx = nullptr;
  const char* what = "";        // "CNN" / "mixer": the family's name in messages
  int64_t n_params = 0;
  std::vector<double> params;   // host copy, torch order
  bool have_params = false;
  DeviceBuffer packed;          // the parameters as the kernels read them, in the problem dtype; grow-only
  int packed_dtype = -1;
  bool packed_valid = false;
  int s_dtype = -1;             // dtype of the workspace the family keeps; -1: there is none
  DeviceBuffer grad;            // [n_params], fp64, accumulates until net_grad_read(reset)
};

// the tail of pdeopt_*_create, for a handle whose family fields and n_params are set
template <class Net>
int net_open(pdeopt_ctx* ctx, Net* n, Net** out) {
  n->ctx = ctx;
  const auto bail = [&](hipError_t e, const char* what) {
    delete n;
    return fail(ctx, PDEOPT_EHIP, "%s failed: %s", what, hipGetErrorString(e));
  };
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return bail(e, "hipSetDevice");
  if (const int rc = ensure_buffer(ctx, n->grad, n->n_params * sizeof(double))) {
    delete n;
    return rc;
  }
  if ((e = hipMemsetAsync(n->grad.get(), 0, n->n_params * sizeof(double), ctx->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
  *out = n;
  return PDEOPT_OK;
}

inline int net_set_params(NativeNet* n, const double* params, int64_t count) {
  if (!n) return PDEOPT_EINVAL;
  if (!params || count != n->n_params)
    return fail(n->ctx, PDEOPT_EINVAL, "the %s has %lld parameters (got %lld)", n->what, (long long)n->n_params, (long long)count);
  n->params.assign(params, params + count);
  n->have_params = true;
  n->packed_valid = false;  // packed in the problem dtype by the next forward / vjp
  return PDEOPT_OK;
}

// the tail of F::pack<T>: the staging vector h to the device
template <typename T>
int net_upload(NativeNet* n, const std::vector<T>& h) {
  pdeopt_ctx* ctx = n->ctx;
  const size_t bytes = h.size() * sizeof(T);
  if (const int rc = grow_device_buffer(ctx, n->packed, bytes, /*sync_first=*/true)) return rc;
  // the staging vector dies with the caller: the copy is complete for the host when this returns (pageable memory)
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(n->packed.get(), h.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  n->packed_dtype = ctx->prob.dtype;
  n->packed_valid = true;
  return PDEOPT_OK;
}

// what every call asks of the ctx's problem and of the fields it is given; packs parameters and sizes the workspace
template <class F, class Net>
int net_prepare(Net* n, bool backward, std::initializer_list<const void*> fields) {
  pdeopt_ctx* ctx = n->ctx;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const pdeopt_problem& p = ctx->prob;
  if (p.nz > 1 || ctx->comps != 1 || ctx->halo)
    return fail(ctx, PDEOPT_EINVAL, "the %s runs on periodic 2-D real fields [batch][nx][ny]", n->what);
  if (const int rc = F::refuse(n, p)) return rc;
  if (!n->have_params) return fail(ctx, PDEOPT_ESTATE, "set_params has not been called for this %s", n->what);
  for (const void* f : fields)
    if (!f || (uintptr_t)f % ctx->esize)
      return fail(ctx, PDEOPT_EINVAL, "field pointer %p: device fields are [batch][nx][ny] in the problem dtype, aligned to it", f);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!n->packed_valid || n->packed_dtype != p.dtype)
    if (const int rc = with_dtype(ctx, [&](auto t) { return F::pack(t, n); })) return rc;
  if (!F::keyed_for(n, p)) {
    if (n->s_dtype >= 0) PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // launches may still use the old workspace
    F::rekey(n, p);
  }
  return F::size_workspace(n, backward);
}

template <class F, class Net>
int net_forward(Net* n, const void* u, void* mu) {
  if (!n) return PDEOPT_EINVAL;
  if (const int rc = net_prepare<F>(n, false, {u, mu})) return rc;
  n->ctx->last_kernel = F::forward_kernels;
  return with_dtype(n->ctx, [&](auto t) { return F::forward(t, n, u, mu, false); });
}

// lam is read and written while u and gmu are read: does it share a byte with either
inline bool net_vjp_overlaps(const pdeopt_ctx* ctx, const void* lam, const void* u, const void* gmu) {
  const auto overlap = [&](const void* a, const void* b) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + ctx->total_bytes && y < x + ctx->total_bytes;
  };
  return overlap(lam, u) || overlap(lam, gmu);
}

template <class F, class Net>
int net_vjp(Net* n, const void* u, const void* gmu, void* lam) {
  if (!n) return PDEOPT_EINVAL;
  pdeopt_ctx* ctx = n->ctx;
  if (const int rc = net_prepare<F>(n, true, {u, gmu, lam})) return rc;
  if (net_vjp_overlaps(ctx, lam, u, gmu)) return fail(ctx, PDEOPT_EINVAL, "lam_dev is written: it must not overlap u_dev or gmu_dev");
  ctx->last_kernel = F::vjp_kernels;
  return with_dtype(ctx, [&](auto t) {
    // the value mu itself is not needed: the forward pass stops below the last layer
    if (const int rc = F::forward(t, n, u, (void*)nullptr, true)) return rc;
    return F::backward(t, n, u, gmu, lam);
  });
}

inline int net_grad_read(NativeNet* n, double* out, int64_t count, int reset) {
  if (!n) return PDEOPT_EINVAL;
  pdeopt_ctx* ctx = n->ctx;
  if (!out || count != n->n_params)
    return fail(ctx, PDEOPT_EINVAL, "the %s has %lld parameters (got %lld)", n->what, (long long)n->n_params, (long long)count);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(out, n->grad.get(), count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (reset) PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(n->grad.get(), 0, count * sizeof(double), ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

template <class Net>
int net_close(Net* n) {
  if (!n) return PDEOPT_OK;
  (void)hipSetDevice(n->ctx->device);
  if (n->ctx->stream) (void)hipStreamSynchronize(n->ctx->stream);
  delete n;
  return PDEOPT_OK;
}

}  // namespace pdeopt
