// Batched Jacobians of the Dynamics plugin's point functions (include/pinoloco.h, pl_dyn_jac*).
//
// The reference gets these from ca.jacobian of its point functions (optimization/ocp.py:283-284);
// here one lane evaluates one (point, column) in dual numbers (dyn_jac.h).  A 64-thread workgroup
// is one wave that owns a tile of 64 consecutive columns of one point; the grid is
// batch x ceil(W / 64) workgroups.  For every output row the wave stores
// jac[b][r][c0 .. c0 + 63], consecutive lanes to consecutive doubles.  The kernel is instantiated
// per function family, so a frame-position column does not carry the tree pass's registers and
// LDS.  A device = -1 handle runs the same columns on the host.
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include "dyn_handle.h"
#include "dyn_jac.h"
#include "state.h"

namespace {

const char* const kFnName[PL_FN_COUNT] = {
    "rnea", "aba", "frame_pos", "frame_vel", "gaps_wb", "base_acc_wb", "com_dyn", "base_vel_cv", "base_acc_cv", "gaps_cv",
    "crba", "nle", "frame_jac", "cmap", "com", "integrate_wb", "difference_wb", "integrate_cv", "difference_cv", "gaps_ca"};

struct JacArgs {
  const double* in[4];
  int len[4], tan[4];
  int fn, flags, B, W, tiles, rows;
  unsigned wrt;
};

}  // namespace

template <int FAM>
__global__ __launch_bounds__(64) void k_dyn_jac(const PlModel* Mp, const PlOcpConst* Op, PlFrameRef F, JacArgs A,
                                                double* __restrict__ jac) {
  const int b = (int)blockIdx.x / A.tiles, tile = (int)blockIdx.x - b * A.tiles;
  const int lane = threadIdx.x;
  const int col = tile * 64 + lane;
  const PlModel& M = *Mp;
  const PlOcpConst& O = *Op;
  const double* p[4];
  for (int k = 0; k < 4; ++k) p[k] = A.in[k] ? A.in[k] + (size_t)b * A.len[k] : nullptr;
  // NodeKin<Dual> store of the tree-pass families: per-lane tangents, one shared value per entry
  // (the wave's lanes evaluate the same point, so every writing lane stores identical bits)
  constexpr bool kTree = FAM == pl::PL_JF_TREE || FAM == pl::PL_JF_COMP || FAM == pl::PL_JF_ABA;
  __shared__ double kst_tan[kTree ? PL_KIN_STORE * 64 : 1];
  __shared__ double kst_val[kTree ? PL_KIN_STORE : 1];
  __shared__ double aba_raw[FAM == pl::PL_JF_ABA ? PL_ABA_RAW : 1];
  __shared__ double aba_sh[FAM == pl::PL_JF_ABA ? PL_ABA_SH : 1];
  if constexpr (FAM == pl::PL_JF_ABA) {
    // the point's shared primal: the tile's lanes split the nv + 2 RNEA columns, lane 0 factors
    // M and solves for a (k_eval_jac<PL_DYN_ABA>'s pattern); lanes past W take part
    pl::NodeKin<double> kp;
    kp.store = kst_tan + lane;
    kp.stride = 64;
    for (int c = lane; c < M.nv + 2; c += 64) pl::aba_point_column(M, O, p[0], p[1], p[3], c, kp, aba_raw + c * M.nv);
    __syncthreads();
    if (lane == 0) pl::aba_factor_solve(M.nv, p[2], aba_raw, aba_sh);
    __syncthreads();
  }
  if (col >= A.W) return;
  int k, c;
  pl::dyn_jac_locate(A.tan, A.wrt, col, &k, &c);
  pl::NodeKin<Dual> kin;
  kin.vst = kst_val;
  kin.vstride = 1;
  kin.dst = kst_tan + lane;
  kin.dstride = 64;
  pl::dyn_jac_column<FAM>(M, O, F, A.fn, A.flags, p[0], p[1], p[2], p[3], k, c, kin, aba_sh,
                          jac + (size_t)b * A.rows * A.W + col, (size_t)A.W);
}

namespace {

// Shared front end: checks, sizes.  Returns 0 and fills A / F, or an error code.
int jac_prepare(const pl_dyn* d, int fn, int batch, int frame, int flags, unsigned wrt, const void* const* in,
                const void* jac, JacArgs* A, PlFrameRef* F) {
  if (!d || batch < 0) { pl_set_error("pl_dyn_jac: bad arguments"); return -1; }
  if (fn < 0 || fn >= PL_FN_COUNT) { pl_set_error("unknown dynamics function %d", fn); return -1; }
  const char* name = kFnName[fn];
  if (pl::dyn_jac_family(fn) == pl::PL_JF_NONE) {
    pl_set_error("pl_dyn_jac: %s has no Jacobian here (matrix-valued functions and the state maps are refused)", name);
    return -1;
  }
  if ((flags & 1) && !d->O[1].ext.valid) { pl_set_error("pl_dyn_jac(%s): no external-force frame on this handle", name); return -1; }
  pl::dyn_jac_tan_len(d->M, fn, d->O[flags & 1].nf, A->len, A->tan);
  if (wrt == 0) { pl_set_error("pl_dyn_jac(%s): wrt selects no input", name); return -1; }
  int W = 0;
  for (int k = 0; k < 32; ++k) {
    if (!((wrt >> k) & 1u)) continue;
    if (k >= 4 || A->len[k] == 0) { pl_set_error("pl_dyn_jac(%s): wrt bit %d is not an input of the function", name, k); return -1; }
    W += A->tan[k];
  }
  for (int k = 0; k < 4; ++k)
    if (A->len[k] > 0 && !in[k]) { pl_set_error("pl_dyn_jac(%s): input %d missing", name, k); return -1; }
  if (!jac) { pl_set_error("pl_dyn_jac(%s): jac is NULL", name); return -1; }
  int len2[4];
  if (int rc = pl_dyn_prepare(d, fn, frame, flags, in, len2, F)) {
    // keep the reason, add the function's name
    char msg[256];
    strncpy(msg, pl_last_error(), sizeof(msg) - 1);
    msg[sizeof(msg) - 1] = 0;
    pl_set_error("pl_dyn_jac(%s): %s", name, msg);
    return rc;
  }
  A->fn = fn;
  A->flags = flags;
  A->B = batch;
  A->W = W;
  A->tiles = (W + 63) / 64;
  A->rows = pl::dyn_jac_rows(d->M, fn);
  A->wrt = wrt;
  for (int k = 0; k < 4; ++k) A->in[k] = nullptr;
  if ((size_t)batch * (size_t)A->tiles > (size_t)INT_MAX) { pl_set_error("pl_dyn_jac(%s): batch %d is too large", name, batch); return -1; }
  return 0;
}

int jac_launch(pl_dyn* d, const PlFrameRef& F, const JacArgs& A, double* djac) {
  const dim3 grid((unsigned)((size_t)A.B * A.tiles)), block(64);
  const PlOcpConst* dO = d->dO + (A.flags & 1);
  switch (pl::dyn_jac_family(A.fn)) {
    case pl::PL_JF_TREE: hipLaunchKernelGGL(k_dyn_jac<pl::PL_JF_TREE>, grid, block, 0, d->stream, d->dM, dO, F, A, djac); break;
    case pl::PL_JF_COMP: hipLaunchKernelGGL(k_dyn_jac<pl::PL_JF_COMP>, grid, block, 0, d->stream, d->dM, dO, F, A, djac); break;
    case pl::PL_JF_ABA: hipLaunchKernelGGL(k_dyn_jac<pl::PL_JF_ABA>, grid, block, 0, d->stream, d->dM, dO, F, A, djac); break;
    case pl::PL_JF_CEN: hipLaunchKernelGGL(k_dyn_jac<pl::PL_JF_CEN>, grid, block, 0, d->stream, d->dM, dO, F, A, djac); break;
    default: hipLaunchKernelGGL(k_dyn_jac<pl::PL_JF_FRAME>, grid, block, 0, d->stream, d->dM, dO, F, A, djac); break;
  }
  PL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int pl_dyn_jac_sizes(const pl_dyn* d, int fn, int flags, int* in_len, int* tan_len, int* out_len) {
  if (!d || !in_len || !tan_len || !out_len) { pl_set_error("null argument"); return -1; }
  if (fn < 0 || fn >= PL_FN_COUNT) { pl_set_error("unknown dynamics function %d", fn); return -1; }
  if (pl::dyn_jac_family(fn) == pl::PL_JF_NONE) {
    pl_set_error("pl_dyn_jac_sizes: %s has no Jacobian here (matrix-valued functions and the state maps are refused)",
                 kFnName[fn]);
    return -1;
  }
  if ((flags & 1) && !d->O[1].ext.valid) { pl_set_error("pl_dyn_jac_sizes(%s): no external-force frame on this handle", kFnName[fn]); return -1; }
  pl::dyn_jac_tan_len(d->M, fn, d->O[flags & 1].nf, in_len, tan_len);
  for (int k = 0; k < 4; ++k)
    if (in_len[k] == 0) tan_len[k] = 0;
  *out_len = pl::dyn_out_len(d->M, fn);
  return 0;
}

extern "C" int pl_dyn_jac(pl_dyn* d, int fn, int batch, int frame, int flags, unsigned wrt, const double* in0,
                          const double* in1, const double* in2, const double* in3, double* out, double* jac) {
  const double* in[4] = {in0, in1, in2, in3};
  JacArgs A;
  PlFrameRef F;
  if (int rc = jac_prepare(d, fn, batch, frame, flags, wrt, reinterpret_cast<const void* const*>(in), jac, &A, &F)) return rc;
  if (batch == 0) return 0;
  const int lo = A.rows;
  const size_t B = batch, jl = (size_t)A.rows * A.W;
  if (d->device < 0) {  // host handle
    const PlOcpConst& O = d->O[flags & 1];
    for (size_t b = 0; b < B; ++b) {
      const double* p[4];
      for (int k = 0; k < 4; ++k) p[k] = A.len[k] ? in[k] + b * A.len[k] : nullptr;
      if (out) pl::dyn_eval(d->M, O, F, fn, flags, p[0], p[1], p[2], p[3], out + b * lo);
      pl::dyn_jac_point(d->M, O, F, fn, flags, wrt, p[0], p[1], p[2], p[3], jac + b * jl);
    }
    return 0;
  }
  (void)hipSetDevice(d->device);
  (void)hipGetLastError();
  // staging: inputs | value | Jacobian (the Jacobian is W times the value: size_t throughout)
  const size_t nin = (size_t)A.len[0] + A.len[1] + A.len[2] + A.len[3];
  if (B > (SIZE_MAX / sizeof(double)) / (nin + lo + jl)) { pl_set_error("pl_dyn_jac(%s): staging size overflows", kFnName[fn]); return -2; }
  if (int rc = pl_dyn_reserve(d, B * (nin + lo + jl))) return rc;
  const double* dptr[4];
  size_t off = 0;
  for (int k = 0; k < 4; ++k) {
    dptr[k] = A.len[k] ? d->buf + off : nullptr;
    if (A.len[k]) PL_CHECK_HIP(hipMemcpyAsync(d->buf + off, in[k], B * A.len[k] * 8, hipMemcpyHostToDevice, d->stream));
    off += B * A.len[k];
    A.in[k] = dptr[k];
  }
  double* dout = d->buf + off;
  double* djac = dout + B * lo;
  if (out) {
    if (int rc = pl_dyn_launch_eval(d, F, fn, flags, batch, dptr, A.len, dout, lo)) return rc;
    PL_CHECK_HIP(hipMemcpyAsync(out, dout, B * lo * 8, hipMemcpyDeviceToHost, d->stream));
  }
  if (int rc = jac_launch(d, F, A, djac)) return rc;
  PL_CHECK_HIP(hipMemcpyAsync(jac, djac, B * jl * 8, hipMemcpyDeviceToHost, d->stream));
  PL_CHECK_HIP(hipStreamSynchronize(d->stream));
  return 0;
}

extern "C" int pl_dyn_jac_device(pl_dyn* d, int fn, int batch, int frame, int flags, unsigned wrt, const void* in0,
                                 const void* in1, const void* in2, const void* in3, void* out, void* jac) {
  const void* in[4] = {in0, in1, in2, in3};
  JacArgs A;
  PlFrameRef F;
  if (d && d->device < 0) {
    pl_set_error("pl_dyn_jac_device(%s): the handle has no device (device = -1)",
                 fn >= 0 && fn < PL_FN_COUNT ? kFnName[fn] : "?");
    return -1;
  }
  if (int rc = jac_prepare(d, fn, batch, frame, flags, wrt, in, jac, &A, &F)) return rc;
  if (batch == 0) return 0;
  (void)hipSetDevice(d->device);
  (void)hipGetLastError();
  const double* dptr[4];
  for (int k = 0; k < 4; ++k) {
    dptr[k] = A.len[k] ? static_cast<const double*>(in[k]) : nullptr;
    A.in[k] = dptr[k];
  }
  if (out)
    if (int rc = pl_dyn_launch_eval(d, F, fn, flags, batch, dptr, A.len, static_cast<double*>(out), A.rows)) return rc;
  if (int rc = jac_launch(d, F, A, static_cast<double*>(jac))) return rc;
  PL_CHECK_HIP(hipStreamSynchronize(d->stream));
  return 0;
}
