// OSQP adaptive rho on the device (the rule: rho_adapt.h; sequencing: api.hip enqueue_solve).
//
// Every problem holds its own rho (PlRhoAdapt::rho_b).  After a termination check whose
// iteration is a multiple of the interval, k_rho_adapt re-estimates it from the scaled residual
// norms that k_check_part<true> left per node, and, where the estimate leaves the tolerance
// band, rewrites the problem's d.rho / d.rhoc rows and flags the problem for the masked
// refactor that follows (k_fnode, k_fchain, k_fred and the rhs rebuild skip unflagged problems).
// Nothing here synchronises with the host: the flag lives in device memory.
#include <algorithm>

#include "rho_adapt.h"
#include "state.h"

namespace {

// d.rho of problem b's rows and d.rhoc of its coupling rows from the scaled bounds (the
// classes of k_qp_finish with the problem's rho); any block size
__device__ void rho_write_rows(const PlDev& d, int b, int N, int m, int ncpl_max, double rho_b) {
  const double* ls = d.ls + (size_t)b * m;
  const double* us = d.us + (size_t)b * m;
  double* rho = d.rho + (size_t)b * m;
  for (int r = threadIdx.x; r < m; r += blockDim.x) rho[r] = pl::rho_row(ls[r], us[r], rho_b);
  double* rhoc = d.rhoc + (size_t)b * (N + 1) * ncpl_max;
  for (int i = 0; i < N; ++i) {
    const PlNode& nd = d.nodes[i];
    for (int s = threadIdx.x; s < nd.ncpl; s += blockDim.x) {
      const int r = nd.row_off + d.cplrow[nd.cpl_off + s];
      rhoc[(size_t)i * ncpl_max + s] = pl::rho_row(ls[r], us[r], rho_b);
    }
  }
}

}  // namespace

__global__ __launch_bounds__(64) void k_rho_reset(PlRhoAdapt ra, int B, double rho, int full) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (full) {
    ra.rho_b[b] = rho;
    ra.rho_est[b] = rho;
  }
  ra.nupd[b] = 0;
  ra.mask[b].active = 0;
  for (int k = 0; k < PL_RHO_LOG; ++k) ra.upd_it[(size_t)b * PL_RHO_LOG + k] = 0.0;
}

__global__ __launch_bounds__(256) void k_rho_rows(PlDev d, PlRhoAdapt ra, int N, int m, int ncpl_max) {
  const int b = blockIdx.x;
  rho_write_rows(d, b, N, m, ncpl_max, ra.rho_b[b]);
}

// One wave per problem.  final_check: the check at max_iter -- the problems its approximate
// pass closed (the exact pass did not terminate them) still adapt, for the next solve; no
// refactor follows, so no flag.
__global__ __launch_bounds__(64) void k_rho_adapt(PlDev d, PlRhoAdapt ra, int N, int m, int ncpl_max, int it,
                                                  int final_check) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int done = d.info[b].done, status = d.info[b].status;
  // statuses only the approximate pass gives (k_qp.hip): solved / infeasible inaccurate, max_iter
  const bool approx_end = status == 2 || status == 3 || status == 4 || status == -2;
  const bool adapt = final_check ? (done && approx_end) : !done;
  if (!adapt) {  // uniform over the workgroup
    if (lane == 0) ra.mask[b].active = 0;
    return;
  }
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i <= N; i += 64) {
    const double* s = ra.sn + ((size_t)b * (N + 1) + i) * 8;
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = pl::rho_nmax(v[k], s[k]);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = pl::rho_nmax(v[k], __shfl_xor(v[k], s, 64));
  const double rho = ra.rho_b[b];
  const double est = pl::rho_estimate(v, rho);
  const bool upd = pl::rho_update(est, rho, ra.tol);  // the same bits on every lane
  if (lane == 0) {
    ra.rho_est[b] = est;
    ra.mask[b].active = (upd && !final_check) ? 1 : 0;
    if (upd) {
      const int k = ra.nupd[b];
      ra.rho_b[b] = est;
      ra.nupd[b] = k + 1;
      if (k < PL_RHO_LOG) ra.upd_it[(size_t)b * PL_RHO_LOG + k] = (double)it;
    }
  }
  // at the last check d.rho stays what the factor was built with; the next solve's
  // launch_rho_rows writes the rows from the new rho_b
  if (upd && !final_check) rho_write_rows(d, b, N, m, ncpl_max, est);
}

void launch_rho_reset(PlOcpHandle* h, int full) {
  hipLaunchKernelGGL(k_rho_reset, dim3((h->B + 63) / 64), dim3(64), 0, h->stream, h->ra, h->B, h->set.rho, full);
}

void launch_rho_rows(PlOcpHandle* h) {
  hipLaunchKernelGGL(k_rho_rows, dim3(h->B), dim3(256), 0, h->stream, h->d, h->ra, h->N, h->m,
                     std::max(h->ncpl_max, 1));
}

void launch_rho_adapt(PlOcpHandle* h, int it, int final_check) {
  hipLaunchKernelGGL(k_rho_adapt, dim3(h->B), dim3(64), 0, h->stream, h->d, h->ra, h->N, h->m,
                     std::max(h->ncpl_max, 1), it, final_check);
}
