// Rollout log of the device MPC loop: after the step's sequence (the graph launch, the eager SQP
// sequence or the interior-point solve, each ending in the plant) pl_mpc_step launches
// k_mpc_record, which writes one row per problem into the log and updates the problem's outcome
// metrics (record.h has the row, the metrics and the slot rule).  It runs outside the captured
// step, as k_mpc_prepare runs before it: the step index and the log slot are plain arguments, so
// the log never touches the graph, and while the log is off nothing is launched.
//
// Mapping: one 64-lane workgroup per problem, the lanes across the row's elements.  The log is
// [slot][B][row], so a step's rows are one contiguous block and a row is row / 64 rounds of
// consecutive 8-byte stores, whole 64-byte lines apart from its two ends.  Every element is one
// read of a buffer the step left behind (parameters, iterate, PlProbInfo, x_state, the plant's
// contact buffers); nothing is recomputed, so there is no per-thread array, no scratch and no
// LDS.  Lane 0 updates the metrics: a serial pass over the nx entries of x_state its wave has
// just read.  slot < 0: metrics only (a stride step, a full log, or capacity 0).
// 18 VGPRs, no scratch (tools/kernel_resources.sh k_record).  Measured on the MI355X at B2G
// whole_body_rnea N = 50, B = 1024 (179 doubles per row, 1.47 MB per step; tools/plant_timing.py
// run --log, profiles/plant/record_timing.json): 10.0 us beside k_mpc_finish's 33.1 us in the same
// run, 9.8 us after the contact plant: launch-bound.
#include "record.h"

__global__ __launch_bounds__(64) void k_mpc_record(PlDev d, int k, long long slot, int n, int np, int nx, int nu0,
                                                   double* __restrict__ log, PlMpcMetrics* __restrict__ met,
                                                   const double* __restrict__ ref) {
  const int b = blockIdx.x, B = gridDim.x;
  const PlOcpConst& O = *d.oc;
  const int nfeet = O.nfeet;
  const double* xs = d.xstate + (size_t)b * nx;
  const pl::RecSrc S{d.p + (size_t)b * np + O.P.x_init, d.x + (size_t)b * n + O.ndx, d.info + b, xs,
                     d.plant_cf + (size_t)b * nfeet * 3, d.plant_anchor + (size_t)b * nfeet * 3};
  if (slot >= 0) {
    const pl::RecLayout L = pl::rec_layout(nx, nu0, nfeet);
    double* row = log + ((size_t)slot * B + b) * L.row;
    for (int e = threadIdx.x; e < L.row; e += 64) row[e] = pl::rec_elem(L, S, e);
  }
  if (threadIdx.x == 0) {
    PlMpcMetrics m = met[b];
    pl::rec_metrics(m, k, xs, nx, PL_IS_CV(O.dyn) ? 6 : 0, ref[b], ref[B + b], ref[2 * B + b], d.info[b]);
    met[b] = m;
  }
}

// pl_mpc_log_start: the metrics' start values and z_ref = the base height of x_state now, read
// on the device in stream order (no host copy of the state)
__global__ void k_mpc_record_start(PlDev d, int B, int nx, PlMpcMetrics* __restrict__ met, double* __restrict__ ref) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  PlMpcMetrics m;
  pl::rec_metrics_reset(m);
  met[b] = m;
  ref[b] = d.xstate[(size_t)b * nx + (PL_IS_CV(d.oc->dyn) ? 6 : 0) + 2];
}

void launch_mpc_record(PlOcpHandle* h, int k, long long slot, int nu0) {
  hipLaunchKernelGGL(k_mpc_record, dim3(h->B), dim3(64), 0, h->stream, h->d, k, slot, h->n, h->np, h->nx, nu0,
                     h->rec_log, h->rec_met, (const double*)h->rec_ref);
}

void launch_mpc_record_start(PlOcpHandle* h) {
  hipLaunchKernelGGL(k_mpc_record_start, dim3((h->B + 63) / 64), dim3(64), 0, h->stream, h->d, h->B, h->nx,
                     h->rec_met, h->rec_ref);
}
