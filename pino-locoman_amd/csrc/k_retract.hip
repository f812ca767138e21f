// Batched retract of the solved horizon: q, v, a, contact forces, joint torques and the base
// rows of the equations of motion of every (problem, node) from d.x and d.p.
//
// The reference retracts after every solve (retract_stacked_sol in OCP.solve, optimization/
// ocp.py:422; compile_solution, ocp_whole_body_rnea.py:326-366) and its driver recomputes
// torques and the base-wrench residual per node (run_mpc.py:186-241), one node at a time on
// the host.  Here one thread owns one (problem, node) pair, the thread-per-point mapping of
// k_dyn / k_mpc_finish, so the tree passes of retract_node (retract.h) keep their per-thread
// arrays; every problem reads its own parameters (x_init, step sizes).  A thread's result
// depends on its problem's x and p and on its node only, not on the batch or the row count.
#include "dispatch.h"
#include "retract.h"
#include "state.h"

template <int DYN>
__global__ __launch_bounds__(64) void k_retract(PlDev d, int B, int R, int N, int n, int np, pl::RetractLayout L,
                                                double* out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * R) return;  // the last block's spare threads
  const int b = idx / R, i = idx - b * R;  // R = steps (+ 1 with the terminal node, then i == N)
  const PlOcpConst& O = *d.oc;
  const double* p = d.p + (size_t)b * np;
  double* row[PL_RETRACT_FIELDS];
  for (int k = 0; k < PL_RETRACT_FIELDS; ++k)
    row[k] = (i < L.rows[k] && L.width[k] > 0) ? out + L.off[k] + ((size_t)b * L.rows[k] + i) * L.width[k] : nullptr;
  const pl::RetractOut o{row[0], row[1], row[2], row[3], row[4], row[5], 1};
  pl::retract_node(*d.model, O, DYN, d.nodes, N, p, d.x + (size_t)b * n, p + O.P.x_init, i, o);
}

// steps in [1, N]; terminal (0 / 1) needs steps == N (the callers check); out: L.total doubles
void launch_retract(PlOcpHandle* h, int steps, int terminal, double* out) {
  const pl::RetractLayout L = pl::retract_layout(h->oc, h->B, steps, terminal);
  const int R = steps + (terminal ? 1 : 0);
  const int total = h->B * R;
  PL_DISPATCH_DYN(h->oc.dyn, k_retract, dim3((total + 63) / 64), dim3(64), 0, h->stream, h->d, h->B, R, h->N, h->n,
                  h->np, L, out);
}
