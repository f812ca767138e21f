// Plant of the device MPC loop: after the solve of a step, every problem's true state
// d.xstate is stepped through the forward dynamics (ABA) under the torques and contact forces
// that solve commands and the problem's base wrench (plant.h).  It takes the place of
// k_mpc_finish (k_eval.hip), x_state <- integrate(x_state, DX[1]) (run_mpc.py:142), when
// pl_mpc_set_plant selects PL_PLANT_ABA, on the OSQP path (inside the captured step) and on
// the interior-point path alike.
//
// Mapping: one thread per problem, as k_mpc_finish and k_retract.  The ABA passes keep their
// per-joint arrays per thread (Ia alone is PL_MAXJ x 36 doubles; 24 272 bytes of scratch per
// lane, 209-250 VGPRs), which no register file holds, so they live in scratch whatever the
// mapping; spreading one problem's tree over lanes would turn the three sequential passes into
// cross-lane traffic for a kernel that is under 1 % of the step.  The kernel's time is one
// thread's serial chain through scratch: at the batch sizes of the loop every wave is resident
// at once.  What the mapping does choose is how many lanes of a wave share that scratch
// traffic: PL_PLANT_LANES problems per workgroup (one wave, the other lanes idle).  Measured
// on the MI355X at B2G whole_body_rnea N = 50, B = 1024 (tools/plant_timing.py,
// profiles/plant/plant_timing.json), substeps 1 / 4: 64 lanes 263 / 688 us, 32 lanes
// 223 / 599 us, 16 lanes 238 / 629 us, 8 lanes 236 / 687 us (k_mpc_finish: 32.6 us; the
// same dispatch repeated in another process differs by under 1 %).  Hence 32.
// The wrench is read from a buffer the handle owns (zero rows when none is set), so new
// values never change the launch and a captured graph replays them.
#include "plant.h"
#include "state.h"

#ifndef PL_PLANT_LANES
#define PL_PLANT_LANES 32
#endif

template <int DYN>
__global__ __launch_bounds__(64) void k_plant(PlDev d, int B, int N, int n, int np, int nx, int substeps) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;  // the last block's spare threads
  const double* p = d.p + (size_t)b * np;
  pl::plant_step(*d.model, *d.oc, DYN, d.nodes, N, p, d.x + (size_t)b * n, d.plant_w + (size_t)b * 6, substeps,
                 d.xstate + (size_t)b * nx);
}

// pl_mpc_set_plant refuses PL_PLANT_ABA on centroidal_vel (x = [h, q]), so those kinds never get here
void launch_plant(PlOcpHandle* h) {
  const dim3 grid((h->B + PL_PLANT_LANES - 1) / PL_PLANT_LANES), block(PL_PLANT_LANES);
#define PL_PLANT_CASE(DYN)                                                                                    \
  case DYN:                                                                                                   \
    hipLaunchKernelGGL(k_plant<DYN>, grid, block, 0, h->stream, h->d, h->B, h->N, h->n, h->np, h->nx,         \
                       h->plant_substeps);                                                                    \
    break;
  switch (h->oc.dyn) {
    PL_PLANT_CASE(PL_DYN_RNEA)
    PL_PLANT_CASE(PL_DYN_RNEAFD)
    PL_PLANT_CASE(PL_DYN_ACC)
    PL_PLANT_CASE(PL_DYN_ACCNB)
    PL_PLANT_CASE(PL_DYN_CA)
    PL_PLANT_CASE(PL_DYN_ABA)
    default: break;
  }
#undef PL_PLANT_CASE
}
