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
//
// The contact instantiation (pl_mpc_set_contact: ground forces out of aba_forward's first pass,
// joint PD towards node 1) carries the joints' world positions on top: 25 712 bytes of scratch
// per lane, 230-256 VGPRs, no spills.  Same shape, same box and run
// (profiles/plant/plant_contact_timing.json), substeps 1 / 4 / 16, contact off | on:
// 32 lanes 224 / 595 / 2092 | 292 / 794 / 2734 us, 64 lanes 262 / 686 / 2385 | 341 / 902 / 3086 us,
// 16 lanes 241 / 630 / 2214 | 314 / 826 / 2848 us; the parent commit's kernel 223 / 596 / 2080 us
// (repeats of a row differ by under 1 %).  32 lanes stays the choice for both.  Contact costs
// about 38 us per substep on top of 125 us (30 %), far more than its arithmetic; staging the
// problem's parameters, ground heights, anchors and forces in the lane's own storage instead of
// the handle's buffers changed that by -1.4 % (16 substeps) to +3 % (1), so those buffers are
// not the cost and they are read and written in place (DESIGN section 3 for what is known).
#include "plant.h"
#include "state.h"

#ifndef PL_PLANT_LANES
#define PL_PLANT_LANES 32
#endif

// CONTACT (pl_mpc_set_contact): the ground's forces at the feet and the joint PD term, an
// instantiation of its own so that the plain plant compiles to what it was.  Anchors and last
// forces are read and written in place in the handle's buffers (a few doubles per substep).
template <int DYN, bool CONTACT>
__global__ __launch_bounds__(64) void k_plant(PlDev d, int B, int N, int n, int np, int nx, int substeps) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;  // the last block's spare threads
  const double* p = d.p + (size_t)b * np;
  if constexpr (CONTACT) {
    const size_t nf = d.oc->nfeet;
    pl::plant_step<true>(*d.model, *d.oc, DYN, d.nodes, N, p, d.x + (size_t)b * n, d.plant_w + (size_t)b * 6, substeps,
                         d.xstate + (size_t)b * nx, d.plant_cprm + b, d.plant_gz + b * nf, d.plant_anchor + b * nf * 3,
                         d.plant_cf + b * nf * 3);
  } else {
    pl::plant_step(*d.model, *d.oc, DYN, d.nodes, N, p, d.x + (size_t)b * n, d.plant_w + (size_t)b * 6, substeps,
                   d.xstate + (size_t)b * nx);
  }
}

// pl_mpc_set_plant refuses PL_PLANT_ABA on centroidal_vel (x = [h, q]), so those kinds never get here
void launch_plant(PlOcpHandle* h) {
  const dim3 grid((h->B + PL_PLANT_LANES - 1) / PL_PLANT_LANES), block(PL_PLANT_LANES);
#define PL_PLANT_CASE(DYN)                                                                                    \
  case DYN:                                                                                                   \
    if (h->plant_contact_on)                                                                                  \
      hipLaunchKernelGGL((k_plant<DYN, true>), grid, block, 0, h->stream, h->d, h->B, h->N, h->n, h->np,      \
                         h->nx, h->plant_substeps);                                                           \
    else                                                                                                      \
      hipLaunchKernelGGL((k_plant<DYN, false>), grid, block, 0, h->stream, h->d, h->B, h->N, h->n, h->np,     \
                         h->nx, h->plant_substeps);                                                           \
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
