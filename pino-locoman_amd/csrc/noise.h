// Per-step random state noise and base wrench of the device MPC loop (host+device): what the
// gait / warm-start launch (k_mpc_prepare) draws before MPC step k while pl_mpc_set_noise holds
// seeds, and the host restatement pl_mpc_noise_host runs.  The reference sketches the state noise
// as a fresh Gaussian draw on x_init at every step (run_mpc.py:79-82).
//
// The generator is counter-based, Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random
// numbers: as easy as 1, 2, 3", SC'11): a draw is a pure function of (problem seed, stream, step k,
// component).  It keeps no state, so it does not depend on the batch size, the problem's slot, the
// launch geometry, the steps that ran before or the GPU that holds the shard.
//   block address   counter (k, i, stream, 0), key (seed & 0xffffffff, seed >> 32); k the MPC
//                   step (>= 0), i the block inside the stream, stream 0 the state noise, 1 the
//                   base wrench
//   uniforms        of the block's words w0..w3: U(a, b) = ((a >> 5) 2^26 + (b >> 6)) 2^-53, exact
//                   in a double, in [0, 1);  u1 = 1 - U(w0, w1), exact, in (0, 1];
//                   theta = 0x1.921fb54442d18p+2 U(w2, w3), one rounding
//   normals         Box-Muller, two per block: r = sqrt(-2 log u1), z_{2i} = r cos theta,
//                   z_{2i+1} = r sin theta; component j of a stream is normal j & 1 of block j >> 1
//   noise_j         sigma_j z_j, j < ndx, stream 0
//   wrench_c        det_c + sigma_w,c z_c, c < 6, stream 1, product and sum each rounded (never
//                   fused); det is the push window's wrench of the step, zero without a schedule
// The integer part and the uniforms are bit-exact everywhere; log, cos and sin are the build's
// libm, so host and device normals agree within a few ulp.
// One definition for k_mpc_prepare, k_rng_blocks (k_eval.hip) and the host.
#pragma once
#include <stdint.h>

#include "rows.h"
#include "state.h"

#define PL_RNG_STREAM_STATE 0u
#define PL_RNG_STREAM_WRENCH 1u

namespace pl {

// high word of a 32 x 32 bit product
PL_HD uint32_t rng_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

PL_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = rng_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = rng_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// block (c0 = k, c1 = i, c2 = stream, c3) of a problem's seed; the loop's draws have c3 = 0
PL_HD void rng_block(unsigned long long seed, uint32_t k, uint32_t i, uint32_t stream, uint32_t c3, uint32_t out[4]) {
  const uint32_t ctr[4] = {k, i, stream, c3};
  const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
  philox4x32_10(ctr, key, out);
}

// 53 bits of two words as a double in [0, 1): exact
PL_HD double rng_uniform(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * 0x1p-53;
}

PL_HD void rng_uniforms(const uint32_t w[4], double* u1, double* theta) {
  *u1 = 1.0 - rng_uniform(w[0], w[1]);
  *theta = 0x1.921fb54442d18p+2 * rng_uniform(w[2], w[3]);
}

// standard normal: component j of `stream` at step k
PL_HD double rng_normal(unsigned long long seed, int k, uint32_t stream, int j) {
  uint32_t w[4];
  rng_block(seed, (uint32_t)k, (uint32_t)(j >> 1), stream, 0u, w);
  double u1, theta;
  rng_uniforms(w, &u1, &theta);
  const double r = sqrt(-2.0 * log(u1));
  return (j & 1) ? r * sin(theta) : r * cos(theta);
}

PL_HD double noise_state(unsigned long long seed, int k, int j, double sigma) {
  return sigma * rng_normal(seed, k, PL_RNG_STREAM_STATE, j);
}

PL_HD double noise_wrench(unsigned long long seed, int k, int c, double det, double sigma) {
#pragma clang fp contract(off)  // product and sum each rounded, on the host and on the device
  const double s = sigma * rng_normal(seed, k, PL_RNG_STREAM_WRENCH, c);
  return det + s;
}

// The measured state the MPC plans from: x_init = state_integrate(x_state, noise), the "add noise to
// x_init" of run_mpc.py:79-82; x = [q, v], or centroidal_vel's x = [h, q]
// (dynamics_centroidal_vel.py:12-26).
PL_HD void noise_x_init(const PlModel& M, const PlOcpConst& O, const double* xs, const double* nb, double* xi) {
  if (PL_IS_CV(O.dyn)) {
    VecIn<double> acc{nb + 6, nullptr, 0.0, -1};
    for (int j = 0; j < 6; ++j) xi[j] = xs[j] + nb[j];
    integrate_q<double>(M, xs + 6, acc, xi + 6);
  } else {
    VecIn<double> acc{nb, nullptr, 0.0, -1};
    integrate_q<double>(M, xs, acc, xi);
    for (int j = 0; j < O.nv; ++j) xi[O.nq + j] = xs[O.nq + j] + nb[O.nv + j];
  }
}

// One problem's draw of step k and its x_init on the host (pl_mpc_noise_host).  A null sigma is a
// stream that is off: the noise is zero and x_init the plain copy of x_state that k_mpc_prepare
// makes then; the wrench is det.  Any output may be null; x_init needs x_state.
inline void noise_prepare_host(const PlModel& M, const PlOcpConst& O, int nx, int k, unsigned long long seed,
                               const double* state_sigma, const double* wrench_sigma, const double* det,
                               const double* x_state, double* state_noise, double* base_wrench, double* x_init) {
  double nb[2 * PL_MAXV] = {0.0};  // ndx <= 2 nv
  for (int j = 0; state_sigma && j < O.ndx; ++j) nb[j] = noise_state(seed, k, j, state_sigma[j]);
  for (int j = 0; state_noise && j < O.ndx; ++j) state_noise[j] = nb[j];
  for (int c = 0; base_wrench && c < 6; ++c) {
    const double dc = det ? det[c] : 0.0;
    base_wrench[c] = wrench_sigma ? noise_wrench(seed, k, c, dc, wrench_sigma[c]) : dc;
  }
  if (!x_init || !x_state) return;
  if (state_sigma) noise_x_init(M, O, x_state, nb, x_init);
  else
    for (int j = 0; j < nx; ++j) x_init[j] = x_state[j];
}

}  // namespace pl
