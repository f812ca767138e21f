// Host-side internals of the C-ABI shared by api.hip (handles, the OSQP-SQP solve, retract),
// api_ip.hip (the interior point's setup and structural probes), api_mpc.hip (the device MPC
// loop), api_debug.hip (profiling, debug access), api_build.hip (the layout / program
// builders) and api_casadi.hip (the CasADi external-function ABI).
#pragma once
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/pinoloco.h"
#include "dyn.h"
#include "handles.h"
#include "rows.h"
#include "state.h"

struct pl_ocp {
  PlOcpHandle h;
  bool on_device;
  std::vector<PlNode> nodes;
  std::vector<int> colptr, rowidx, entcol, rowptr, rowent, cplrow, rownode, colnode;
  std::vector<int> gr_ptr, gc_ptr;    // global CSR / CSC of the whole A (k_check)
  std::vector<int2> gr_ec, gc_er;     // (entry, global column) / (entry, global row)
  std::vector<PlAdmmNode> anodes;
  std::vector<uint16_t> aprog, fprog;
  std::vector<uint32_t> ttab;
  std::vector<PlFacNode> fnodes;
  std::vector<uint32_t> kasm, kcpl;
  std::vector<uint16_t> kfl;
  std::vector<double> h_params;  // host copy of the parameters (B x np)
  std::vector<void*> allocs;
  hipEvent_t ev[5];
  // pl_mpc_step replay: the launches of one OSQP-SQP MPC step after k_mpc_prepare, captured
  // once into a HIP graph and replayed while the handle's host state is unchanged
  hipGraphExec_t mpc_graph = nullptr;
  std::vector<unsigned char> mpc_key;  // bytes of `h` the graph was captured with (or last seen)
  int mpc_graph_off = 0;               // 1: capture failed or PL_PATH_NO_MPC_GRAPH: launch eagerly
  long long mpc_captures = 0;
  long long mpc_replays = 0;           // graph launches (pl_mpc_graph_info)
  // pinned staging of pl_mpc_download, pl_mpc_log_read, pl_mpc_timeline_state and pl_ocp_retract
  // (stage_reserve): each ends with a stream synchronise and a memcpy before it returns
  void* dl_host = nullptr;
  size_t dl_bytes = 0;
  // pl_ocp_retract: the packed device result, allocated on first use (here, not in `h`: the
  // bytes of `h` are the MPC graph key)
  double* rt_dev = nullptr;
  size_t rt_cap = 0;                   // doubles
};

#define REQUIRE_DEVICE(o)                                              \
  do {                                                                 \
    if (!(o) || !(o)->on_device) {                                     \
      pl_set_error("handle has no device (created with device = -1)"); \
      return -1;                                                       \
    }                                                                  \
    (void)hipSetDevice((o)->h.device);                                 \
    (void)hipGetLastError(); /* errors of earlier calls were reported there */ \
  } while (0)

template <class T>
inline int dalloc(pl_ocp* o, T** p, size_t count) {
  void* q = nullptr;
  count += 256;  // slack: kernels issue clamped, unconditional loads up to one row past the end
  hipError_t e = hipMalloc(&q, count * sizeof(T));
  if (e != hipSuccess) {
    pl_set_error("hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    return -2;
  }
  (void)hipMemset(q, 0, count * sizeof(T));
  o->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

template <class T>
inline int upload(pl_ocp* o, T** p, const std::vector<T>& v) {
  if (dalloc(o, p, v.size())) return -2;
  if (!v.empty()) PL_CHECK_HIP(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// Buffers that grow on demand and never shrink: device memory (*have and need in elements of
// T) and pinned host memory (bytes).  0 when the block is already large enough.  Otherwise the
// stream, if given, is drained (an earlier launch may still use the old block), the old block
// is freed and a new one allocated; on failure pointer and size stay null / 0, HIP's last
// error is cleared and the caller's name and the byte count are reported.  pl_ocp_destroy
// frees them from its table.
inline int grow_failed(const char* who, const char* what, size_t bytes, hipError_t e) {
  (void)hipGetLastError();
  pl_set_error("%s: %s(%zu bytes): %s", who, what, bytes, hipGetErrorString(e));
  return -2;
}

template <class T>
inline int grow_device(T** p, size_t* have, size_t need, hipStream_t stream, const char* who) {
  if (*have >= need) return 0;
  if (stream) PL_CHECK_HIP(hipStreamSynchronize(stream));
  (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  const hipError_t e = hipMalloc((void**)p, need * sizeof(T));
  if (e != hipSuccess) return grow_failed(who, "hipMalloc", need * sizeof(T), e);
  *have = need;
  return 0;
}

inline int grow_pinned(void** p, size_t* have, size_t need, hipStream_t stream, const char* who) {
  if (*have >= need) return 0;
  if (stream) PL_CHECK_HIP(hipStreamSynchronize(stream));
  (void)hipHostFree(*p);
  *p = nullptr;
  *have = 0;
  const hipError_t e = hipHostMalloc(p, need, hipHostMallocDefault);
  if (e != hipSuccess) return grow_failed(who, "hipHostMalloc", need, e);
  *have = need;
  return 0;
}

// the handle's pinned staging buffer: its users finish with it before they return
inline int stage_reserve(pl_ocp* o, size_t bytes, const char* who) {
  return grow_pinned(&o->dl_host, &o->dl_bytes, bytes, nullptr, who);
}

// api.hip: the launches of one OSQP-SQP iteration, the per-problem results, the ADMM kernel choice
int enqueue_solve(pl_ocp* o, bool timed);
int fetch_stats(pl_ocp* o, pl_stats* stats);
int admm_select(pl_ocp* o, int kind);
// api_debug.hip: fold the recorded per-launch events into the profile sums
void prof_collect(PlOcpHandle* h);
// api_build.hip: variable / row / sparsity layout and the device programs of one OCP
void build_blocks(PlOcpConst& O, bool has_ext, bool has_arm);
int build_layout(pl_ocp* o);
int build_admm_prog(pl_ocp* o);
int build_factor_prog(pl_ocp* o);
// lin (use_lin, rnea): the a / f columns, for k_eval_jac_lin, instead of tree-pass lanes in list
// n_ex: entries of list before the cheap columns (whole waves)
int build_jac_list(pl_ocp* o, std::vector<int2>& list, std::vector<int2>& lin, bool use_lin, int* n_ex);
// api_casadi.hip: drop the CasADi binding of an OCP that is being destroyed
void cas_forget(const pl_ocp* o);
// api_ip.hip: the structurally non-zero Jacobian entries of node i
void jac_pattern(const PlOcpHandle& h, const std::vector<PlNode>& nodes, int i, std::vector<uint8_t>& nz);
