// The Dynamics plugin handle (pl_dyn of include/pinoloco.h), shared by k_dyn.hip (values) and
// k_dyn_jac.hip (Jacobians).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/pinoloco.h"
#include "handles.h"
#include "model.h"

struct pl_dyn {
  const pl_model* model;
  PlModel M;
  PlOcpConst O[2];   // contact frames: [0] feet only, [1] feet + external-force frame
  int device;
  hipStream_t stream;
  PlModel* dM;
  PlOcpConst* dO;
  double* buf;
  size_t cap;        // doubles in buf
};

// k_dyn.hip: the argument checks of pl_dyn_eval (input lengths -> len, the frame -> F), the
// staging buffer, and a k_dyn launch on the handle's stream with device pointers.
int pl_dyn_prepare(const pl_dyn* d, int fn, int frame, int flags, const void* const* in, int* len, PlFrameRef* F);
int pl_dyn_reserve(pl_dyn* d, size_t need);
int pl_dyn_launch_eval(pl_dyn* d, const PlFrameRef& F, int fn, int flags, int batch, const double* const* dptr,
                       const int* len, double* dout, int lo);
