// C-ABI of the batched MPC inner loop (include/pinoloco.h).
//
// Host side of the drop-in boundary: owns the device buffers of a batch and sequences
// the kernels of one SQP iteration exactly as OCP.solve() sequences sqp_data ->
// osqp.update -> osqp.solve -> line search (ocp.py:375-414).  The layout the reference gets
// from CasADi Opti (optimization/ocp.py:38-44, 103-198, 283, 305) and the device programs are
// built in api_build.hip; the interior-point setup is api_ip.hip, the device MPC loop
// api_mpc.hip, profiling and the test hooks api_debug.hip, the CasADi external-function ABI
// api_casadi.hip.
#include "api_internal.h"
#include "retract.h"
#include "rho_adapt.h"

static thread_local char g_err[1024] = "";

void pl_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}



extern "C" const char* pl_last_error(void) { return g_err; }
// 2: pl_mpc_set_timeline and its siblings, pl_debug_mpc_prepare; 3: pl_mpc_set_noise and its
// siblings, pl_rng_*_host, pl_debug_rng
extern "C" int pl_version(void) { return 3; }

// Build provenance: build.py passes the sha256 of csrc/* + include/*.h (PL_SRC_SHA), so a
// caller can tell which sources a pushed binary was built from (bench.py prints it,
// __graft_entry__.smoke() asserts it against the tree).
#ifndef PL_SRC_SHA
#define PL_SRC_SHA "unknown"
#endif
extern "C" const char* pl_build_info(void) { return "pl_src_sha256=" PL_SRC_SHA " arch=gfx950"; }

// ---------------------------------------------------------------------------
// model
extern "C" int pl_model_create(const pl_model_desc* d, pl_model** out) {
  if (!d || !out) { pl_set_error("null argument"); return -1; }
  if (d->njoints > PL_MAXJ || d->nq > PL_MAXQ || d->nv > PL_MAXV) {
    pl_set_error("model too large (njoints=%d nq=%d nv=%d)", d->njoints, d->nq, d->nv);
    return -1;
  }
  pl_model* M = new pl_model();
  PlModel& m = M->m;
  memset(&m, 0, sizeof(m));
  m.njoints = d->njoints;
  m.nq = d->nq;
  m.nv = d->nv;
  int iq = 0, iv = 0;
  m.total_mass = 0.0;
  for (int j = 0; j < d->njoints; ++j) {
    m.parent[j] = d->parent[j];
    m.jtype[j] = d->jtype[j];
    for (int k = 0; k < 3; ++k) m.axis[j][k] = d->axis[3 * j + k];
    for (int k = 0; k < 9; ++k) m.jR[j][k] = d->placement_R[9 * j + k];
    for (int k = 0; k < 3; ++k) m.jp[j][k] = d->placement_p[3 * j + k];
    m.mass[j] = d->mass[j];
    for (int k = 0; k < 3; ++k) m.lever[j][k] = d->lever[3 * j + k];
    for (int k = 0; k < 9; ++k) m.Ic[j][k] = d->inertia[9 * j + k];
    m.total_mass += d->mass[j];
    if (j == 0) continue;
    m.idx_q[j] = iq;
    m.idx_v[j] = iv;
    if (m.jtype[j] == PL_JT_FREEFLYER) {
      if (j != 1) { pl_set_error("free-flyer must be joint 1"); delete M; return -1; }
      iq += 7;
      iv += 6;
    } else if (m.jtype[j] == PL_JT_REVOLUTE) {
      iq += 1;
      iv += 1;
      const double* a = m.axis[j];
      if (a[0] == 1.0 && a[1] == 0.0 && a[2] == 0.0) m.axis_kind[j] = PL_AX_X;
      else if (a[0] == 0.0 && a[1] == 1.0 && a[2] == 0.0) m.axis_kind[j] = PL_AX_Y;
      else if (a[0] == 0.0 && a[1] == 0.0 && a[2] == 1.0) m.axis_kind[j] = PL_AX_Z;
      else m.axis_kind[j] = PL_AX_GEN;
    } else {
      pl_set_error("unsupported joint type %d at joint %d", m.jtype[j], j);
      delete M;
      return -1;
    }
  }
  if (iq != d->nq || iv != d->nv || d->jtype[1] != PL_JT_FREEFLYER) {
    pl_set_error("inconsistent nq/nv or missing free-flyer root");
    delete M;
    return -1;
  }
  for (int k = 0; k < 3; ++k) m.gravity[k] = d->gravity[k];
  // chains: every non-root joint's parent is the root or the previous joint, and
  // only the root branches (utils/robot.py robots: 4 legs + optional arm)
  std::vector<int> nchild(d->njoints, 0);
  for (int j = 2; j < d->njoints; ++j) nchild[m.parent[j]]++;
  m.nchains = 0;
  for (int j = 2; j < d->njoints; ++j) {
    const int p = m.parent[j];
    if (p == 1) {
      if (m.nchains >= PL_MAXCHAIN) { pl_set_error("too many chains"); delete M; return -1; }
      m.chain_first[m.nchains] = j;
      m.chain_len[m.nchains] = 1;
      m.nchains++;
    } else if (p == j - 1 && nchild[p] == 1 && m.nchains > 0) {
      m.chain_len[m.nchains - 1]++;
      if (m.chain_len[m.nchains - 1] > PL_MAXCL) { pl_set_error("chain too long"); delete M; return -1; }
    } else {
      pl_set_error("joint %d breaks the root+chains tree shape", j);
      delete M;
      return -1;
    }
  }
  M->nframes = d->nframes;
  M->frame_parent.assign(d->frame_parent, d->frame_parent + d->nframes);
  M->frame_R.assign(d->frame_R, d->frame_R + 9 * d->nframes);
  M->frame_p.assign(d->frame_p, d->frame_p + 3 * d->nframes);
  *out = M;
  return 0;
}

extern "C" void pl_model_destroy(pl_model* m) { delete m; }


// ADMM kernel selection (the three give the same iterates to round-off):
//   sweep   k_admm: one wave per problem, node-by-node block sweeps (HBM-bound at B >= 1024)
//   sweep2  k_admm2: two waves per problem
//   chain   k_admm_rc: reduced chain, 8 waves per problem (small batches); up to ceil((N + 1) / 8)
//           workgroups per problem while the batch's workgroups fit one per CU (rc_groups)
// AUTO: chain up to PL_ADMM_CHAIN_MAX_B problems when supported, else sweep2 up to 512
// problems (idle SIMDs below 4 x 256), else sweep.  The chain
// buffers are allocated on first selection.
#define PL_ADMM_CHAIN_MAX_B 256  // measured: profiles/r03b (B2 aba B=256 13.8 -> 5.3 ms per launch; B2G at 512 the sweep2 wins)
int admm_select(pl_ocp* o, int kind) {
  PlOcpHandle& h = o->h;
  if (kind == PL_ADMM_AUTO) {
    if (h.B <= PL_ADMM_CHAIN_MAX_B && admm_rc_supported(&h)) kind = PL_ADMM_CHAIN;
    else kind = (h.B <= 512 && admm2_supported(&h)) ? PL_ADMM_SWEEP2 : PL_ADMM_SWEEP;
  }
  if (kind == PL_ADMM_SWEEP2 && !admm2_supported(&h)) { pl_set_error("sweep2 ADMM kernel does not support this OCP"); return -1; }
  if (kind == PL_ADMM_CHAIN && !admm_rc_supported(&h)) { pl_set_error("chain ADMM kernel does not support this OCP"); return -1; }
  if (kind == PL_ADMM_CHAIN && o->on_device && !h.d.CH) {
    if (dalloc(o, &h.d.CH, (size_t)h.B * h.ch_stride) || dalloc(o, &h.d.chv, (size_t)h.B * h.chv_stride) ||
        dalloc(o, &h.d.rcsync, (size_t)h.B * PL_RC_SYNC))
      return -2;
  }
  h.admm_rc = kind == PL_ADMM_CHAIN ? 1 : 0;
  h.admm_waves = kind == PL_ADMM_SWEEP2 ? 2 : 1;
  return 0;
}

extern "C" int pl_ocp_create(const pl_model* model, const pl_ocp_desc* d, int batch, int device, pl_ocp** out) {
  if (!model || !d || !out || batch <= 0) { pl_set_error("bad arguments"); return -1; }
  if (d->dynamics < 0 || d->dynamics > 4) { pl_set_error("Unknown dynamics type: %d", d->dynamics); return -1; }
  // nodes >= 2 is also what k_admm's software pipeline relies on (the prefetch / deferred-store
  // invariant in its header: steps q - 1 and q + 1 never meet at a node both touch)
  if (d->nodes < 2 || d->n_feet != 4) { pl_set_error("need nodes >= 2 and 4 feet"); return -1; }
  if (d->debug_paths & ~PL_PATH_ALL) {
    pl_set_error("debug_paths 0x%x has bits outside PL_PATH_* (0x%x): zero the pl_ocp_desc", d->debug_paths, PL_PATH_ALL);
    return -1;
  }
  pl_ocp* o = new pl_ocp();
  PlOcpHandle& h = o->h;
  memset(&h, 0, sizeof(h));
  h.model = model->m;
  PlOcpConst& O = h.oc;
  memset(&O, 0, sizeof(O));
  const PlModel& M = h.model;
  O.dyn = d->dynamics;
  // whole_body_acc / centroidal_acc without the base in u share the ACCNB rows
  if ((O.dyn == PL_DYN_ACC || O.dyn == PL_DYN_CA) && !d->include_base) O.dyn = PL_DYN_ACCNB;
  // centroidal_vel without the base velocity in u (the class default, ocp_centroidal_vel.py:9-23)
  if (O.dyn == PL_DYN_CV && !d->include_base) O.dyn = PL_DYN_CVNB;
  // whole_body_rnea with finite-difference accelerations (include_acc = False,
  // ocp_whole_body_rnea.py:21-26, 183-191): u = [f | tau_j], no dv_{i+1} rows; the RNEA rows
  // of node i read dv_{i+1}, so the factor takes the general coupling program (fac_gc)
  if (O.dyn == PL_DYN_RNEA && !d->include_acc) O.dyn = PL_DYN_RNEAFD;
  O.N = d->nodes;
  O.nq = M.nq;
  O.nv = M.nv;
  O.nj = M.nq - 7;
  O.nfeet = 4;
  const bool has_ext = d->ext_force_frame >= 0;
  const bool has_arm = d->arm_ee_frame >= 0;
  O.nf = 12 + (has_ext ? 3 : 0);
  O.nee = 4 + (has_ext ? 1 : 0);
  const bool cv = PL_IS_CV(O.dyn);
  O.nx = cv ? 6 + M.nq : M.nq + M.nv;   // centroidal_vel: x = [h, q] (ocp_centroidal_vel.py:50-52)
  O.ndx = cv ? 6 + M.nv : 2 * M.nv;
  O.na = (O.dyn == PL_DYN_RNEA || O.dyn == PL_DYN_ACC || O.dyn == PL_DYN_CA) ? M.nv
         : (O.dyn == PL_DYN_ACCNB ? M.nq - 7 : 0);
  O.tau_nodes = PL_IS_RNEA(O.dyn) ? d->tau_nodes : 0;
  O.mu = d->mu;
  for (int k = 0; k < 4; ++k) O.feet[k] = frame_ref(model, d->foot_frames[k]);
  O.ext = frame_ref(model, d->ext_force_frame);
  O.arm = frame_ref(model, d->arm_ee_frame);
  O.base = frame_ref(model, d->base_frame);
  if (has_arm && !O.base.valid) { pl_set_error("arm velocity needs the base_link frame"); delete o; return -1; }
  for (int k = 0; k < M.nq; ++k) O.q0[k] = d->q0[k];
  for (int k = 0; k < O.nj; ++k) {
    O.pos_min[k] = d->joint_pos_min[k];
    O.pos_max[k] = d->joint_pos_max[k];
    O.vel_max[k] = d->joint_vel_max[k];
    O.tau_max[k] = d->joint_torque_max[k];
  }
  build_blocks(O, has_ext, has_arm);
  // parameter layout (Opti declaration order)
  int off = 0;
  auto take = [&](int len) { int r = off; off += len; return r; };
  const int nu0 = pl::node_nu(O, 0);
  O.P.x_init = take(O.nx);
  O.P.dt_min = take(1);
  O.P.dt_max = take(1);
  O.P.contact = take(4 * O.N);
  O.P.swing = take(4 * O.N);
  O.P.n_contacts = take(1);
  O.P.swing_period = take(1);
  O.P.swing_height = take(1);
  O.P.swing_vel_limits = take(2);
  O.P.Q_diag = take(O.ndx);
  O.P.R_diag = take(nu0);
  O.P.base_vel_des = take(6);
  O.P.ext_force_des = take(3);
  O.P.arm_vel_des = take(3);
  if (PL_IS_RNEA(O.dyn)) {
    O.P.tau_prev = take(O.nj);
    O.P.W_diag = take(O.nj);
  } else {
    O.P.tau_prev = O.P.W_diag = -1;
  }
  O.P.np = off;
  if (build_layout(o) || build_admm_prog(o) || build_factor_prog(o)) { delete o; return -1; }
  O.n = h.n;
  O.m = h.m;
  h.B = batch;
  h.N = O.N;
  h.np = O.P.np;
  h.nx = O.nx;
  h.ndx = O.ndx;
  h.set.rho = d->rho;
  h.set.sigma = d->sigma;
  h.set.alpha = d->alpha;
  h.set.eps_abs = d->eps_abs;
  h.set.eps_rel = d->eps_rel;
  h.set.eps_prim_inf = d->eps_prim_inf;
  h.set.eps_dual_inf = d->eps_dual_inf;
  h.set.max_iter = d->max_iter;
  h.set.scaling = d->scaling;
  h.set.check_termination = d->check_termination;
  h.set.warm_start = d->warm_start;
  h.sqp_iters = 1;
  h.plant_mode = PL_PLANT_NOMINAL;  // pl_mpc_set_plant / pl_mpc_set_disturbance: the loop follows its own plan
  h.plant_substeps = 1;
  h.plant_noise_on = 0;
  h.plant_contact_on = 0;
  h.solver = PL_SOLVER_OSQP;
  // Fatrop settings of the reference (ocp.py:254-262) + the restatement's constants
  // (oracle/ip_ref.py IP_SETTINGS)
  h.ip = PlIpSettings{1e-3, 1e-4, 1e-7, 1e-2, 1e-8, 1e-4, 10, 12, 8, 0, 1e-7};
  h.ip_hess = PL_IP_HESS_EXACT;  // the Lagrangian Hessian (pl_ip_settings.hessian)
  // ADMM kernel (admm_select below): the batch-size rule at creation, pl_ocp_set_admm_kernel
  // afterwards.  No environment variable changes a kernel path: the reference paths of the
  // regression tests and the phase timing are pl_ocp_desc.debug_paths bits.
  h.debug_paths = d->debug_paths;
  h.admm_waves = 1;
  h.admm_rc = 0;
  h.admm_operands = PL_ADMM_OPERANDS_FUSED;  // pl_ocp_set_admm_operands: _SPLIT is the earlier path
  h.admm_rho_rule = 0;                       // nothing has written d.rho yet
  h.ra.tol = 5.0;                            // adaptive rho: off (pl_ocp_set_adaptive_rho), OSQP's tolerance
  h.rc_waves = 8;
  h.ruiz_fused = !(h.debug_paths & PL_PATH_RUIZ_PER_PASS);
  h.ch_stride = rc_ch_stride(h.N, h.ndx, h.rc_waves);
  h.chv_stride = rc_chv_stride(h.N, h.ndx);
  h.gait_type = d->gait_type;
  h.gait_period = d->gait_period;
  h.swing_period = d->gait_type == 0 ? 0.5 * d->gait_period : (d->gait_type == 1 ? 0.25 * d->gait_period : d->gait_period);
  o->h_params.assign((size_t)batch * h.np, 0.0);
  o->on_device = device >= 0;
  h.device = device;
  if (!o->on_device) { *out = o; return 0; }

  if (hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();  // do not leave the failure as the thread's sticky last error
    pl_set_error("hipSetDevice(%d) failed", device);
    delete o;
    return -2;
  }
  if (hipDeviceGetAttribute(&h.num_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h.num_cu <= 0)
    h.num_cu = 1;  // unknown: k_admm_rc then runs one workgroup per problem
  if (hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking) != hipSuccess) {
    pl_set_error("hipStreamCreate failed");
    delete o;
    return -2;
  }
  for (int k = 0; k < 5; ++k) hipEventCreate(&o->ev[k]);
  PlDev& D = h.d;
  const size_t B = batch;
  int rc = 0;
  rc |= dalloc(o, &D.model, 1);
  rc |= dalloc(o, &D.oc, 1);
  rc |= upload(o, &D.nodes, o->nodes);
  rc |= upload(o, &D.colptr, o->colptr);
  rc |= upload(o, &D.rowidx, o->rowidx);
  rc |= upload(o, &D.entcol, o->entcol);
  rc |= upload(o, &D.rowptr, o->rowptr);
  rc |= upload(o, &D.rowent, o->rowent);
  rc |= upload(o, &D.cplrow, o->cplrow);
  rc |= upload(o, &D.rownode, o->rownode);
  rc |= upload(o, &D.colnode, o->colnode);
  rc |= upload(o, &D.gr_ptr, o->gr_ptr);
  rc |= upload(o, &D.gr_ec, o->gr_ec);
  rc |= upload(o, &D.gc_ptr, o->gc_ptr);
  rc |= upload(o, &D.gc_er, o->gc_er);
  {  // node-local (row, column) of each entry: the entry-order residual gathers of k_check_part
    std::vector<uint32_t> erl(h.nnz);
    for (int e = 0; e < h.nnz; ++e) erl[e] = ((uint32_t)o->rowidx[e] << 16) | (uint32_t)o->entcol[e];
    rc |= upload(o, &D.erl, erl);
  }
  if (h.n < 65536 && h.m < 65536) {  // entry coordinates of the fused Ruiz kernel (k_qp.hip)
    std::vector<uint32_t> erc(h.nnz);
    for (int i = 0; i < h.N; ++i) {
      const PlNode& nd = o->nodes[i];
      for (int e = 0; e < nd.nent; ++e) {
        const int lc = o->entcol[nd.ent_off + e];
        const int r = nd.row_off + o->rowidx[nd.ent_off + e];
        const int j = lc < nd.nw ? nd.x_off + lc : o->nodes[i + 1].x_off + (lc - nd.nw);
        erc[nd.ent_off + e] = ((uint32_t)r << 16) | (uint32_t)j;
      }
    }
    rc |= upload(o, &D.erc, erc);
  }
  rc |= upload(o, &D.anodes, o->anodes);
  rc |= upload(o, &D.aprog, o->aprog);
  rc |= upload(o, &D.fprog, o->fprog);
  rc |= upload(o, &D.ttab, o->ttab);
  rc |= upload(o, &D.fnodes, o->fnodes);
  rc |= upload(o, &D.kasm, o->kasm);
  rc |= upload(o, &D.kfl, o->kfl);
  rc |= upload(o, &D.kcpl, o->kcpl);
  {
    std::vector<int2> jl, jlin;
    // PL_PATH_JAC_DUAL_ALL keeps the rnea a / f columns as dual tree-pass lanes (the r03 path)
    const bool use_lin = !(h.debug_paths & PL_PATH_JAC_DUAL_ALL);
    if (build_jac_list(o, jl, jlin, use_lin, &h.jl_ex)) {
      pl_ocp_destroy(o);
      return -1;
    }
    h.jl_len = (int)jl.size();
    h.jlin_len = (int)jlin.size();
    rc |= upload(o, &D.jlist, jl);
    D.jlin = nullptr;
    D.model0 = nullptr;
    if (!jlin.empty()) {
      rc |= upload(o, &D.jlin, jlin);
      PlModel m0 = h.model;  // zero gravity: the primal RNEA pass is then linear in (a, f)
      for (int k = 0; k < 3; ++k) m0.gravity[k] = 0.0;
      rc |= dalloc(o, &D.model0, 1);
      if (!rc && hipMemcpy(D.model0, &m0, sizeof(PlModel), hipMemcpyHostToDevice) != hipSuccess) rc = 1;
    }
  }
  const size_t n = h.n, m = h.m, nnz = h.nnz;
  rc |= dalloc(o, &D.p, B * h.np);
  rc |= dalloc(o, &D.x, B * n);
  rc |= dalloc(o, &D.x0, B * n);
  rc |= dalloc(o, &D.g, B * m);
  rc |= dalloc(o, &D.lbg, B * m);
  rc |= dalloc(o, &D.ubg, B * m);
  rc |= dalloc(o, &D.grad, B * n);
  rc |= dalloc(o, &D.Araw, B * nnz);
  rc |= dalloc(o, &D.P, B * n);
  rc |= dalloc(o, &D.As, B * nnz);
  rc |= dalloc(o, &D.qs, B * n);
  rc |= dalloc(o, &D.ls, B * m);
  rc |= dalloc(o, &D.us, B * m);
  rc |= dalloc(o, &D.rho, B * m);
  rc |= dalloc(o, &D.rhoc, B * (size_t)(h.N + 1) * std::max(h.ncpl_max, 1));
  rc |= dalloc(o, &D.Acpl, B * (size_t)(h.N + 1) * PL_ACPL);
  rc |= dalloc(o, &D.D, B * n);
  rc |= dalloc(o, &D.E, B * m);
  rc |= dalloc(o, &D.cs, B);
  rc |= dalloc(o, &D.Ps, B * n);
  rc |= dalloc(o, &D.xa, B * n);
  rc |= dalloc(o, &D.za, B * m);
  rc |= dalloc(o, &D.ya, B * m);
  rc |= dalloc(o, &D.rhs, B * n);
  rc |= dalloc(o, &D.bt, B * n);
  rc |= dalloc(o, &D.dxs, B * n);
  rc |= dalloc(o, &D.dys, B * m);
  rc |= dalloc(o, &D.aty, B * n);
  rc |= dalloc(o, &D.step, B * n);
  rc |= dalloc(o, &D.S, B * (size_t)h.S_stride);
  rc |= dalloc(o, &D.FS, B * (size_t)h.fs_stride);
  rc |= dalloc(o, &D.work, B * 8);
  rc |= dalloc(o, &D.chk, B * (size_t)(h.N + 1) * 8);
  rc |= dalloc(o, &D.info, B);
  rc |= dalloc(o, &D.t0, B);
  rc |= dalloc(o, &D.xstate, B * (size_t)h.nx);
  // the plant's disturbances (pl_mpc_set_disturbance), zeroed: allocated here so that their
  // pointers, part of the MPC graph's launches, never change
  rc |= dalloc(o, &D.plant_w, B * 6);
  rc |= dalloc(o, &D.plant_noise, B * (size_t)h.ndx);
  // the plant's contact data (pl_mpc_set_contact), zeroed, for the same reason
  rc |= dalloc(o, &D.plant_cprm, B);
  rc |= dalloc(o, &D.plant_gz, B * (size_t)h.oc.nfeet);
  rc |= dalloc(o, &D.plant_anchor, B * (size_t)h.oc.nfeet * 3);
  rc |= dalloc(o, &D.plant_cf, B * (size_t)h.oc.nfeet * 3);
  D.dbg = nullptr;
  if (h.debug_paths & PL_PATH_ADMM_TIMING) rc |= dalloc(o, &D.dbg, B * 40);
  if (rc) { pl_ocp_destroy(o); return -2; }
  if (admm_select(o, PL_ADMM_AUTO)) { pl_ocp_destroy(o); return -2; }
  o->mpc_graph_off = (h.debug_paths & PL_PATH_NO_MPC_GRAPH) != 0;
  // the cheap Jacobian columns (dx_{i+1}, rnea tau_j, centroidal_vel h) have constant entries
  // (+-1, -m): written by the first evaluation only (PL_PATH_JAC_CONST_EVERY: every evaluation)
  o->h.jac_cheap_every = (h.debug_paths & PL_PATH_JAC_CONST_EVERY) != 0;
  o->h.jac_cheap_ok = 0;
  if (hipMemcpy(D.model, &h.model, sizeof(PlModel), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(D.oc, &h.oc, sizeof(PlOcpConst), hipMemcpyHostToDevice) != hipSuccess) {
    pl_set_error("upload of model tables failed");
    pl_ocp_destroy(o);
    return -2;
  }
  *out = o;
  return 0;
}


extern "C" void pl_ocp_destroy(pl_ocp* o) {
  if (!o) return;
  cas_forget(o);  // a bound CasADi handle must not outlive its OCP
  if (o->on_device) {
    hipSetDevice(o->h.device);
    hipStreamSynchronize(o->h.stream);
    for (void* p : o->allocs) hipFree(p);
    for (int k = 0; k < 5; ++k) hipEventDestroy(o->ev[k]);
    if (o->mpc_graph) hipGraphExecDestroy(o->mpc_graph);
    // the buffers that grow on demand (grow_device / grow_pinned): a new one is one entry here
    const struct { void* p; bool pinned; } own[] = {
        {o->dl_host, true},    {o->rt_dev, false},     {o->h.rec_log, false},
        {o->h.tl_keys, false}, {o->h.tl_count, false}, {o->h.tl_state, false}};
    for (const auto& b : own) b.pinned ? hipHostFree(b.p) : hipFree(b.p);  // null: no operation
    hipStreamDestroy(o->h.stream);
  }
  delete o;
}

extern "C" int pl_ocp_dims(const pl_ocp* o, int* n, int* m, int* np, int* nnz) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (n) *n = o->h.n;
  if (m) *m = o->h.m;
  if (np) *np = o->h.np;
  if (nnz) *nnz = o->h.nnz;
  return 0;
}

extern "C" int pl_ocp_pattern(const pl_ocp* o, int* rows, int* cols) {
  if (!o || !rows || !cols) { pl_set_error("null argument"); return -1; }
  const int N = o->h.N;
  for (int i = 0; i < N; ++i) {
    const PlNode& nd = o->nodes[i];
    for (int e = 0; e < nd.nent; ++e) {
      const int lc = o->entcol[nd.ent_off + e];
      rows[nd.ent_off + e] = nd.row_off + o->rowidx[nd.ent_off + e];
      cols[nd.ent_off + e] = lc < nd.nw ? nd.x_off + lc : o->nodes[i + 1].x_off + (lc - nd.nw);
    }
  }
  return 0;
}

extern "C" int pl_ocp_set_params(pl_ocp* o, const double* P) {
  REQUIRE_DEVICE(o);
  const size_t len = (size_t)o->h.B * o->h.np;
  memcpy(o->h_params.data(), P, len * sizeof(double));
  PL_CHECK_HIP(hipMemcpyAsync(o->h.d.p, P, len * sizeof(double), hipMemcpyHostToDevice, o->h.stream));
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  return 0;
}

extern "C" int pl_ocp_get_params(pl_ocp* o, double* P) {
  REQUIRE_DEVICE(o);
  PL_CHECK_HIP(hipMemcpyAsync(P, o->h.d.p, (size_t)o->h.B * o->h.np * sizeof(double), hipMemcpyDeviceToHost,
                              o->h.stream));
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  return 0;
}

extern "C" int pl_ocp_set_x(pl_ocp* o, const double* X) {
  REQUIRE_DEVICE(o);
  PL_CHECK_HIP(hipMemcpyAsync(o->h.d.x, X, (size_t)o->h.B * o->h.n * sizeof(double), hipMemcpyHostToDevice,
                              o->h.stream));
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  return 0;
}

extern "C" int pl_ocp_get_x(pl_ocp* o, double* X) {
  REQUIRE_DEVICE(o);
  PL_CHECK_HIP(hipMemcpyAsync(X, o->h.d.x, (size_t)o->h.B * o->h.n * sizeof(double), hipMemcpyDeviceToHost,
                              o->h.stream));
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  return 0;
}

extern "C" int pl_ocp_get_step(pl_ocp* o, double* dx) {
  REQUIRE_DEVICE(o);
  PL_CHECK_HIP(hipMemcpyAsync(dx, o->h.d.step, (size_t)o->h.B * o->h.n * sizeof(double), hipMemcpyDeviceToHost,
                              o->h.stream));
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  return 0;
}

extern "C" int pl_ocp_init_solver(pl_ocp* o) {
  REQUIRE_DEVICE(o);
  launch_hess(&o->h);
  launch_reset_iterates(&o->h);
  launch_reset_info(&o->h);
  if (o->h.ra.rho_b) launch_rho_reset(&o->h, 1);  // every problem back to the handle's rho
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  return 0;
}

int enqueue_solve(pl_ocp* o, bool timed) {
  PlOcpHandle* h = &o->h;
  if (timed) hipEventRecord(o->ev[0], h->stream);
  // sqp_data(x, p): grad_f, J_g, g, lbg, ubg (ocp.py:386)
  launch_eval_values(h, h->d.x);
  launch_eval_jac(h);
  launch_objective(h);
  if (timed) hipEventRecord(o->ev[1], h->stream);
  // osqp.update(q, Ax, l, u): rescale + refactor (ocp.py:391-395)
  launch_qp_setup(h);
  launch_factor(h);
  if (timed) hipEventRecord(o->ev[2], h->stream);
  // osqp.solve() (ocp.py:401)
  launch_reset_info(h);
  if (rho_adapt_on(h)) launch_rho_reset(h, 0);  // the update counts are per solve; rho_b carries over
  if (!h->set.warm_start) launch_reset_iterates(h);
  launch_admm_init(h);
  const int ct = h->set.check_termination > 0 ? h->set.check_termination : h->set.max_iter;
  int it = 0;
  while (it < h->set.max_iter) {
    const int nit = std::min(ct, h->set.max_iter - it);
    it += nit;
    const bool final = it >= h->set.max_iter;
    const bool at_check = (h->set.check_termination > 0 && it % h->set.check_termination == 0);
    launch_admm(h, nit, (at_check || final) ? 1 : 0, it - nit);
    if (at_check || final) launch_check(h, it, final ? 1 : 0);
    if ((at_check || final) && rho_adapt_at(h, it)) {
      // adaptive rho: the problems the exact pass left running re-estimate their rho; those that
      // leave the band are refactored (the host does not know which: the launches are masked on
      // the device and enqueued every time) and get their carried rhs rebuilt with the new rho
      launch_rho_adapt(h, it, final ? 1 : 0);
      if (!final) {
        h->d.ipskip = h->ra.mask;
        launch_factor_core(h);
        h->d.ipskip = nullptr;
        if (h->admm_rc) launch_fred_masked(h, h->ra.mask);
        launch_admm_init_masked(h, h->ra.mask);
      }
    }
  }
  launch_unscale(h);
  if (timed) hipEventRecord(o->ev[3], h->stream);
  // _armijo_line_search (ocp.py:406, 430-480)
  launch_line_search(h);
  if (timed) hipEventRecord(o->ev[4], h->stream);
  return 0;
}

int fetch_stats(pl_ocp* o, pl_stats* stats) {
  if (!stats) return 0;
  std::vector<PlProbInfo> info(o->h.B);
  PL_CHECK_HIP(hipMemcpyAsync(info.data(), o->h.d.info, o->h.B * sizeof(PlProbInfo), hipMemcpyDeviceToHost,
                              o->h.stream));
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  for (int b = 0; b < o->h.B; ++b) {
    pl_stats& s = stats[b];
    memset(&s, 0, sizeof(s));
    s.status = info[b].status;
    s.admm_iters = info[b].iter;
    s.ls_accepted = info[b].ls_accepted;
    s.ls_branch = info[b].ls_branch;
    s.ls_trials = info[b].ls_trials;
    s.ls_alpha = info[b].ls_alpha;
    s.viol_max = info[b].viol_max;
    s.pri_res = info[b].pri_res;
    s.dua_res = info[b].dua_res;
    s.f = info[b].f;
  }
  return 0;
}

// SQP iterations per solve.  The reference runs one (`for _ in range(1)` with a TODO,
// optimization/ocp.py:382-383); k > 1 repeats eval -> osqp.update -> warm-started
// osqp.solve -> line search from the accepted point.  Phase times are those of the
// last iteration.
extern "C" int pl_ocp_set_admm_kernel(pl_ocp* o, int kind) {
  REQUIRE_DEVICE(o);
  if (kind < PL_ADMM_AUTO || kind > PL_ADMM_CHAIN) { pl_set_error("ADMM kernel %d unknown", kind); return -1; }
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  return admm_select(o, kind);
}

extern "C" int pl_ocp_get_admm_kernel(const pl_ocp* o) {
  if (!o) { pl_set_error("null handle"); return -1; }
  return o->h.admm_rc ? PL_ADMM_CHAIN : (o->h.admm_waves == 2 ? PL_ADMM_SWEEP2 : PL_ADMM_SWEEP);
}

// How k_admm (the "sweep" kernel) reads the small operands of a step: PL_ADMM_OPERANDS_FUSED
// (default: unconsumed prefetches skipped, rho from the bounds where k_qp_finish wrote it) or
// PL_ADMM_OPERANDS_SPLIT (the earlier path, the regression reference).  Bit-identical results; the other ADMM kernels ignore it.
extern "C" int pl_ocp_set_admm_operands(pl_ocp* o, int mode) {
  REQUIRE_DEVICE(o);
  if (mode != PL_ADMM_OPERANDS_SPLIT && mode != PL_ADMM_OPERANDS_FUSED) {
    pl_set_error("ADMM operand mode %d unknown", mode);
    return -1;
  }
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  o->h.admm_operands = mode;  // inside the MPC-graph key: the next pl_mpc_step captures again
  return 0;
}

extern "C" int pl_ocp_get_admm_operands(const pl_ocp* o) {
  if (!o) { pl_set_error("null handle"); return -1; }
  return o->h.admm_operands;
}

// 1 when a fused sweep launched now would compute rho from the bounds (d.rho was last written
// by k_qp_finish), 0 when it would stream d.rho (the interior point's weights) or the mode is
// PL_ADMM_OPERANDS_SPLIT.
extern "C" int pl_ocp_get_admm_rho_from_bounds(const pl_ocp* o) {
  if (!o) { pl_set_error("null handle"); return -1; }
  return o->h.admm_operands == PL_ADMM_OPERANDS_FUSED && o->h.admm_rho_rule && !rho_adapt_on(&o->h) ? 1 : 0;
}

// OSQP adaptive rho (rho_adapt.h, k_rho.hip).  The settings are stored on any handle; a device
// handle allocates the per-problem state on the first enabling call, and every call puts every
// problem's rho back to the handle's.  With PL_SOLVER_IP they have no effect (the interior point
// writes its own row weights).
extern "C" int pl_ocp_set_adaptive_rho(pl_ocp* o, int enable, int interval, double tolerance) {
  if (!o) { pl_set_error("null handle"); return -1; }
  PlOcpHandle* h = &o->h;
  if (enable != 0 && enable != 1) { pl_set_error("adaptive_rho %d: must be 0 or 1", enable); return -1; }
  const int ct = h->set.check_termination;
  if (interval < 0 || (interval > 0 && (ct <= 0 || interval % ct != 0))) {
    pl_set_error("adaptive_rho_interval %d: must be 0 (= check_termination) or a positive multiple of "
                 "check_termination (%d)", interval, ct);
    return -1;
  }
  if (!(tolerance > 1.0)) { pl_set_error("adaptive_rho_tolerance %g: must be > 1", tolerance); return -1; }
  if (o->on_device) {
    (void)hipSetDevice(h->device);
    (void)hipGetLastError();
    PL_CHECK_HIP(hipStreamSynchronize(h->stream));
    if (enable && !h->ra.rho_b) {
      const size_t B = h->B;
      PlRhoAdapt ra = h->ra;
      if (dalloc(o, &ra.rho_b, B) || dalloc(o, &ra.rho_est, B) || dalloc(o, &ra.nupd, B) ||
          dalloc(o, &ra.upd_it, B * PL_RHO_LOG) || dalloc(o, &ra.sn, B * (size_t)(h->N + 1) * 8) ||
          dalloc(o, &ra.mask, B))
        return -2;
      h->ra = ra;
    }
  }
  h->ra.enable = enable;
  h->ra.interval = interval;
  h->ra.tol = tolerance;
  if (o->on_device && h->ra.rho_b) {
    launch_rho_reset(h, 1);
    PL_CHECK_HIP(hipGetLastError());
    PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int pl_ocp_get_adaptive_rho(const pl_ocp* o, int* enable, int* interval, double* tolerance) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (enable) *enable = o->h.ra.enable;
  if (interval) *interval = o->h.ra.interval;
  if (tolerance) *tolerance = o->h.ra.tol;
  return 0;
}

// Per problem: rho, the last estimate and the updates of the last solve.  Before the option was
// ever enabled every problem holds the handle's rho and has made no update.
extern "C" int pl_ocp_get_rho(pl_ocp* o, double* rho, double* rho_estimate, int* updates) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  const size_t B = h->B;
  if (!h->ra.rho_b) {
    for (size_t b = 0; b < B; ++b) {
      if (rho) rho[b] = h->set.rho;
      if (rho_estimate) rho_estimate[b] = h->set.rho;
      if (updates) updates[b] = 0;
    }
    return 0;
  }
  if (rho) PL_CHECK_HIP(hipMemcpyAsync(rho, h->ra.rho_b, B * 8, hipMemcpyDeviceToHost, h->stream));
  if (rho_estimate) PL_CHECK_HIP(hipMemcpyAsync(rho_estimate, h->ra.rho_est, B * 8, hipMemcpyDeviceToHost, h->stream));
  if (updates) PL_CHECK_HIP(hipMemcpyAsync(updates, h->ra.nupd, B * 4, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// The device's rule on the host (tests): nrm = the seven scaled norms of rho_adapt.h.
extern "C" int pl_osqp_rho_estimate_host(const double nrm[7], double rho, double tol, double* rho_est, int* update) {
  if (!nrm || !rho_est || !update) { pl_set_error("null argument"); return -1; }
  const double est = pl::rho_estimate(nrm, rho);
  *rho_est = est;
  *update = pl::rho_update(est, rho, tol) ? 1 : 0;
  return 0;
}

extern "C" int pl_ocp_get_admm_groups(const pl_ocp* o) {
  if (!o) { pl_set_error("null handle"); return -1; }
  return o->h.admm_rc ? rc_groups(&o->h) : 1;
}

extern "C" int pl_ocp_set_sqp_iters(pl_ocp* o, int sqp_iters) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (sqp_iters < 1 || sqp_iters > 1000) { pl_set_error("sqp_iters %d outside [1, 1000]", sqp_iters); return -1; }
  o->h.sqp_iters = sqp_iters;
  return 0;
}

extern "C" int pl_ocp_solve(pl_ocp* o, pl_stats* stats, double* phase_ms) {
  REQUIRE_DEVICE(o);
  if (o->h.solver == PL_SOLVER_IP) {
    enqueue_ip(&o->h);
    PL_CHECK_HIP(hipGetLastError());
    PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
    if (phase_ms)
      for (int k = 0; k < 4; ++k) phase_ms[k] = 0.0;
    return fetch_stats(o, stats);
  }
  for (int k = 0; k < o->h.sqp_iters; ++k) enqueue_solve(o, phase_ms != nullptr);
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  if (phase_ms) {
    for (int k = 0; k < 4; ++k) {
      float ms = 0.f;
      hipEventElapsedTime(&ms, o->ev[k], o->ev[k + 1]);
      phase_ms[k] = ms;
    }
  }
  return fetch_stats(o, stats);
}

extern "C" int pl_eval_sqp_data(pl_ocp* o, double* grad, double* Jvals, double* g, double* lbg, double* ubg) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  launch_eval_values(h, h->d.x);
  launch_eval_jac(h);
  launch_objective(h);
  PL_CHECK_HIP(hipGetLastError());
  const size_t B = h->B;
  if (grad) PL_CHECK_HIP(hipMemcpyAsync(grad, h->d.grad, B * h->n * 8, hipMemcpyDeviceToHost, h->stream));
  if (Jvals) PL_CHECK_HIP(hipMemcpyAsync(Jvals, h->d.Araw, B * h->nnz * 8, hipMemcpyDeviceToHost, h->stream));
  if (g) PL_CHECK_HIP(hipMemcpyAsync(g, h->d.g, B * h->m * 8, hipMemcpyDeviceToHost, h->stream));
  if (lbg) PL_CHECK_HIP(hipMemcpyAsync(lbg, h->d.lbg, B * h->m * 8, hipMemcpyDeviceToHost, h->stream));
  if (ubg) PL_CHECK_HIP(hipMemcpyAsync(ubg, h->d.ubg, B * h->m * 8, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pl_eval_f(pl_ocp* o, double* f) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  launch_objective(h);
  std::vector<double> w((size_t)h->B * 8);
  PL_CHECK_HIP(hipMemcpyAsync(w.data(), h->d.work, w.size() * 8, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  for (int b = 0; b < h->B; ++b) f[b] = w[(size_t)b * 8];
  return 0;
}

// ---------------------------------------------------------------------------
// Batched retract of the solved horizon (k_retract.hip, retract.h): what the reference's
// retract_stacked_sol / compile_solution return per problem (ocp_whole_body_rnea.py:293-366)
// plus the base rows of the equations of motion (run_mpc.py:211-233), for the whole batch.
static int retract_args(const pl_ocp* o, int steps, int terminal) {
  if (!o) { pl_set_error("null handle"); return -1; }
  const int N = o->h.N;
  if (steps < 1 || steps > N) { pl_set_error("retract: steps %d outside [1, %d]", steps, N); return -1; }
  if (terminal != 0 && terminal != 1) { pl_set_error("retract: terminal must be 0 or 1, got %d", terminal); return -1; }
  if (terminal && steps != N) { pl_set_error("retract: the terminal row needs steps == N (%d), got %d", N, steps); return -1; }
  if (PL_IS_CV(o->h.oc.dyn) && N < 2) { pl_set_error("retract: centroidal_vel needs N >= 2"); return -1; }
  return 0;
}

extern "C" int pl_ocp_retract_sizes(const pl_ocp* o, int steps, int terminal, long long* out) {
  if (retract_args(o, steps, terminal)) return -1;
  if (!out) { pl_set_error("null argument"); return -1; }
  const pl::RetractLayout L = pl::retract_layout(o->h.oc, o->h.B, steps, terminal);
  for (int k = 0; k < PL_RETRACT_FIELDS; ++k) {
    out[3 * k] = L.width[k];
    out[3 * k + 1] = L.rows[k];
    out[3 * k + 2] = L.off[k];
  }
  out[3 * PL_RETRACT_FIELDS] = L.total;
  return 0;
}

// the packed result into the handle's device buffer (grown on demand), on the handle's stream
static int retract_enqueue(pl_ocp* o, int steps, int terminal, const pl::RetractLayout& L) {
  if (grow_device(&o->rt_dev, &o->rt_cap, (size_t)L.total, o->h.stream, "pl_ocp_retract")) return -2;
  launch_retract(&o->h, steps, terminal, o->rt_dev);
  PL_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int pl_ocp_retract_device(pl_ocp* o, int steps, int terminal, void* device_dst) {
  if (retract_args(o, steps, terminal)) return -1;
  REQUIRE_DEVICE(o);
  if (!device_dst) { pl_set_error("null argument"); return -1; }
  launch_retract(&o->h, steps, terminal, (double*)device_dst);
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  return 0;
}

extern "C" int pl_ocp_retract(pl_ocp* o, int steps, int terminal, double* q, double* v, double* a, double* forces,
                              double* tau, double* eom_base) {
  if (retract_args(o, steps, terminal)) return -1;
  REQUIRE_DEVICE(o);
  const pl::RetractLayout L = pl::retract_layout(o->h.oc, o->h.B, steps, terminal);
  if (retract_enqueue(o, steps, terminal, L)) return -2;
  if (stage_reserve(o, (size_t)L.total * sizeof(double), "pl_ocp_retract")) return -2;
  // only the wanted fields cross the bus (each is one contiguous range of the packed buffer)
  double* dst[PL_RETRACT_FIELDS] = {q, v, a, forces, tau, eom_base};
  double* stage = (double*)o->dl_host;
  for (int k = 0; k < PL_RETRACT_FIELDS; ++k) {
    const size_t len = (size_t)o->h.B * L.rows[k] * L.width[k];
    if (dst[k] && len)
      PL_CHECK_HIP(hipMemcpyAsync(stage + L.off[k], o->rt_dev + L.off[k], len * 8, hipMemcpyDeviceToHost, o->h.stream));
  }
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  for (int k = 0; k < PL_RETRACT_FIELDS; ++k) {
    const size_t len = (size_t)o->h.B * L.rows[k] * L.width[k];
    if (dst[k] && len) memcpy(dst[k], stage + L.off[k], len * 8);
  }
  return 0;
}

// Host entry points of the Lie-group state maps (DynamicsWholeBodyTorque.state_integrate /
// state_difference, dynamics_whole_body_torque.py:11-40), same code as the kernels.
extern "C" int pl_state_integrate(const pl_model* model, const double* x, const double* dx, double* out) {
  if (!model || !x || !dx || !out) { pl_set_error("null argument"); return -1; }
  const PlModel& M = model->m;
  pl::VecIn<double> acc{dx, nullptr, 0.0, -1};
  double q[PL_MAXQ];
  pl::integrate_q<double>(M, x, acc, q);
  for (int k = 0; k < M.nq; ++k) out[k] = q[k];
  for (int k = 0; k < M.nv; ++k) out[M.nq + k] = x[M.nq + k] + dx[M.nv + k];
  return 0;
}

extern "C" int pl_state_difference(const pl_model* model, const double* x0, const double* x1, double* dx) {
  if (!model || !x0 || !x1 || !dx) { pl_set_error("null argument"); return -1; }
  const PlModel& M = model->m;
  pl::difference_q(M, x0, x1, dx);
  for (int k = 0; k < M.nv; ++k) dx[M.nv + k] = x1[M.nq + k] - x0[M.nq + k];
  return 0;
}
