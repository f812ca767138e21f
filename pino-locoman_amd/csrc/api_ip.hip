// C-ABI, interior-point branch (include/pinoloco.h): the host-side structural probes of the
// Lagrangian Hessian and the Jacobian, solver selection with the Hessian work lists, the
// settings, the multiplier warm start, the statistics and the stage hooks of the tests.
#include "api_internal.h"

#include <map>

// Solver selection (ocp.py:248 / :265 dispatch on the solver string).  The interior
// point's per-problem state (slacks and multipliers, 7 x m doubles per problem) is
// allocated on first selection.
// ---- structurally non-zero pairs of the Lagrangian Hessian blocks (k_lag_hess work list)
// Probed once on the host with the same hyper-dual row code (rows.h) at a generic point:
// random x, parameters and multipliers, contact c = 0.5 so that stance and swing rows are
// both active.  A column pair whose contracted second derivative is exactly 0 there is
// identically 0 (RNEA is linear in a and f, the velocity rows in v, the integration rows in
// everything, the base position never enters): about half of the pairs of a whole-body node.
namespace {
struct HostHessEmit {
  const double* lam;
  double acc;
  int r;
  void operator()(const HDual& v, double, double) {
    acc += lam[r] * v.c;
    ++r;
  }
};

template <int DYN>
void probe_hess(const PlModel& M, const PlOcpConst& O, int i, const double* p, const double* xw, int nw,
                const double* lam, std::vector<uint8_t>& nz) {
  std::vector<HDual> kst(PL_KIN_STORE);
  const int ndx = O.ndx;
  nz.assign((size_t)nw * (nw + 1) / 2, 0);
  for (int k = 0; k < nw; ++k)
    for (int j = 0; j <= k; ++j) {
      pl::VecIn<HDual> dx{xw, nullptr, 0.0, j, k};
      pl::VecIn<HDual> u{xw + ndx, nullptr, 0.0, j - ndx, k - ndx};
      pl::VecIn<HDual> dxn{xw + nw, nullptr, 0.0, j - nw, k - nw};
      HostHessEmit e{lam, 0.0, 0};
      pl::node_rows<HDual, DYN>(M, O, i, p, dx, u, dxn, e, kst.data(), 1);
      nz[(size_t)k * (k + 1) / 2 + j] = e.acc != 0.0;
    }
}

// A generic point of node i for the structural probes: random parameters in (0.5, 1.5)
// with sane step sizes and gait counts, contact 0.5 and swing 0.3 (stance and swing rows both
// active), a unit x_init quaternion, w_i and dx_{i+1} in (-0.1, 0.1); lam (if given) of both
// signs.
void generic_point(const PlOcpHandle& h, const std::vector<PlNode>& nodes, int i, std::vector<double>& p,
                   std::vector<double>& xw, std::vector<double>* lam, uint64_t salt = 0) {
  const PlOcpConst& O = h.oc;
  uint64_t st = 0x9e3779b97f4a7c15ull ^ (uint64_t)(i + 1) ^ (salt << 32);
  auto rnd = [&]() {  // uniform in (0.5, 1.5)
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    return 0.5 + (double)(st >> 11) / 9007199254740992.0;
  };
  p.assign(O.P.np, 0.0);
  for (double& v : p) v = rnd();
  p[O.P.dt_min] = 0.02;
  p[O.P.dt_max] = 0.05;
  for (int k = 0; k < 4 * O.N; ++k) {
    p[O.P.contact + k] = 0.5;
    p[O.P.swing + k] = 0.3;
  }
  p[O.P.n_contacts] = 2.0;
  p[O.P.swing_period] = 0.4;
  p[O.P.swing_vel_limits + 1] = -0.2;
  const int qo = PL_IS_CV(O.dyn) ? 9 : 3;  // quaternion of x_init
  double qn = 0.0;
  for (int k = 0; k < 4; ++k) qn += p[O.P.x_init + qo + k] * p[O.P.x_init + qo + k];
  for (int k = 0; k < 4; ++k) p[O.P.x_init + qo + k] /= sqrt(qn);
  xw.assign(nodes[i].nw + O.ndx, 0.0);
  for (double& v : xw) v = 0.2 * (rnd() - 1.0);
  if (lam) {
    lam->assign(nodes[i].nrow, 0.0);
    for (size_t r = 0; r < lam->size(); ++r) (*lam)[r] = (r & 1) ? rnd() : -rnd();
  }
}

void hess_pattern(const PlOcpHandle& h, const std::vector<PlNode>& nodes, int i, std::vector<uint8_t>& nz) {
  const PlOcpConst& O = h.oc;
  std::vector<double> p, xw, lam;
  generic_point(h, nodes, i, p, xw, &lam);
  const int nw = nodes[i].nw;
  const PlModel& M = h.model;
  switch (O.dyn) {
    case PL_DYN_RNEA: probe_hess<PL_DYN_RNEA>(M, O, i, p.data(), xw.data(), nw, lam.data(), nz); break;
    case PL_DYN_ACC: probe_hess<PL_DYN_ACC>(M, O, i, p.data(), xw.data(), nw, lam.data(), nz); break;
    case PL_DYN_CV: probe_hess<PL_DYN_CV>(M, O, i, p.data(), xw.data(), nw, lam.data(), nz); break;
    case PL_DYN_CA: probe_hess<PL_DYN_CA>(M, O, i, p.data(), xw.data(), nw, lam.data(), nz); break;
    case PL_DYN_ACCNB: probe_hess<PL_DYN_ACCNB>(M, O, i, p.data(), xw.data(), nw, lam.data(), nz); break;
    case PL_DYN_CVNB: probe_hess<PL_DYN_CVNB>(M, O, i, p.data(), xw.data(), nw, lam.data(), nz); break;
    default: probe_hess<PL_DYN_ABA>(M, O, i, p.data(), xw.data(), nw, lam.data(), nz); break;
  }
}
struct HostJacEmit {
  uint8_t* nz;  // [nrow] of one column
  int r;
  void operator()(const Dual& v, double, double) {
    nz[r] = v.d != 0.0;
    ++r;
  }
};

template <int DYN>
void probe_jac(const PlModel& M, const PlOcpConst& O, int i, const double* p, const double* xw, int nw, int nrow,
               std::vector<uint8_t>& nz) {
  std::vector<Dual> kst(PL_KIN_STORE);
  std::vector<double> aba_sh(PL_ABA_SH);
  if (DYN == PL_DYN_ABA) pl::aba_primal(M, O, p, xw, aba_sh.data());  // the implicit-function ABA's primal
  const int ndx = O.ndx, ncol = nw + ndx;
  nz.assign((size_t)ncol * nrow, 0);
  for (int c = 0; c < ncol; ++c) {
    pl::VecIn<Dual> dx{xw, nullptr, 0.0, c};
    pl::VecIn<Dual> u{xw + ndx, nullptr, 0.0, c - ndx};
    pl::VecIn<Dual> dxn{xw + nw, nullptr, 0.0, c - nw};
    HostJacEmit e{nz.data() + (size_t)c * nrow, 0};
    pl::node_rows<Dual, DYN>(M, O, i, p, dx, u, dxn, e, kst.data(), 1, nullptr, aba_sh.data());
  }
}
}  // namespace

// Numerically non-zero Jacobian entries of node i at a generic point (column-major
// [ncol][nrow] flags over the node's local columns w_i, dx_{i+1}): the structural-dependency
// pattern CasADi's symbolic jacobian(g, x) would report, a subset of the library's
// kinematic-dependency pattern (api_build.hip::node_row_deps).  One forward-mode dual pass
// per column on the host, with the device's row code.
static void jac_probe(const PlOcpHandle& h, const std::vector<PlNode>& nodes, int i, uint64_t salt,
                      std::vector<uint8_t>& nz) {
  const PlOcpConst& O = h.oc;
  std::vector<double> p, xw;
  generic_point(h, nodes, i, p, xw, nullptr, salt);
  const int nw = nodes[i].nw, nrow = nodes[i].nrow;
  const PlModel& M = h.model;
  switch (O.dyn) {
    case PL_DYN_RNEA: probe_jac<PL_DYN_RNEA>(M, O, i, p.data(), xw.data(), nw, nrow, nz); break;
    case PL_DYN_RNEAFD: probe_jac<PL_DYN_RNEAFD>(M, O, i, p.data(), xw.data(), nw, nrow, nz); break;
    case PL_DYN_ACC: probe_jac<PL_DYN_ACC>(M, O, i, p.data(), xw.data(), nw, nrow, nz); break;
    case PL_DYN_CV: probe_jac<PL_DYN_CV>(M, O, i, p.data(), xw.data(), nw, nrow, nz); break;
    case PL_DYN_CA: probe_jac<PL_DYN_CA>(M, O, i, p.data(), xw.data(), nw, nrow, nz); break;
    case PL_DYN_ACCNB: probe_jac<PL_DYN_ACCNB>(M, O, i, p.data(), xw.data(), nw, nrow, nz); break;
    case PL_DYN_CVNB: probe_jac<PL_DYN_CVNB>(M, O, i, p.data(), xw.data(), nw, nrow, nz); break;
    default: probe_jac<PL_DYN_ABA>(M, O, i, p.data(), xw.data(), nw, nrow, nz); break;
  }
}

// The union over two independent generic points (an entry that vanishes at one random point
// by accident does not vanish at both).
void jac_pattern(const PlOcpHandle& h, const std::vector<PlNode>& nodes, int i, std::vector<uint8_t>& nz) {
  std::vector<uint8_t> nz2;
  jac_probe(h, nodes, i, 0, nz);
  jac_probe(h, nodes, i, 1, nz2);
  for (size_t k = 0; k < nz.size(); ++k) nz[k] |= nz2[k];
}

extern "C" int pl_ocp_set_solver(pl_ocp* o, int solver) {
  REQUIRE_DEVICE(o);
  if (solver != PL_SOLVER_OSQP && solver != PL_SOLVER_IP) {
    pl_set_error("Solver %d not supported (PL_SOLVER_OSQP = 0, PL_SOLVER_IP = 1)", solver);
    return -1;
  }
  PlOcpHandle* h = &o->h;
  if (solver == PL_SOLVER_IP && h->oc.dyn == PL_DYN_RNEAFD) {
    // the reference keeps the accelerations in u for its Fatrop branch ("necessary for Fatrop
    // solver", ocp_whole_body_rnea.py:21); the Lagrangian Hessian here is block diagonal over w_i
    pl_set_error("the interior-point solver needs include_acc=True (ocp_whole_body_rnea.py:21)");
    return -1;
  }
  if (solver == PL_SOLVER_IP && !h->d.ipinfo) {
    const size_t Bm = (size_t)h->B * h->m;
    if (dalloc(o, &h->d.ip_s, Bm) || dalloc(o, &h->d.ip_lam, Bm) || dalloc(o, &h->d.ip_lam0, Bm) ||
        dalloc(o, &h->d.ip_zl, Bm) ||
        dalloc(o, &h->d.ip_zu, Bm) || dalloc(o, &h->d.ip_rh, Bm) || dalloc(o, &h->d.ip_dl, Bm) ||
        dalloc(o, &h->d.ip_ds, Bm) || dalloc(o, &h->d.ip_jdx, Bm) || dalloc(o, &h->d.ip_dx, (size_t)h->B * h->n) ||
        dalloc(o, &h->d.ipinfo, (size_t)h->B) || dalloc(o, &h->d.ip_dwi, (size_t)2 * h->B) ||
        dalloc(o, &h->d.ip_iflag, (size_t)4 * h->B) || dalloc(o, &h->d.ip_act, (size_t)h->B + 2))
      return -2;
    // Lagrangian Hessian work list (k_hess.hip): the structurally non-zero column pairs
    // j <= k of every w_i block (hess_pattern, one probe per node type); node blocks packed
    // lower, the pairs not listed stay 0
    std::vector<int2> hl, hlin, hvv, htr, hcone, htrf;
    std::vector<int> hoff;
    long long off = 0;
    const PlOcpConst& O = h->oc;
    std::vector<uint8_t> pat[3];
    // whole_body_rnea / whole_body_acc: the rows are linear in a and in the contact forces, and only the RNEA rows
    // couple them to q, so the (dq, a) and (dq, f_feet) blocks are d/dq of M(q) lambda_tau and
    // of -J_e(q) lambda_tau (k_lag_hess_lin: two dual tree passes per dq column instead of one
    // hyper-dual pass per pair); PL_PATH_HESS_DUAL_ALL keeps them as pairs
    const bool lin = (O.dyn == PL_DYN_RNEA || O.dyn == PL_DYN_ACC) &&
                     !(h->debug_paths & PL_PATH_HESS_DUAL_ALL);
    const int lin_lo = O.ndx, lin_hi = O.ndx + O.na + 3 * O.nfeet;
    // rnea family and whole_body_acc: the chain of a w_i coordinate (-1: the base, or none).  The rows are sums of
    // per-chain terms that read the base and their own chain only, so a pair with a coordinate
    // of chain c has a mixed part from chain c's terms alone, and its pass skips the other
    // chains (tree_pass only_ch, packed as .x = node | (chain + 1) << 16).  PL_PATH_HESS_FULL_TREE: off
    const bool chains = (PL_IS_RNEA(O.dyn) || O.dyn == PL_DYN_ACC) &&
                        !(h->debug_paths & PL_PATH_HESS_FULL_TREE);
    const PlModel& Mo = h->model;
    const auto joint_chain = [&](int jt) {
      for (int c = 0; c < Mo.nchains; ++c)
        if (jt >= Mo.chain_first[c] && jt < Mo.chain_first[c] + Mo.chain_len[c]) return c;
      return -1;
    };
    const auto vidx_chain = [&](int vi) {
      if (vi < 6) return -1;
      for (int jt = 2; jt < Mo.njoints; ++jt)
        if (Mo.idx_v[jt] == vi) return joint_chain(jt);
      return -1;
    };
    const auto coord_chain = [&](int c) {
      if (c < O.ndx) return vidx_chain(c < O.nv ? c : c - O.nv);
      const int k = c - O.ndx;
      if (k < O.na) return vidx_chain(k);
      if (k < O.na + O.nf) {
        const int e = (k - O.na) / 3;
        return joint_chain(e < O.nfeet ? O.feet[e].joint : O.ext.joint);
      }
      return vidx_chain(6 + k - O.na - O.nf);
    };
    const auto pair_chain = [&](int j, int k) {
      if (!chains) return -1;
      const int cj = coord_chain(j), ck = coord_chain(k);
      if (cj < 0) return ck;
      if (ck < 0 || ck == cj) return cj;
      return -1;  // two chains: structurally zero, kept on the full pass
    };
    for (int i = 0; i <= h->N; ++i) {
      const int nw = o->nodes[i].nw;
      hoff.push_back((int)off);
      off += (long long)nw * (nw + 1) / 2;
      if (i == h->N) break;  // no rows on the last node
      const int type = pl::node_type(O, i);
      if (pat[type].empty()) hess_pattern(*h, o->nodes, i, pat[type]);
      for (int k = 0; k < nw; ++k)
        for (int j = 0; j <= k; ++j) {
          if (lin && j < O.nv && k >= lin_lo && k < lin_hi) continue;
          if (!pat[type][(size_t)k * (k + 1) / 2 + j]) continue;
          // two state columns: the curvature of the tree-pass rows alone (k_lag_hess_tree), and for
          // (dv, dv) the quadratic form of the RNEA bias term (k_lag_hess_vv)
          const int ff = O.ndx + O.na;  // the foot forces
          if (lin && j == k && j >= ff && j < ff + 3 * O.nfeet) {  // the friction cones (k_lag_hess_cone)
            hcone.push_back(make_int2(i, j));
            continue;
          }
          if (lin && j >= 3 && j < O.nv && k >= ff + 3 * O.nfeet && k < ff + 3 * O.nee) {  // (dq, f_ext)
            htrf.push_back(make_int2(i | ((pair_chain(j, k) + 1) << 16), j | (k << 16)));
            continue;
          }
          const bool st = lin && k < O.ndx;
          (st ? (j >= O.nv ? hvv : htr) : hl).push_back(make_int2(i | ((pair_chain(j, k) + 1) << 16), j | (k << 16)));
        }
      if (lin)  // RNEA ignores the base position
        for (int k = 3; k < O.nv; ++k) hlin.push_back(make_int2(i, k | ((chains ? vidx_chain(k) + 1 : 0) << 16)));
    }
    for (int t = 0; t < 3; ++t) {  // first row of the RNEA base / joint-torque row blocks per node type
      h->hl_rb_base[t] = h->hl_rb_tau[t] = -1;
      int r = 0;
      for (int bi = 0; bi < O.nblk[t]; ++bi) {
        if (O.blk[t][bi].kind == PL_RB_RNEA_BASE) h->hl_rb_base[t] = r;
        if (O.blk[t][bi].kind == PL_RB_TAU_EQ) h->hl_rb_tau[t] = r;
        r += O.blk[t][bi].count;
      }
    }
    // the written entries of a node block per node type (k_ip_refine's H_i dx): the pattern and,
    // with the linear-column identity, the whole (dq_k, a | f_feet) rows k_lag_hess_lin stores
    std::vector<int> hnz;
    for (int t = 0; t < 3; ++t) {
      h->hnz_off[t] = (int)hnz.size();
      int nw = -1;
      for (int i = 0; i < h->N; ++i)
        if (pl::node_type(O, i) == t) { nw = o->nodes[i].nw; break; }
      if (nw < 0 || pat[t].empty()) continue;
      for (int k = 0; k < nw; ++k)
        for (int j = 0; j <= k; ++j)
          if (pat[t][(size_t)k * (k + 1) / 2 + j] || (lin && j >= 3 && j < O.nv && k >= lin_lo && k < lin_hi))
            hnz.push_back(k | (j << 16));
    }
    h->hnz_off[3] = (int)hnz.size();
    if (!hnz.empty() && upload(o, &h->d.hnz, hnz)) return -2;
    // the (dq, dq) / (dq, dv) pairs as forward-over-reverse columns (k_lag_hess_col, r06): the pair
    // (j, k), j <= k, is written by the item (node, chain, j) with k's local coordinate in its mask
    // (hess_tree.h col_coord).  The column sweep assumes no frame on the root and at most one frame
    // (a foot or the external force) per chain; otherwise, without chain confinement, or with
    // PL_PATH_HESS_PAIRS the pair kernel runs.
    std::vector<int4> hcol;
    {
      bool ok = chains && !htr.empty() && !(h->debug_paths & PL_PATH_HESS_PAIRS);
      for (int e = 0; e < O.nee && ok; ++e)
        if ((e < O.nfeet ? O.feet[e].joint : O.ext.joint) == 1) ok = false;
      for (int c = 0; c < Mo.nchains && ok; ++c) {
        int nfr = 0;
        for (int e = 0; e < O.nee; ++e) {
          const int fj = e < O.nfeet ? O.feet[e].joint : O.ext.joint;
          if (fj >= Mo.chain_first[c] && fj < Mo.chain_first[c] + Mo.chain_len[c]) ++nfr;
        }
        if (nfr > 1 || 12 + 2 * Mo.chain_len[c] > 32) ok = false;
      }
      const auto loc_of = [&](int ch, int k) {  // k (a state dx index) in chain ch's local coordinates
        if (k < 6) return k;
        if (k >= O.nv && k < O.nv + 6) return 6 + k - O.nv;
        if (ch < 0) return -1;
        const int first = Mo.chain_first[ch], L = Mo.chain_len[ch];
        for (int kk = 0; kk < L; ++kk) {
          if (Mo.idx_v[first + kk] == k) return 12 + kk;
          if (O.nv + Mo.idx_v[first + kk] == k) return 12 + L + kk;
        }
        return -1;
      };
      std::map<long long, uint32_t> cols;  // (node, chain, j) -> mask, in work-list order
      for (const int2& pr : htr) {
        const int i = pr.x & 0xffff, ch = (pr.x >> 16) - 1, j = pr.y & 0xffff, k = pr.y >> 16;
        const int lk = loc_of(ch, k);
        if (lk < 0) { ok = false; break; }
        cols[((long long)i << 32) | ((long long)(ch + 1) << 16) | j] |= 1u << lk;
      }
      h->hcol_nbase = 0;
      if (ok)
        for (int pass = 0; pass < 2; ++pass)  // the whole-tree base columns first (k_lag_hess_col<true>)
          for (const auto& kv : cols) {
            const int chp = (int)((kv.first >> 16) & 0xffff);
            if ((chp == 0) != (pass == 0)) continue;
            hcol.push_back(make_int4((int)(kv.first >> 32) | (chp << 16), (int)(kv.first & 0xffff), (int)kv.second, 0));
            if (pass == 0) ++h->hcol_nbase;
          }
    }
    h->hcol_len = (int)hcol.size();
    // k_lag_hess_arm's pairs: those on the base or the arm's chain (the others have no arm-row curvature;
    // until r05 their waves ran and exited)
    std::vector<int2> harm;
    {
      int arm_ch = -1;
      for (int c = 0; c < Mo.nchains; ++c)
        if (O.arm.valid && O.arm.joint >= Mo.chain_first[c] && O.arm.joint < Mo.chain_first[c] + Mo.chain_len[c]) arm_ch = c;
      if (arm_ch >= 0)
        for (const int2& pr : htr) {
          const int ch = (pr.x >> 16) - 1;
          if (ch < 0 || ch == arm_ch) harm.push_back(pr);
        }
    }
    h->harm_len = (int)harm.size();
    h->hl_len = (int)hl.size();
    h->hlin_len = (int)hlin.size();
    h->hvv_len = (int)hvv.size();
    h->htr_len = (int)htr.size();
    h->hcone_len = (int)hcone.size();
    h->htrf_len = (int)htrf.size();
    h->hl_stride = (off + 1) & ~1LL;
    if ((!hl.empty() && upload(o, &h->d.hlist, hl)) || upload(o, &h->d.hoff, hoff) ||
        dalloc(o, &h->d.Hlag, (size_t)h->B * h->hl_stride))
      return -2;
    if (lin) {
      PlModel m0 = h->model;
      for (int k = 0; k < 3; ++k) m0.gravity[k] = 0.0;
      if (upload(o, &h->d.hlin, hlin) || (!hvv.empty() && upload(o, &h->d.hvv, hvv)) ||
          (!htr.empty() && upload(o, &h->d.htr, htr)) || (!hcone.empty() && upload(o, &h->d.hcone, hcone)) ||
          (!htrf.empty() && upload(o, &h->d.htrf, htrf)) || (!hcol.empty() && upload(o, &h->d.hcol, hcol)) ||
          (!harm.empty() && upload(o, &h->d.harm, harm)))
        return -2;
      if (!h->d.model0 && (dalloc(o, &h->d.model0, 1) ||
                           hipMemcpy(h->d.model0, &m0, sizeof(PlModel), hipMemcpyHostToDevice) != hipSuccess))
        return -2;
    }
  }
  h->solver = solver;
  return 0;
}

extern "C" int pl_ocp_set_ip_settings(pl_ocp* o, const pl_ip_settings* s) {
  if (!o || !s) { pl_set_error("null argument"); return -1; }
  if (s->max_iter < 0 || s->max_iter > PL_IP_MAXFILT) {
    pl_set_error("ip max_iter %d outside [0, %d]", s->max_iter, PL_IP_MAXFILT);
    return -1;
  }
  if (s->ls_max < 1 || s->ls_max > 60 || !(s->tol > 0) || !(s->mu_init > 0) || !(s->bound_push > 0) ||
      !(s->bound_frac > 0) || !(s->delta_w >= 0) || !(s->delta_c > 0) || s->n_refine < 0 || s->n_refine > 8) {
    pl_set_error("invalid interior-point settings");
    return -1;
  }
  if (s->hessian != PL_IP_HESS_EXACT && s->hessian != PL_IP_HESS_GN) {
    pl_set_error("ip hessian %d unknown (PL_IP_HESS_EXACT = 0, PL_IP_HESS_GN = 1)", s->hessian);
    return -1;
  }
  o->h.ip = PlIpSettings{s->tol, s->mu_init, s->bound_push, s->bound_frac, s->delta_w, s->delta_c, s->max_iter,
                         s->ls_max, s->n_refine, 0, 1e-7};
  o->h.ip_hess = s->hessian;
  return 0;
}

// lam_g warm start of the interior-point branch (opti.set_initial(opti.lam_g, lam_g),
// ocp_whole_body_rnea.py:234-235 and the other OCPs' warm_start): lam = NULL returns to the
// cold start (lam = 0).  Kept until changed, like an Opti initial value.
extern "C" int pl_ocp_set_lam(pl_ocp* o, const double* lam) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (!h->d.ip_lam0) { pl_set_error("no interior-point state (pl_ocp_set_solver(o, PL_SOLVER_IP) first)"); return -1; }
  if (!lam) {
    h->ip_lam_warm = 0;
    return 0;
  }
  PL_CHECK_HIP(hipMemcpyAsync(h->d.ip_lam0, lam, (size_t)h->B * h->m * 8, hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  h->ip_lam_warm = 1;
  return 0;
}

extern "C" int pl_ocp_get_lam(pl_ocp* o, double* lam) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (!h->d.ip_lam) { pl_set_error("no interior-point state (pl_ocp_set_solver(o, PL_SOLVER_IP) first)"); return -1; }
  PL_CHECK_HIP(hipMemcpyAsync(lam, h->d.ip_lam, (size_t)h->B * h->m * 8, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pl_ocp_ip_stats(pl_ocp* o, pl_ip_stats* out) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (!h->d.ipinfo) { pl_set_error("no interior-point state (pl_ocp_set_solver(o, PL_SOLVER_IP) first)"); return -1; }
  std::vector<PlIpInfo> info(h->B);
  PL_CHECK_HIP(hipMemcpyAsync(info.data(), h->d.ipinfo, h->B * sizeof(PlIpInfo), hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  for (int b = 0; b < h->B; ++b) {
    pl_ip_stats& s = out[b];
    memset(&s, 0, sizeof(s));
    s.status = info[b].status;
    s.iter = info[b].iter;
    s.ls_trials = info[b].trials;
    s.nfilter = info[b].nfilt;
    s.err = info[b].err;
    s.mu = info[b].mu;
    s.alpha = info[b].alpha;
    s.alpha_z = info[b].alpha_z;
    s.f = info[b].f;
    s.viol_max = info[b].viol_max;
    for (int q = 0; q < PL_IP_MAXFILT; ++q) s.alphas[q] = info[b].alphas[q];
    s.ref_solves = info[b].ref_solves;
  }
  return 0;
}

extern "C" int pl_debug_ip_direction(pl_ocp* o, const double* S, const double* LAM, const double* ZL,
                                     const double* ZU, const double* MU) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (!h->d.ipinfo) { pl_set_error("no interior-point state (pl_ocp_set_solver(o, PL_SOLVER_IP) first)"); return -1; }
  const size_t Bm = (size_t)h->B * h->m * 8;
  PL_CHECK_HIP(hipMemcpyAsync(h->d.ip_s, S, Bm, hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipMemcpyAsync(h->d.ip_lam, LAM, Bm, hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipMemcpyAsync(h->d.ip_zl, ZL, Bm, hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipMemcpyAsync(h->d.ip_zu, ZU, Bm, hipMemcpyHostToDevice, h->stream));
  std::vector<PlIpInfo> info(h->B);
  for (int b = 0; b < h->B; ++b) {
    memset(&info[b], 0, sizeof(PlIpInfo));
    info[b].mu = MU[b];
    info[b].active = 1;
  }
  PL_CHECK_HIP(hipMemcpyAsync(h->d.ipinfo, info.data(), h->B * sizeof(PlIpInfo), hipMemcpyHostToDevice, h->stream));
  launch_reset_info(h);
  enqueue_ip_direction(h);
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// Tests: one interior-point stage on the device buffers as they are (include/pinoloco.h).
extern "C" int pl_debug_ip_stage(pl_ocp* o, int stage, int arg) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (!h->d.ipinfo) { pl_set_error("no interior-point state (pl_ocp_set_solver(o, PL_SOLVER_IP) first)"); return -1; }
  if (stage == PL_IP_STAGE_KKT && (arg < 0 || arg > h->ip.max_iter)) {
    pl_set_error("ip stage KKT: iteration %d outside [0, max_iter %d]", arg, h->ip.max_iter);
    return -1;
  }
  if (enqueue_ip_stage(h, stage, arg) != 0) { pl_set_error("ip stage %d unknown", stage); return -1; }
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}
