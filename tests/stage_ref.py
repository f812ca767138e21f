"""Stage references for the block factor and the ADMM kernels (shared by test_stage_ref.py,
test_stage_kernels_gpu.py and the tools/gpu_factor_*.py reports; a plain module, no fixtures).

Everything here works on ONE scaled QP, a dict ``qp`` (scaled_qp: read back from a device handle,
oracle_qp: built by the numpy oracle), so evaluation and Ruiz scaling stay outside the comparison:

    K = diag(P + sigma) + A^T diag(rho) A,  block tridiagonal over the node blocks w_i = [dx_i, u_i]

* the long-double reference (x87 extended, eps 1.08e-19): block-tridiagonal elimination with a
  Gauss-Jordan inverse per block (LDFactor: S_i, forward / backward block solve), the per-node
  stages of k_fnode (node_stages: C^-1, G = C^-1 B^T, A' = A - B G) and the OSQP iteration
  (admm_iterate, the loop of oracle/osqp_ref.py:222-236, which stays the authority);
* the fp64 routes through the same admm_iterate: oracle.osqp_ref.BlockReduced (the GPU's
  elimination order in LAPACK arithmetic) and a sparse LU of K;
* the decoders of the device layouts: decode_S (lane-tile S_i) and fs_blocks (A', G, C^-1 in FS).
"""
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for _p in (ROOT, os.path.join(ROOT, "pino-locoman_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the stage reference needs an extended-precision long double (x87)"

# ---------------------------------------------------------------------------- the case table
# (tag, robot, dynamics, constructor keywords, horizons); every case runs B = 3 synthetic problems
# of pinoloco.synthetic.build_batch(R, dyn, N, 3, 0)
CASES = [
    ("cv24", "go2", "centroidal_vel", {}, (2, 3, 4, 7, 8, 9, 16)),   # ndx 24; chain groups 1/1/1/1/2/2/3
    ("cv30", "b2g", "centroidal_vel", {}, (2, 4)),                   # ndx 30, padded tile
    ("rnea36", "go2", "whole_body_rnea", {}, (2, 3, 4, 8, 9)),       # ASR 32 below N = 9, three node types
    ("fd36", "go2", "whole_body_rnea", {"include_acc": False}, (2, 4)),  # general coupling: sweeps only
    ("aba36", "b2", "whole_body_aba", {}, (2, 4)),                   # MFMA E_{i+1}
    ("rnea48", "b2g", "whole_body_rnea", {}, (2, 4)),                # nw 105, nunit 6
    ("acc48", "b2g", "whole_body_acc", {}, (3,)),
    ("accnb", "go2", "whole_body_acc", {"include_base": False}, (3,)),
]
CASE_IDS = [(tag, N) for tag, _, _, _, Ns in CASES for N in Ns]
BATCH = 3
# problems per workgroup of the one-wave sweep: (tag, N, batch, expected admm_ppw)
PPW_CASES = [("cv24", 2, 1027, 4), ("cv24", 2, 515, 2)]


def case(tag):
    for c in CASES:
        if c[0] == tag:
            return c
    raise KeyError(tag)


def make_problem(tag, N, B, first=0):
    """(robot, dynamics, keywords, P, X) of the case's synthetic problems first .. first + B - 1."""
    from pinoloco import robots
    from pinoloco.synthetic import build_batch
    _, rname, dyn, kw, _ = case(tag)
    R = robots.ROBOTS[rname]()
    R.set_gait_sequence("trot", 0.8)
    _, P, X, _, _ = build_batch(R, dyn, N, B, first, **kw)
    return R, dyn, kw, P, X


def make_handle(tag, N, B, device=0, debug_paths=()):
    """A BatchedOCP of the case with parameters, x and the solver set (device < 0: host only)."""
    from pinoloco.ocp import BatchedOCP
    R, dyn, kw, P, X = make_problem(tag, N, B if device >= 0 else 1)
    bo = BatchedOCP(R, dyn, N, batch=B, device=device, debug_paths=debug_paths, **kw)
    if device >= 0:
        bo.set_params(P)
        bo.set_x(X)
        bo.init_solver()
    return bo


# ---------------------------------------------------------------------------- device layouts
def decode_S(Sflat, s_off, nw, ntile, K):
    """Lane-tile layout (state.h) -> dense symmetric nw x nw.  Tile t = I (I + 1) / 2 + J of the
    packed lower 4 x 4 tiles sits in slot t % K of lane t // K; off-diagonal tiles are mirrored,
    diagonal tiles are stored full."""
    T = ntile
    M = np.zeros((4 * T, 4 * T))
    for I in range(T):
        for J in range(I + 1):
            t = I * (I + 1) // 2 + J
            ln, sl = t // K, t % K
            for r in range(4):
                for h in range(2):
                    base = s_off + ((sl * 8 + 2 * r + h) * 64 + ln) * 2
                    M[4 * I + r, 4 * J + 2 * h] = Sflat[base]
                    M[4 * I + r, 4 * J + 2 * h + 1] = Sflat[base + 1]
    full = M.copy()
    for I in range(T):
        for J in range(I):
            full[4 * J:4 * J + 4, 4 * I:4 * I + 4] = M[4 * I:4 * I + 4, 4 * J:4 * J + 4].T
    return full[:nw, :nw]


def fs_offsets(nodes, X):
    """Offsets of every node's [A' (X x X) | G (U x X) | C^-1 (U x U)] in the factor scratch FS
    (32-double aligned, api_build.hip) and the stride per problem."""
    offs, fs = [], 0
    for nd in nodes:
        U = int(nd[1])
        offs.append(fs)
        fs = (fs + X * X + U * X + U * U + 31) & ~31
    return offs, max(fs, 32)


def fs_blocks(FSb, off, X, U):
    """A', G and C^-1 of one node from one problem's FS; C^-1 from its lower triangle, the part
    k_fchain reads."""
    Ap = FSb[off:off + X * X].reshape(X, X)
    G = FSb[off + X * X:off + X * X + U * X].reshape(U, X)
    Cg = FSb[off + X * X + U * X:off + X * X + U * X + U * U].reshape(U, U)
    return Ap, G, np.tril(Cg) + np.tril(Cg, -1).T


def general_coupling(bo):
    """The factor's general-coupling rule (api_build.hip) from the pattern: some node's rows touch
    a dx_{i+1} column more or less than once, or one row touches several of them."""
    rows, cols = bo.pattern()
    nodes, X = bo.node_table(), bo.layout.ndx
    for nd in nodes[:-1]:
        c0 = int(nd[2]) + int(nd[0])
        sel = (rows >= nd[3]) & (rows < nd[3] + nd[4]) & (cols >= c0) & (cols < c0 + X)
        if np.any(np.bincount(cols[sel] - c0, minlength=X) != 1) or np.unique(rows[sel]).size != X:
            return True
    return False


def read_scaled(bo):
    """The device's scaled QP data of the whole batch, one read per array."""
    B, n, m, nnz = bo.batch, bo.n, bo.m, bo.nnz
    out = {k: bo.debug(k, B * ln).reshape(B, ln) for k, ln in
           (("As", nnz), ("Ps", n), ("qs", n), ("ls", m), ("us", m), ("rho", m))}
    out["pattern"] = bo.pattern()
    out["nodes"] = bo.node_table()
    return out


def scaled_qp(bo, b, raw=None):
    """Problem b's scaled QP as the device holds it (after debug_admm / solve)."""
    raw = raw or read_scaled(bo)
    rows, cols = raw["pattern"]
    nodes = raw["nodes"]
    X = bo.layout.ndx
    return _finish_qp(dict(
        A=sp.csr_matrix((raw["As"][b], (rows, cols)), shape=(bo.m, bo.n)), P=raw["Ps"][b].copy(),
        q=raw["qs"][b].copy(), l=raw["ls"][b].copy(), u=raw["us"][b].copy(), rho=raw["rho"][b].copy(),
        sigma=float(bo.settings["sigma"]), alpha=float(bo.settings["alpha"]),
        blocks=[(int(nd[2]), int(nd[0]), X) for nd in nodes]),
        row_ranges=[(int(nd[3]), int(nd[4])) for nd in nodes])


def oracle_qp(tag, N, prob=1):
    """The same dict built by the numpy oracle alone (OracleOCP + OSQPRef._scale) for synthetic
    problem ``prob`` of the case: the CPU tests' data.  Also returns the oracle and (grad, Ax, l, u)."""
    from oracle import osqp_ref as O
    from oracle.ocp import OracleOCP
    R, dyn, kw, P, X = make_problem(tag, N, 1, prob)
    o = OracleOCP(R, dyn, N, **kw)
    x, p = X[0], P[0]
    o.init_solver(x, p)
    _, grad = o.f_and_grad(x, p)
    g, lbg, ubg = o.eval_g(x, p)
    Ax = o.jacobian_values(x, p)
    os_ = o.osqp
    A_raw = sp.csc_matrix((Ax, os_.A_pat.indices, os_.A_pat.indptr), shape=os_.A_pat.shape)
    l = np.maximum(lbg - g, -O.OSQP_INFTY)
    u = np.minimum(ubg - g, O.OSQP_INFTY)
    Ps, qs, A, D, E, c = os_._scale(os_.P_raw, grad, A_raw)
    ls, us = E * l, E * u
    s = os_.s
    rho = np.full(os_.m, s["rho"])
    loose = (ls < -O.OSQP_INFTY * O.MIN_SCALING) & (us > O.OSQP_INFTY * O.MIN_SCALING)
    eq = (~loose) & (us - ls < O.RHO_TOL)
    rho[loose] = O.RHO_MIN
    rho[eq] = O.RHO_EQ_OVER_RHO_INEQ * s["rho"]
    qp = _finish_qp(dict(A=A.tocsr(), P=Ps, q=qs, l=ls, u=us, rho=rho, sigma=s["sigma"], alpha=s["alpha"],
                         blocks=[tuple(int(v) for v in bl) for bl in os_.blocks]))
    return qp, o, (grad, Ax, lbg - g, ubg - g)


def _finish_qp(qp, row_ranges=None):
    """Adds the node structure of A: per node its rows (row_ranges: the device's (row_off, nrow);
    else the rows whose first column lies in w_i) and the column span they touch,
    [x_off_i, x_off_i + nw_i + ce_i) with ce_i columns of the next node (its dx part)."""
    A = qp["A"].tocsr()
    A.sort_indices()
    qp["A"] = A
    m, n = A.shape
    qp["m"], qp["n"] = m, n
    offs = np.array([o for o, _, _ in qp["blocks"]])
    lo = np.full(m, n)
    hi = np.zeros(m, dtype=np.int64)
    coo = A.tocoo()
    np.minimum.at(lo, coo.row, coo.col)
    np.maximum.at(hi, coo.row, coo.col)
    lo[lo == n] = 0  # a row without entries belongs nowhere and adds nothing
    rnode = np.searchsorted(offs, lo, side="right") - 1
    if row_ranges is not None:
        own = np.full(m, -1)
        for i, (ro, nr) in enumerate(row_ranges):
            own[ro:ro + nr] = i
        assert np.all(own >= 0) and np.all(rnode >= own), "a row reaches behind its node"
        rnode = own
    rows, span = [], []
    for i, (o, w, X) in enumerate(qp["blocks"]):
        r = np.flatnonzero(rnode == i)
        end = int(hi[r].max()) + 1 if r.size else o + w
        ce = max(end - (o + w), 0)
        if ce:
            assert i + 1 < len(qp["blocks"]) and ce <= qp["blocks"][i + 1][1], "A is not block bidiagonal"
        rows.append(r)
        span.append(ce)
    qp["rows"], qp["span"] = rows, span
    return qp


# ---------------------------------------------------------------------------- arithmetic
def gj_inv(M, dt=LD):
    """Inverse by symmetric Gauss-Jordan sweeps in ``dt`` (no pivoting: the blocks are SPD)."""
    M = np.array(M, dtype=dt)
    for k in range(M.shape[0]):
        p = M[k, k]
        r, c = M[k, :].copy(), M[:, k].copy()
        M -= np.outer(c, r) / p
        M[k, :], M[:, k] = r / p, c / p
        M[k, k] = -1 / p
    return -M


def rel(a, ref):
    """max |a - ref| / max |ref|, formed in long double."""
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), LD(1e-300)))


class NodeBlocks:
    """A and K of one QP as dense per-node blocks in ``dt``: A_i (the node's rows over their
    column span), Kt_ii (own rows: what k_fnode assembles), K_ii and the coupling C_i = K_{i,i-1}
    restricted to its non-zero rows (the first ce_{i-1} of w_i)."""

    def __init__(self, qp, dt=LD):
        self.qp, self.dt = qp, dt
        A = qp["A"]
        bl = qp["blocks"]
        P, rho, sig = np.asarray(qp["P"], dt), np.asarray(qp["rho"], dt), dt(qp["sigma"])
        self.Ai, self.Kt, self.Kd, self.C = [], [], [], [None]
        carry = None
        for i, (o, w, _) in enumerate(bl):
            r, ce = qp["rows"][i], qp["span"][i]
            Ai = np.asarray(A[r, o:o + w + ce].toarray(), dt)
            self.Ai.append(Ai)
            Ki = (Ai.T * rho[r]) @ Ai
            Kt = Ki[:w, :w] + np.diag(P[o:o + w] + sig)
            self.Kt.append(Kt)
            Kd = Kt.copy()
            if carry is not None:
                c = carry.shape[0]
                Kd[:c, :c] += carry
            self.Kd.append(Kd)
            if i + 1 < len(bl):
                self.C.append(Ki[w:, :w])
            carry = Ki[w:, w:] if ce else None

    def mul(self, x):
        """A x"""
        z = np.zeros(self.qp["m"], self.dt)
        for (o, w, _), r, ce, Ai in zip(self.qp["blocks"], self.qp["rows"], self.qp["span"], self.Ai):
            z[r] = Ai @ x[o:o + w + ce]
        return z

    def tmul(self, v):
        """A^T v"""
        x = np.zeros(self.qp["n"], self.dt)
        for (o, w, _), r, ce, Ai in zip(self.qp["blocks"], self.qp["rows"], self.qp["span"], self.Ai):
            x[o:o + w + ce] += Ai.T @ v[r]
        return x


class LDFactor:
    """Block-tridiagonal elimination in ``dt``: S_i = (K_ii - C_i S_{i-1} C_i^T)^-1 by Gauss-Jordan,
    and the forward / backward block solve."""

    def __init__(self, nb):
        self.nb = nb
        self.S = []
        for i in range(len(nb.Kd)):
            M = nb.Kd[i].copy()
            if i > 0:
                C = nb.C[i]
                c = C.shape[0]
                M[:c, :c] -= C @ self.S[-1] @ C.T
            S = gj_inv(M, nb.dt)
            self.S.append((S + S.T) / 2)

    def solve(self, r):
        nb, bl = self.nb, self.nb.qp["blocks"]
        r = np.asarray(r, nb.dt)
        bt, wv = [], []
        for i, (o, w, _) in enumerate(bl):
            b = r[o:o + w].copy()
            if i > 0:
                C = nb.C[i]
                b[:C.shape[0]] -= C @ wv[-1]
            bt.append(b)
            wv.append(self.S[i] @ b)
        x = np.zeros_like(r)
        xn = None
        for i in range(len(bl) - 1, -1, -1):
            o, w, _ = bl[i]
            if xn is None:
                xi = wv[i]
            else:
                C = nb.C[i + 1]
                xi = self.S[i] @ (bt[i] - C.T @ xn[:C.shape[0]])
            x[o:o + w] = xi
            xn = xi
        return x


def node_stages(nb, i, lapack=False):
    """(A', G, C^-1) of node i from Kt_ii = [[A, B], [B^T, C]] in the blocks' precision; lapack:
    the fp64 route's formulas (oracle.osqp_ref.BlockReduced: LAPACK inverse, symmetrised)."""
    _, w, X = nb.qp["blocks"][i]
    Kt = nb.Kt[i]
    Am, Bm, Cm = Kt[:X, :X], Kt[:X, X:], Kt[X:, X:]
    if lapack:
        Ci = np.linalg.inv(Cm)
        Ci = 0.5 * (Ci + Ci.T)
    else:
        Ci = gj_inv(Cm, nb.dt)
    G = Ci @ Bm.T
    return Am - Bm @ G, G, Ci


def reduced_K(qp):
    """K in fp64 as oracle.osqp_ref.OSQPRef forms it."""
    A = qp["A"]
    return (sp.diags(qp["P"] + qp["sigma"]) + A.T @ sp.diags(qp["rho"]) @ A).tocsr()


def admm_iterate(solve, qp, k, x0=None, z0=None, y0=None, dtype=LD, ops=None):
    """k OSQP iterations in ``dtype`` with the linear solve ``solve(rhs)``; returns the iterates
    [(x, z, y)] after iterations 1 .. k.  ops: the A products (NodeBlocks of the same dtype);
    fp64 without ops multiplies with the scipy matrix, as the oracle does."""
    dt = dtype
    n, m = qp["n"], qp["m"]
    if ops is None:
        if dt is not np.float64:
            ops = NodeBlocks(qp, dt)
    mul = (lambda v: qp["A"] @ v) if ops is None else ops.mul
    tmul = (lambda v: qp["A"].T @ v) if ops is None else ops.tmul
    q, l, u, rho = (np.asarray(qp[key], dt) for key in ("q", "l", "u", "rho"))
    sigma, alpha = dt(qp["sigma"]), dt(qp["alpha"])
    x = np.zeros(n, dt) if x0 is None else np.asarray(x0, dt)
    z = np.zeros(m, dt) if z0 is None else np.asarray(z0, dt)
    y = np.zeros(m, dt) if y0 is None else np.asarray(y0, dt)
    hist = []
    for _ in range(k):
        xt = np.asarray(solve(sigma * x - q + tmul(rho * z - y)), dt)
        zt = mul(xt)
        x = alpha * xt + (1 - alpha) * x
        zr = alpha * zt + (1 - alpha) * z
        z = np.clip(zr + y / rho, l, u)
        y = y + rho * (zr - z)
        hist.append((x, z, y))
    return hist


class Reference:
    """Everything the tests compare with, for one QP: the long-double factor stages and iterates
    and the two fp64 routes; iterates are computed on demand from a given start and cached."""

    def __init__(self, qp):
        from oracle.osqp_ref import BlockReduced
        self.qp = qp
        self.nb = NodeBlocks(qp, LD)
        self.ld = LDFactor(self.nb)
        self.nb64 = NodeBlocks(qp, np.float64)
        K = reduced_K(qp)
        self.block64 = BlockReduced(K, qp["blocks"])
        self._K = K
        self._lu = None
        self._runs = {}

    def lu_solve(self, r):
        if self._lu is None:
            self._lu = spla.splu(self._K.tocsc())
        return self._lu.solve(r)

    def iterates(self, route, k, start=None, key="cold"):
        """[(x, z, y)] of iterations 1 .. k by route "ld", "block64" or "lu64"."""
        ck = (route, key)
        if ck not in self._runs or len(self._runs[ck]) < k:
            x0, z0, y0 = start if start is not None else (None, None, None)
            if route == "ld":
                h = admm_iterate(self.ld.solve, self.qp, k, x0, z0, y0, LD, self.nb)
            elif route == "block64":
                h = admm_iterate(self.block64.solve, self.qp, k, x0, z0, y0, np.float64)
            else:
                h = admm_iterate(self.lu_solve, self.qp, k, x0, z0, y0, np.float64)
            self._runs[ck] = h
        return self._runs[ck][:k]

    def e64(self, k, start=None, key="cold"):
        """Relative inf-norm error of the fp64 block route's x, z, y after k iterations."""
        a = self.iterates("block64", k, start, key)[k - 1]
        r = self.iterates("ld", k, start, key)[k - 1]
        return {nm: rel(a[j], r[j]) for j, nm in enumerate("xzy")}

    def e64_factor(self, i):
        """Errors of the fp64 block route's S_i and (nodes with u columns) A', G, C^-1."""
        out = {"S": rel(self.block64.S[i], self.ld.S[i])}
        if self.qp["blocks"][i][1] > self.qp["blocks"][i][2]:
            ref = node_stages(self.nb, i)
            got = node_stages(self.nb64, i, lapack=True)
            out.update({nm: rel(g, r) for nm, g, r in zip(("Ap", "G", "Cinv"), got, ref)})
        return out


def floor(k, nw_max):
    """Rounding of the sums themselves, k nw_max 2^-52: the bar where the fp64 route's error is ~0."""
    return k * nw_max * 2.0 ** -52
