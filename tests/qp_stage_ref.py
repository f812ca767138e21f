"""Stage references for the QP setup (Ruiz scaling, k_qp_finish), k_admm_init, the termination
check (k_check_part, k_check) and k_unscale (shared by test_qp_stage_ref.py and
test_qp_stages_gpu.py; a plain module, no fixtures; the cases, handles and the error measure are
stage_ref's).

Everything works on ONE problem's data as plain arrays over the Jacobian pattern (rows, cols):

    raw  = dict(rows, cols, m, n, A (values in pattern order), P, q (the gradient), g, lbg, ubg,
                blocks [(x_off, nw, ndx)], node_rows [row indices of node i])

raw_from_device reads it back from a handle, raw_from_oracle builds it from the numpy oracle.  The
long-double functions restate oracle/osqp_ref.py (OSQPRef._scale, update_and_solve lines 195-205,
_info, _check, _primal_infeasible, _dual_infeasible), which stays the authority; the fp64
companions (scale64, finish64, info64, terminate64) call those methods themselves.

Margins.  scale_ld returns every argument of a _limit clamp, finish_ld the two sides of every
rho-class decision and check_ld the two sides of every comparison it evaluated, so a test can
assert that no decision sits where rounding could flip it (margin, clamp_margin).  check_ld
records the comparisons that decide something: the thresholds, the bound classes us > big /
ls < -big of every row and the sign tests of delta_y where delta_y is not zero (at zero both
branches give the same value) and, in the dual certificate, A dx against +-eps |dx| on the rows
whose bound is finite.
"""
import numpy as np
import scipy.sparse as sp

import stage_ref as sr
from stage_ref import LD

from oracle import osqp_ref as O

EPS64 = 2.0 ** -52


# ---------------------------------------------------------------------------- data
def raw_from_device(bo, b, arrays=None):
    """Problem b's raw QP data as the device holds it (after an evaluation)."""
    arrays = arrays or read_raw(bo)
    rows, cols = bo.pattern()
    nodes = bo.node_table()
    X = bo.layout.ndx
    return dict(rows=rows.astype(np.int64), cols=cols.astype(np.int64), m=bo.m, n=bo.n,
                A=arrays["Araw"][b].copy(), P=arrays["P"][b].copy(), q=arrays["grad"][b].copy(),
                g=arrays["g"][b].copy(), lbg=arrays["lbg"][b].copy(), ubg=arrays["ubg"][b].copy(),
                blocks=[(int(nd[2]), int(nd[0]), X) for nd in nodes],
                node_rows=[np.arange(int(nd[3]), int(nd[3]) + int(nd[4])) for nd in nodes])


def read_raw(bo):
    B = bo.batch
    return {k: bo.debug(k, B * ln).reshape(B, ln) for k, ln in
            (("Araw", bo.nnz), ("P", bo.n), ("grad", bo.n), ("g", bo.m), ("lbg", bo.m), ("ubg", bo.m))}


def raw_from_oracle(tag, N, prob=1):
    """The same dict from the numpy oracle alone (stage_ref.oracle_qp's data; g = 0, the bounds
    are the oracle's l and u)."""
    qp, o, (grad, Ax, l, u) = sr.oracle_qp(tag, N, prob)
    pat = o.osqp.A_pat
    cols = np.repeat(np.arange(pat.shape[1]), np.diff(pat.indptr)).astype(np.int64)
    return dict(rows=pat.indices.astype(np.int64), cols=cols, m=pat.shape[0], n=pat.shape[1],
                A=np.asarray(Ax, float).copy(), P=o.osqp.P_raw.copy(), q=np.asarray(grad, float).copy(),
                g=np.zeros(pat.shape[0]), lbg=np.asarray(l, float).copy(), ubg=np.asarray(u, float).copy(),
                blocks=qp["blocks"], node_rows=[np.asarray(r) for r in qp["rows"]]), o.osqp.s


def settings_of(bo):
    s = dict(O.REFERENCE_SETTINGS)
    s.update({k: bo.settings[k] for k in s if k in bo.settings})
    return s


def node_of_col(raw, j):
    return max(i for i, (o, w, _) in enumerate(raw["blocks"]) if o <= j)


def node_of_row(raw, r):
    for i, rr in enumerate(raw["node_rows"]):
        if rr.size and r in rr:
            return i
    return -1


def _amax(idx, v, size):
    out = np.zeros(size, v.dtype)
    np.maximum.at(out, idx, v)
    return out


def _asum(idx, v, size):
    out = np.zeros(size, v.dtype)
    np.add.at(out, idx, v)
    return out


def _csc(raw, vals):
    """scipy matrix of the pattern with the values as they are (explicit zeros kept)."""
    return sp.csc_matrix((np.asarray(vals, float), (raw["rows"], raw["cols"])), shape=(raw["m"], raw["n"]))


def _osqp(raw, settings):
    pat = _csc(raw, np.ones(raw["rows"].size))
    return O.OSQPRef(np.zeros(raw["n"]), pat, settings)


# ---------------------------------------------------------------------------- scaling
def _limit_ld(v):
    v = np.where(v < LD(O.MIN_SCALING), LD(1), v)
    return np.where(v > LD(O.MAX_SCALING), LD(O.MAX_SCALING), v)


def scale_ld(P, q, A, settings):
    """OSQP 0.6 scale_data (OSQPRef._scale) in long double.  A = (rows, cols, values, m).
    Returns dict(D, E, c, P, q, A (values in pattern order), clamps: every _limit argument)."""
    rows, cols, vals, m = A
    n = P.size
    P, q, vals = np.asarray(P, LD).copy(), np.asarray(q, LD).copy(), np.asarray(vals, LD).copy()
    D, E, c = np.ones(n, LD), np.ones(m, LD), LD(1)
    clamps = []
    for _ in range(settings["scaling"]):
        a = np.abs(vals)
        Dt = np.maximum(np.abs(P), _amax(cols, a, n))
        Et = _amax(rows, a, m)
        clamps += [Dt.copy(), Et.copy()]
        Dt = 1 / np.sqrt(_limit_ld(Dt))
        Et = 1 / np.sqrt(_limit_ld(Et))
        P = Dt * P * Dt
        vals = Et[rows] * vals * Dt[cols]
        q = Dt * q
        D, E = D * Dt, E * Et
        ct = np.mean(np.abs(P))
        iq = np.abs(q).max()
        clamps.append(np.array([iq]))
        lq = _limit_ld(np.array([iq]))[0]
        ct = max(ct, lq)
        # the cost scale's second clamp: when the first one clamped |q| to MAX_SCALING and that
        # won the max, its argument IS the constant MAX_SCALING, not a computed number (a 1e8
        # gradient always gets there); v > MAX ? MAX : v then returns MAX on either side, so it is
        # the one argument that is not held to the margin
        if not (iq > LD(O.MAX_SCALING) and ct == lq):
            clamps.append(np.array([ct]))
        ct = 1 / _limit_ld(np.array([ct]))[0]
        P, q, c = P * ct, q * ct, c * ct
    return dict(D=D, E=E, c=c, P=P, q=q, A=vals, clamps=np.concatenate(clamps))


def scale64(raw, settings):
    """OSQPRef._scale itself on the same data; the same keys as scale_ld."""
    P, q, A, D, E, c = _osqp(raw, settings)._scale(raw["P"], raw["q"], _csc(raw, raw["A"]))
    return dict(D=D, E=E, c=c, P=P, q=q, A=np.asarray(A.tocsr()[raw["rows"], raw["cols"]]).ravel())


def clamp_margin(clamps):
    """Smallest relative distance of a _limit argument from a threshold."""
    c = np.asarray(clamps, LD)
    return float(min(np.abs(c / LD(t) - 1).min() for t in (O.MIN_SCALING, O.MAX_SCALING)))


def finish_ld(lbg, ubg, g, E, settings):
    """l, u clamped to +-OSQP_INFTY, ls = E l, us = E u and the rho classes of update_and_solve
    lines 201-205.  decisions: (left, right, rounding scale) of every class comparison."""
    l = np.maximum(np.asarray(lbg, LD) - np.asarray(g, LD), -LD(O.OSQP_INFTY))
    u = np.minimum(np.asarray(ubg, LD) - np.asarray(g, LD), LD(O.OSQP_INFTY))
    E = np.asarray(E, LD)
    ls, us = E * l, E * u
    big = LD(O.OSQP_INFTY) * LD(O.MIN_SCALING)
    loose = (ls < -big) & (us > big)
    eq = (~loose) & (us - ls < LD(O.RHO_TOL))
    rho = np.full(ls.size, settings["rho"])
    rho[loose] = O.RHO_MIN
    rho[eq] = O.RHO_EQ_OVER_RHO_INEQ * settings["rho"]
    mag = np.abs(us) + np.abs(ls)
    dec = [(-ls, np.full(ls.size, big), np.abs(ls)), (us, np.full(ls.size, big), np.abs(us)),
           ((us - ls)[~loose], np.full(int((~loose).sum()), LD(O.RHO_TOL)), mag[~loose])]
    return dict(ls=ls, us=us, rho=rho, loose=loose, eq=eq, decisions=dec)


def finish64(raw, E, settings):
    """update_and_solve lines 195-205 in fp64 on the same data."""
    l = np.maximum(raw["lbg"] - raw["g"], -O.OSQP_INFTY)
    u = np.minimum(raw["ubg"] - raw["g"], O.OSQP_INFTY)
    return dict(ls=E * l, us=E * u)


def rho_margin(decisions):
    """Smallest |left - right| of a rho-class decision in units of the fp64 rounding of its
    operands (the bar: 1e6)."""
    out = np.inf
    for a, b, mag in decisions:
        if a.size:
            out = min(out, float((np.abs(a - b) / (LD(EPS64) * np.maximum(mag, np.abs(b)))).min()))
    return out


# ---------------------------------------------------------------------------- k_admm_init
def rhs_any(raw, qp, x, z, y, sigma, dt):
    """sigma x - q + A^T (rho z - y) on the scaled QP ``qp`` (dict A, q, rho) in ``dt``."""
    A, q, rho = (np.asarray(qp[k], dt) for k in ("A", "q", "rho"))
    x, z, y = (np.asarray(v, dt) for v in (x, z, y))
    return dt(sigma) * x - q + _asum(raw["cols"], A * (rho * z - y)[raw["rows"]], raw["n"])


# ---------------------------------------------------------------------------- termination
CHK = ("pri", "nz", "nax", "dua", "nq", "naty", "npx")


def _partials(raw, rowv, colv):
    """Per-node maxima [N + 1][7] of three row vectors and four column vectors (k_check_part's
    d.chk: |E^-1 (A x - z)|, |E^-1 z|, |E^-1 A x| over the node's rows, |D^-1 (P x + q + A^T y)|,
    |D^-1 q|, |D^-1 A^T y|, |D^-1 P x| over w_i)."""
    out = np.zeros((len(raw["blocks"]), 7), rowv[0].dtype)
    for i, ((o, w, _), rr) in enumerate(zip(raw["blocks"], raw["node_rows"])):
        for k, v in enumerate(rowv):
            out[i, k] = np.abs(v[rr]).max() if rr.size else 0
        for k, v in enumerate(colv):
            out[i, 3 + k] = np.abs(v[o:o + w]).max()
    return out


def info_ld(raw, qp, x, z, y, D, E, c):
    """OSQPRef._info in long double, with the per-node partial maxima."""
    A, P, q = (np.asarray(qp[k], LD) for k in ("A", "P", "q"))
    x, z, y, D, E = (np.asarray(v, LD) for v in (x, z, y, D, E))
    Einv, Dinv, cinv = 1 / E, 1 / D, 1 / LD(c)
    Ax = _asum(raw["rows"], A * x[raw["cols"]], raw["m"])
    Aty = _asum(raw["cols"], A * y[raw["rows"]], raw["n"])
    Px = P * x
    part = _partials(raw, (Einv * (Ax - z), Einv * z, Einv * Ax), (Dinv * (q + Px + Aty), Dinv * q, Dinv * Aty,
                                                                      Dinv * Px))
    tot = part.max(axis=0)
    return dict(pri_res=tot[0], dua_res=cinv * tot[3], norms=tot, part=part, cinv=cinv)


def info64(raw, qp, x, z, y, D, E, c, settings):
    """OSQPRef._info itself; the partial maxima from the vectors it returns."""
    A = _csc(raw, qp["A"])
    Dinv, Einv, cinv = 1.0 / D, 1.0 / E, 1.0 / c
    info = _osqp(raw, settings)._info(qp["P"], qp["q"], A, x, z, y, Dinv, Einv, cinv)
    info["part"] = _partials(raw, (Einv * (info["Ax"] - z), Einv * z, Einv * info["Ax"]),
                             (Dinv * (qp["q"] + info["Px"] + info["Aty"]), Dinv * qp["q"], Dinv * info["Aty"],
                              Dinv * info["Px"]))
    return info


def check_ld(raw, qp, info, dx, dy, D, E, c, settings, approximate):
    """OSQPRef._check with _primal_infeasible and _dual_infeasible in long double.  Returns
    (status, comparisons): the (left, right) arrays of every comparison evaluated."""
    s = settings
    mul = 10 if approximate else 1
    eps_abs, eps_rel = LD(s["eps_abs"]) * mul, LD(s["eps_rel"]) * mul
    eps_pinf, eps_dinf = LD(s["eps_prim_inf"]) * mul, LD(s["eps_dual_inf"]) * mul
    A, P, q, ls, us = (np.asarray(qp[k], LD) for k in ("A", "P", "q", "l", "u"))
    dx, dy, D, E = (np.asarray(v, LD) for v in (dx, dy, D, E))
    c, cinv = LD(c), info["cinv"]
    rows, cols, m, n = raw["rows"], raw["cols"], raw["m"], raw["n"]
    comps = []

    def cmp(a, b):
        comps.append((np.atleast_1d(np.asarray(a, LD)), np.atleast_1d(np.asarray(b, LD))))

    inf = LD(O.OSQP_INFTY)
    cmp(info["pri_res"], inf)
    if info["pri_res"] > inf:
        return O.NON_CVX, comps
    cmp(info["dua_res"], inf)
    if info["dua_res"] > inf:
        return O.NON_CVX, comps
    nm = info["norms"]
    eps_prim = eps_abs + eps_rel * max(nm[1], nm[2])
    cmp(info["pri_res"], eps_prim)
    prim_ok = info["pri_res"] < eps_prim
    big = inf * LD(O.MIN_SCALING)
    prim_inf = False
    if not prim_ok:
        cmp(us, np.full(m, big))
        cmp(ls, np.full(m, -big))
        uinf, linf = us > big, ls < -big
        one = (uinf ^ linf) & (dy != 0)
        cmp(dy[one], np.zeros(int(one.sum()), LD))
        dyp = np.where(uinf & linf, LD(0), np.where(uinf, np.minimum(dy, 0), np.where(linf, np.maximum(dy, 0), dy)))
        ndy = np.abs(E * dyp).max()
        cmp(ndy, O.OSQP_DIVISION_TOL)
        if ndy > O.OSQP_DIVISION_TOL:
            ineq = np.sum(us * np.maximum(dyp, 0) + ls * np.minimum(dyp, 0))
            cmp(ineq, eps_pinf * ndy)
            if ineq < eps_pinf * ndy:
                natdy = np.abs(_asum(cols, A * dyp[rows], n) / D).max()
                cmp(natdy, eps_pinf * ndy)
                prim_inf = bool(natdy < eps_pinf * ndy)
    eps_dual = eps_abs + eps_rel * cinv * max(nm[4], nm[5], nm[6])
    cmp(info["dua_res"], eps_dual)
    dual_ok = info["dua_res"] < eps_dual
    dual_inf = False
    if not dual_ok:
        ndx = np.abs(D * dx).max()
        cmp(ndx, O.OSQP_DIVISION_TOL)
        if ndx > O.OSQP_DIVISION_TOL:
            qdx = np.sum(q * dx)
            cmp(qdx, c * eps_dinf * ndx)
            if qdx < c * eps_dinf * ndx:
                npdx = np.abs(P * dx / D).max()
                cmp(npdx, c * eps_dinf * ndx)
                if npdx < c * eps_dinf * ndx:
                    adx = _asum(rows, A * dx[cols], m) / E
                    cmp(us, np.full(m, big))
                    cmp(ls, np.full(m, -big))
                    fu, fl = us < big, ls > -big
                    cmp(adx[fu], np.full(int(fu.sum()), eps_dinf * ndx))
                    cmp(adx[fl], np.full(int(fl.sum()), -eps_dinf * ndx))
                    dual_inf = not bool(np.any((fu & (adx > eps_dinf * ndx)) | (fl & (adx < -eps_dinf * ndx))))
    if prim_ok and dual_ok:
        return (O.SOLVED_INACCURATE if approximate else O.SOLVED), comps
    if prim_inf:
        return (O.PRIMAL_INFEASIBLE_INACCURATE if approximate else O.PRIMAL_INFEASIBLE), comps
    if dual_inf:
        return (O.DUAL_INFEASIBLE_INACCURATE if approximate else O.DUAL_INFEASIBLE), comps
    return O.UNSOLVED, comps


def margin(comps):
    """Smallest relative distance |a - b| / max(|a|, |b|) over the comparisons (0 / 0 counts as 0)."""
    out = np.inf
    for a, b in comps:
        if a.size:
            den = np.maximum(np.abs(a), np.abs(b))
            out = min(out, float(np.where(den > 0, np.abs(a - b) / np.where(den > 0, den, 1), 0).min()))
    return out


def terminate(check, final):
    """One termination check as the solver runs it (update_and_solve lines 241-249, k_check):
    the plain pass, and on the final check the x10 pass and MAX_ITER_REACHED.  check(approximate)
    -> (status, comparisons)."""
    st, comps = check(False)
    if st != O.UNSOLVED or not final:
        return st, comps
    st2, c2 = check(True)
    return (st2 if st2 != O.UNSOLVED else O.MAX_ITER_REACHED), comps + c2


def terminate_ld(raw, qp, it, D, E, c, settings, final):
    """Reference status of the state ``it`` = dict(x, z, y, dx, dy) on the scaled QP ``qp``."""
    info = info_ld(raw, qp, it["x"], it["z"], it["y"], D, E, c)
    st, comps = terminate(lambda ap: check_ld(raw, qp, info, it["dx"], it["dy"], D, E, c, settings, ap), final)
    return st, comps, info


def terminate64(raw, qp, it, D, E, c, settings, final):
    """The same through OSQPRef._info and OSQPRef._check themselves."""
    os_ = _osqp(raw, settings)
    A = _csc(raw, qp["A"])
    Dinv, Einv, cinv = 1.0 / D, 1.0 / E, 1.0 / c
    info = os_._info(qp["P"], qp["q"], A, it["x"], it["z"], it["y"], Dinv, Einv, cinv)
    st, _ = terminate(lambda ap: (os_._check(info, qp["P"], qp["q"], A, qp["l"], qp["u"], it["dx"], it["dy"], D, Dinv,
                                             Einv, c, cinv, ap), []), final)
    return st, info


# ---------------------------------------------------------------------------- crafted raw data
def craft_raw(raw, settings, seed, variant):
    """Section (b)'s construction on a copy of ``raw``: returns (crafted raw, what: the chosen
    rows / columns by name).  variant 0: gradient of inf-norm 1e8, 1: 1e-8, 2: as it is.

    Columns: one all-zero with P_jj = 0 (a u column of node 0), one of norm 1e7 (a dx column of
    node 1: entries of two nodes), one of norm 1e-7 (in the last node's dx block).  Rows, none of
    them touching those columns: all-zero (node 0), norm 1e7 (middle node), norm 1e-7 (node N - 1);
    free with +-1e31 (node 0) and +-inf (node N - 1); upper side infinite (middle), lower side
    infinite (node 0); equality (node N - 1); u - l = RHO_TOL (1 +- 1e-3) / E_r with E of the
    long-double scaling of the crafted matrix (above: node 0 and middle, below: middle and node
    N - 1), with l = 0 so that the rounding of E (u - l) is 1e9 times smaller than the distance."""
    rng = np.random.default_rng(seed)
    r = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in raw.items()}
    rows, cols, A = r["rows"], r["cols"], r["A"]
    bl = r["blocks"]
    nrn = [i for i, rr in enumerate(r["node_rows"]) if rr.size]  # nodes with rows: 0 .. N - 1
    first, mid, last = nrn[0], nrn[len(nrn) // 2], nrn[-1]
    what = {}
    o0, w0, X = bl[0]
    what["col_zero"] = int(o0 + X + rng.integers(w0 - X))
    what["col_big"] = int(bl[1][0] + rng.integers(X))
    what["col_small"] = int(bl[-1][0] + rng.integers(X))
    ccols = [what["col_zero"], what["col_big"], what["col_small"]]
    touched = set(rows[np.isin(cols, ccols)].tolist())
    used = set()

    def pick(node, name):
        cand = [int(x) for x in r["node_rows"][node] if int(x) not in touched and int(x) not in used
                and np.any((rows == x) & (A != 0))]
        x = cand[int(rng.integers(len(cand)))]
        used.add(x)
        what[name] = x
        return x

    j = what["col_zero"]
    A[cols == j] = 0.0
    r["P"][j] = 0.0
    j = what["col_big"]
    A[cols == j] *= 1e7 / np.abs(A[cols == j]).max()
    r["P"][j] = min(abs(r["P"][j]), 1.0)
    j = what["col_small"]
    A[cols == j] *= 1e-7 / np.abs(A[cols == j]).max()
    r["P"][j] = 0.25e-7
    A[rows == pick(first, "row_zero")] = 0.0
    x = pick(mid, "row_big")
    A[rows == x] *= 1e7 / np.abs(A[rows == x]).max()
    x = pick(last, "row_small")
    A[rows == x] *= 1e-7 / np.abs(A[rows == x]).max()
    if variant < 2:
        r["q"] *= (1e8, 1e-8)[variant] / np.abs(r["q"]).max()
    g, lbg, ubg = r["g"], r["lbg"], r["ubg"]
    x = pick(first, "row_free_1e31")
    lbg[x], ubg[x] = -1e31, 1e31
    x = pick(last, "row_free_inf")
    lbg[x], ubg[x] = -np.inf, np.inf
    x = pick(mid, "row_upper_inf")
    lbg[x], ubg[x] = g[x] - 0.5, 1e31
    x = pick(first, "row_lower_inf")
    lbg[x], ubg[x] = -np.inf, g[x] + 0.25
    x = pick(last, "row_eq")
    lbg[x] = ubg[x] = g[x] + 0.125
    E = scale_ld(r["P"], r["q"], (rows, cols, A, r["m"]), settings)["E"]
    for name, node, f in (("row_above_a", first, 1 + 1e-3), ("row_above_b", mid, 1 + 1e-3),
                          ("row_below_a", mid, 1 - 1e-3), ("row_below_b", last, 1 - 1e-3)):
        x = pick(node, name)
        lbg[x] = g[x]
        ubg[x] = g[x] + float(LD(O.RHO_TOL) * LD(f) / E[x])
    return r, what


def check_crafted(raw, what, fin, variant, settings):
    """The properties section (b) asks of the construction, on the reference's own numbers."""
    rows, cols, A = raw["rows"], raw["cols"], raw["A"]
    cn = np.maximum(np.abs(raw["P"]), _amax(cols, np.abs(A), raw["n"]))
    rn = _amax(rows, np.abs(A), raw["m"])
    assert cn[what["col_zero"]] == 0 and rn[what["row_zero"]] == 0
    assert abs(cn[what["col_big"]] / 1e7 - 1) < 1e-12 and abs(cn[what["col_small"]] / 1e-7 - 1) < 1e-12
    assert abs(rn[what["row_big"]] / 1e7 - 1) < 1e-12 and abs(rn[what["row_small"]] / 1e-7 - 1) < 1e-12
    if variant < 2:
        assert abs(np.abs(raw["q"]).max() / (1e8, 1e-8)[variant] - 1) < 1e-12
    nodes = {node_of_row(raw, what[k]) for k in what if k.startswith("row_")}
    nrn = [i for i, rr in enumerate(raw["node_rows"]) if rr.size]
    assert {nrn[0], nrn[len(nrn) // 2], nrn[-1]} <= nodes
    j = what["col_big"]  # a dx_{i+1} column: written by two nodes' rows
    assert len({node_of_row(raw, int(x)) for x in rows[cols == j]}) == 2
    rho, s = fin["rho"], settings["rho"]
    assert fin["loose"][what["row_free_1e31"]] and fin["loose"][what["row_free_inf"]]
    for k in ("row_upper_inf", "row_lower_inf", "row_above_a", "row_above_b"):
        assert not fin["loose"][what[k]] and not fin["eq"][what[k]], k
    for k in ("row_eq", "row_below_a", "row_below_b"):
        assert fin["eq"][what[k]], k
    assert rho[what["row_free_inf"]] == O.RHO_MIN and rho[what["row_eq"]] == 1e3 * s and rho[what["row_above_a"]] == s


# ---------------------------------------------------------------------------- crafted termination states
def base_state(raw, qp, D, E, c, settings, seed, fp, fd):
    """Generic iterates with pri_res = fp eps_prim and dua_res = fd eps_dual (to the per cent):
    random x and y, z = A x + t p with |E^-1 p| = 1 and q = -(P x + A^T y) + s w with |D^-1 w| = 1.
    Returns (qp with the new q, state); delta_x = delta_y = 0."""
    rng = np.random.default_rng(seed)
    n, m = raw["n"], raw["m"]
    x, y = 0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(m)
    p, w = E * rng.choice([-1.0, 1.0], m) * rng.uniform(0.2, 1.0, m), D * rng.choice([-1.0, 1.0], n) * rng.uniform(
        0.2, 1.0, n)
    p *= 1 / np.abs(p / E).max()
    w *= 1 / np.abs(w / D).max()
    A = _csc(raw, qp["A"])
    Ax, Aty, Px = A @ x, A.T @ y, qp["P"] * x
    eps_p = settings["eps_abs"] + settings["eps_rel"] * np.abs(Ax / E).max()
    z = Ax + fp * eps_p * p
    q0 = -(Px + Aty)
    eps_d = settings["eps_abs"] + settings["eps_rel"] / c * max(np.abs(q0 / D).max(), np.abs(Aty / D).max(),
                                                                 np.abs(Px / D).max())
    q = q0 + fd * eps_d * c * w
    new = dict(qp, q=q, A=qp["A"].copy(), P=qp["P"].copy(), l=qp["l"].copy(), u=qp["u"].copy())
    return new, dict(x=x, z=z, y=y, dx=np.zeros(n), dy=np.zeros(m))


STATE_NAMES = ("solved", "unsolved", "max_iter", "solved_inaccurate", "non_convex", "primal", "primal_near_miss",
               "primal_inaccurate", "primal_projected", "primal_projection_kept", "dual", "dual_near_miss",
               "dual_inaccurate")


def craft_state(name, raw, qp, D, E, c, settings, seed):
    """Section (e)'s constructions on one scaled QP (dict A, P, q, l, u): returns (qp', state,
    final, expected status).  Every certificate case starts from iterates 20 x outside both
    thresholds, so that neither the plain nor the x10 pass accepts them as solved."""
    rows, cols = raw["rows"], raw["cols"]
    rng = np.random.default_rng(seed + 1000)
    ep, ed = settings["eps_prim_inf"], settings["eps_dual_inf"]
    if name == "solved":
        q2, st = base_state(raw, qp, D, E, c, settings, seed, 0.5, 0.5)
        return q2, st, False, O.SOLVED
    if name in ("unsolved", "max_iter"):
        q2, st = base_state(raw, qp, D, E, c, settings, seed, 20.0, 20.0)
        st["dx"], st["dy"] = 0.1 * rng.standard_normal(raw["n"]), 0.1 * rng.standard_normal(raw["m"])
        return q2, st, name == "max_iter", (O.MAX_ITER_REACHED if name == "max_iter" else O.UNSOLVED)
    if name == "solved_inaccurate":
        q2, st = base_state(raw, qp, D, E, c, settings, seed, 3.0, 3.0)
        return q2, st, True, O.SOLVED_INACCURATE
    if name == "non_convex":
        q2, st = base_state(raw, qp, D, E, c, settings, seed, 0.5, 0.5)
        j = int(cols[np.flatnonzero(qp["A"] != 0)[rng.integers(np.count_nonzero(qp["A"]))]])
        st["x"][j] = 1e40
        return q2, st, False, O.NON_CVX
    q2, st = base_state(raw, qp, D, E, c, settings, seed, 20.0, 20.0)
    A, l, u = q2["A"], q2["l"], q2["u"]
    nz_rows = np.unique(rows[A != 0])
    if name.startswith("primal"):
        pick = rng.choice(nz_rows, 4, replace=False)
        r0 = int(pick[0])
        l[r0] = u[r0] = -1.0
        st["dy"][r0] = 1.0
        ent = np.flatnonzero(rows == r0)
        A[ent] = 0.0
        if name in ("primal_near_miss", "primal_inaccurate"):  # |D^-1 A^T dy| = 1.5 eps |E dy|
            e = int(ent[rng.integers(ent.size)])
            A[e] = 1.5 * ep * E[r0] * D[cols[e]]
        if name in ("primal_projected", "primal_projection_kept"):
            ru, rl, rb = (int(v) for v in pick[1:])
            l[ru], u[ru] = -1.0, 1e30  # the other side finite whatever the row was
            l[rl], u[rl] = -1e30, 1.0
            l[rb], u[rb] = -1e30, 1e30
            st["dy"][ru], st["dy"][rl], st["dy"][rb] = 5.0, -5.0, 5.0  # all three projected to 0
            if name == "primal_projection_kept":
                st["dy"][ru] = -5.0  # min(dy, 0) keeps it: A^T dy is no longer small
        final = name == "primal_inaccurate"
        want = {"primal": O.PRIMAL_INFEASIBLE, "primal_projected": O.PRIMAL_INFEASIBLE,
                "primal_near_miss": O.UNSOLVED, "primal_projection_kept": O.UNSOLVED,
                "primal_inaccurate": O.PRIMAL_INFEASIBLE_INACCURATE}[name]
        return q2, st, final, want
    # dual certificate: dx = e_j, P_jj = 0, q_j < 0, the column's only entry +a in a row whose
    # upper side is infinite (dual), finite (near miss), or a = 3 eps |D dx| E_r (x10 pass only)
    cand = [int(j) for j in np.unique(cols[A != 0])]
    j = cand[int(rng.integers(len(cand)))]
    ent = np.flatnonzero(cols == j)
    e = int(ent[rng.integers(ent.size)])
    r0 = int(rows[e])
    A[ent] = 0.0
    A[e] = 1.0
    q2["P"][j] = 0.0
    q2["q"][j] = -abs(q2["q"][j]) - 1.0
    st["dx"][j] = 1.0
    l[r0], u[r0] = -1.0, 1e30
    if name != "dual":
        u[r0] = 1.0
    if name == "dual_inaccurate":
        A[e] = 3.0 * ed * D[j] * E[r0]
    want = {"dual": O.DUAL_INFEASIBLE, "dual_near_miss": O.UNSOLVED, "dual_inaccurate": O.DUAL_INFEASIBLE_INACCURATE}
    return q2, st, name == "dual_inaccurate", want[name]


def floor_products(settings):
    """Rounding of the cumulative scaling products: scaling_passes * 4 * 2^-52."""
    return settings["scaling"] * 4 * EPS64


def rel_entry(a, ref):
    """Largest entrywise relative error |a - ref| / |ref| and where; an entry whose reference is
    zero or infinite must be equal.  The scaled quantities are products, so nothing cancels."""
    a, ref = np.atleast_1d(np.asarray(a, LD)), np.atleast_1d(np.asarray(ref, LD))
    fin = np.isfinite(ref) & (ref != 0)
    err = np.zeros(ref.shape, LD)
    err[fin] = np.abs(a[fin] - ref[fin]) / np.abs(ref[fin])
    err[~fin] = np.where(a[~fin] == ref[~fin], 0, np.inf)
    err = np.where(np.isnan(err), np.inf, err)
    k = int(np.argmax(err))
    return float(err[k]), k
