"""Stage references for the interior-point kernels of k_ip.hip (shared by test_ip_stage_ref.py and
test_ip_stages_gpu.py; a plain module, no fixtures; the cases and handles are stage_ref's).

One function per stage -- init_ld (k_ip_init), kkt_ld (k_ip_kkt), inertia_ref (k_ip_inertia),
step_ld (k_ip_step) -- each a restatement of the corresponding block of oracle/ip_ref.py
(IPRef.solve, which stays the authority) on explicit state dicts

    state = dict(x, s, lam, zl, zu, mu, theta_min, theta_max, filt [(theta, phi)], dw_last)
    data  = dict(g, lbg, ubg, grad, J (csr, fp64), P (Hessian diagonal), f)   at state["x"]

in the arithmetic ``dt``.  dt = np.longdouble is the reference of the GPU tests: row and objective
values at a point come from an evaluator in fp64 (OracleEval: OracleOCP.eval_g / f_and_grad),
everything built on them -- residual norms, sd / sc, the five candidate errors, W / r^, the
directions, fraction-to-boundary, theta / phi / dphi, the filter tests, the update, the clamps --
is long double.  dt = np.float64 runs the same code with IPRef's own operations in IPRef's order,
so chain(..., dt=np.float64) reproduces IPRef.solve to the bit (test_ip_stage_ref.py): that pins
the formulas, which the long-double run shares.

The Newton direction itself is no stage of k_ip.hip (the factor and the sweep kernels solve it,
tests/test_stage_kernels_gpu.py): newton_dir solves it in fp64 by a sparse LU with IPRef's
refinement, and the step stage takes dx and J dx as inputs.

Margins.  Every comparison that decides a branch -- the termination tests, the barrier update's
E_mu <= kappa_eps mu, the refinement rule, theta_max, every filter entry, theta <= theta_min, the
switching condition, Armijo and the two sufficient-decrease tests, and both bounds of the
multiplier clamp where a case is built around it -- goes through Margins.cmp, which records the
relative distance of its two sides |a - b| / max(|a|, |b|).  A case is usable only if every
distance exceeds MARGIN = 1e-9 (1000 x the project's 1e-12 bar on row values).  Comparisons that
only select between two values that agree at the threshold (max / min in the slack push, W_MIN,
the fraction-to-boundary minimum) decide nothing and are covered by the error bounds instead.
Margins.tags collects the branches a run took (the coverage list of test_ip_stage_ref.py).

Error bounds.  Next to each formula stands its operation count c; the bound of an output is
c * eps * (sum of the magnitudes of the formula's terms) plus the propagated bound of its inputs
to first order (a cancelling difference such as s - l carries its inputs' error, not eps of the
result); sums and max-reductions over k terms: (k + c) * eps * sum |terms|; log / pow count 2.
Quantities that contain row values the device evaluated itself (theta, phi, the filter entries,
f at the accepted trial) add ROW_BAR = 1e-12 relative per row summed.  The functions return the
bounds as ``bnd`` (fp64) beside the values.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import stage_ref as sr  # noqa: F401  (sys.path of the repository)
from stage_ref import LD

from oracle import ip_ref as I

EPS64 = 2.0 ** -52
MARGIN = 1e-9
ROW_BAR = 1e-12
MAXFILT = 32  # PL_IP_MAXFILT
INERTIA_CAP = 8


def settings(**kw):
    s = dict(I.IP_SETTINGS)
    s.update(kw)
    return s


# ---------------------------------------------------------------------------- margins
class Margins:
    def __init__(self):
        self.rec = []  # (name, relative distance, outcome)
        self.tags = set()

    @staticmethod
    def dist(a, b):
        a, b = LD(a), LD(b)
        if not (np.isfinite(a) and np.isfinite(b)):
            return np.inf
        sc = max(abs(a), abs(b))
        return float(abs(a - b) / sc) if sc > 0 else 0.0

    def cmp(self, name, a, op, b):
        res = bool({"<=": a <= b, "<": a < b, ">": a > b, ">=": a >= b}[op])
        self.rec.append((name, self.dist(a, b), res))
        return res

    def note(self, name, d, res):
        self.rec.append((name, float(d), bool(res)))

    def tag(self, *t):
        self.tags.update(t)

    def worst(self):
        return min(self.rec, key=lambda r: r[1]) if self.rec else ("none", np.inf, True)

    def ok(self):
        return self.worst()[1] > MARGIN


# ---------------------------------------------------------------------------- evaluators
class OracleEval:
    """Values and derivatives at a point from the numpy oracle (fp64)."""

    def __init__(self, o, p):
        self.o, self.p = o, p
        self._hess = {}

    def values(self, x):
        x = np.asarray(x, np.float64)
        f, _ = self.o.f_and_grad(x, self.p)
        g, _, _ = self.o.eval_g(x, self.p)
        return float(f), g

    def data(self, x):
        x = np.asarray(x, np.float64)
        f, grad = self.o.f_and_grad(x, self.p)
        g, lbg, ubg = self.o.eval_g(x, self.p)
        return dict(g=g, lbg=lbg, ubg=ubg, grad=grad, J=self.o.eval_J(x, self.p).tocsr(), f=float(f),
                    P=self.o.compute_hess_diag(self.p))

    def lag_hess(self, x, lam):
        """Cached by the bits of (x, lam): IPRef.solve and chain ask at the same points."""
        x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
        key = (x.tobytes(), lam.tobytes())
        if key not in self._hess:
            self._hess[key] = self.o.lag_hess(x, self.p, lam)
        return self._hess[key]


class CachedOracle:
    """An OracleOCP whose lag_hess goes through an OracleEval's cache (for IPRef.solve)."""

    def __init__(self, ev):
        self._ev = ev

    def __getattr__(self, k):
        return getattr(self._ev.o, k)

    def lag_hess(self, x, p, lam):
        return self._ev.lag_hess(x, lam)


# ---------------------------------------------------------------------------- helpers
def _classes(lbg, ubg):
    eq, hl, hu = I.row_classes(np.asarray(lbg, np.float64), np.asarray(ubg, np.float64))
    return eq, hl, hu


def _jt(J, v, dt):
    """J^T v: fp64 as IPRef multiplies (scipy), long double entry by entry."""
    if dt is np.float64:
        return J.T @ v
    C = J.tocoo()
    out = np.zeros(J.shape[1], dt)
    np.add.at(out, C.col, np.asarray(C.data, dt) * v[C.row])
    return out


def _jtabs(J, v):
    C = J.tocoo()
    out = np.zeros(J.shape[1], LD)
    np.add.at(out, C.col, np.abs(np.asarray(C.data, LD) * np.asarray(v, LD)[C.row]))
    return out


def _slacks(s, lbg, ubg, hl, hu, dt):
    lb = np.where(hl, lbg, 0.0).astype(dt)
    ub = np.where(hu, ubg, 0.0).astype(dt)
    with np.errstate(all="ignore"):
        return lb, ub, np.where(hl, s - lb, dt(1.0)), np.where(hu, ub - s, dt(1.0))


def _c(g, s, lbg, eq, dt):
    return np.where(eq, g - np.where(eq, lbg, 0.0).astype(dt), g - s)


def _f64(v):
    return np.asarray(v, np.float64)


def _in(v, dt):
    """A stage input in ``dt`` after rounding to fp64: the stages start from what the device is
    given (uploaded doubles), whatever precision the previous stage kept."""
    return np.asarray(_f64(v), dt)


# ---------------------------------------------------------------------------- k_ip_init
def init_ld(g, lbg, ubg, st, lam0=None, dt=LD):
    """Initial slacks, multipliers and the filter's theta bounds (IPRef.solve lines 147-171,
    push_slacks).  Returns (state without x, bnd)."""
    eq, hl, hu = _classes(lbg, ubg)
    g = np.asarray(g, dt)
    mu = dt(st["mu_init"])
    push, frac = dt(st["bound_push"]), dt(st["bound_frac"])
    lb = np.where(hl, lbg, 0.0).astype(dt)
    ub = np.where(hu, ubg, 0.0).astype(dt)
    pl = push * np.maximum(dt(1.0), np.abs(lb))              # c = 1
    pu = push * np.maximum(dt(1.0), np.abs(ub))
    two = hl & hu
    width = np.where(two, ub - lb, dt(np.inf))               # c = 1
    pl = np.where(two, np.minimum(pl, frac * width), pl)     # c = 2 (width, product)
    pu = np.where(two, np.minimum(pu, frac * width), pu)
    s = g.copy()
    s = np.where(hl, np.maximum(s, lb + pl), s)              # c = 3 (push, sum)
    s = np.where(hu, np.minimum(s, ub - pu), s)
    s = np.where(eq, dt(0.0), s)
    sl = np.where(hl, s - lb, dt(1.0))
    su = np.where(hu, ub - s, dt(1.0))
    if lam0 is None:
        lam = np.zeros(g.size, dt)
        zl = np.where(hl, mu / sl, dt(0.0))                  # c = 2 on top of s
        zu = np.where(hu, mu / su, dt(0.0))
    else:
        lam = np.asarray(lam0, dt).copy()
        wp = dt(st["warm_start_mult_bound_push"])
        zl = np.where(hl, np.maximum(np.maximum(-lam, dt(0.0)), wp), dt(0.0))  # exact selections
        zu = np.where(hu, np.maximum(np.maximum(lam, dt(0.0)), wp), dt(0.0))
    terms = np.abs(_c(g, s, lbg, eq, dt))
    theta0 = dt(np.sum(terms))
    out = dict(s=s, lam=lam, zl=zl, zu=zu, mu=mu, theta_max=dt(1e4) * max(dt(1.0), theta0),
               theta_min=dt(1e-4) * max(dt(1.0), theta0), filt=[], dw_last=0.0, theta0=theta0)
    # bounds: s is g itself or l + push (|l| + push, c = 3) or u - push; the cold multipliers divide
    # by the cancelling s - l, which carries s's error: mu / sl^2 * b_s + 2 eps z
    e = LD(EPS64)
    b_s = np.where(eq, LD(0), 3 * e * (np.abs(lb) + np.abs(ub) + np.maximum(pl, pu))).astype(LD)
    if lam0 is None:
        b_zl = np.where(hl, mu / sl ** 2 * b_s + 2 * e * zl, LD(0))
        b_zu = np.where(hu, mu / su ** 2 * b_s + 2 * e * zu, LD(0))
    else:
        b_zl = b_zu = np.zeros(g.size, LD)
    mag = np.where(eq, np.abs(g) + np.abs(np.where(eq, lbg, 0.0)), np.abs(g) + np.abs(s))
    b_th = (g.size + 1) * e * np.sum(mag) + np.sum(b_s)
    bnd = dict(s=_f64(b_s), zl=_f64(b_zl), zu=_f64(b_zu), lam=np.zeros(g.size), theta0=float(b_th),
               theta_max=float(1e4 * b_th + e * out["theta_max"]), theta_min=float(1e-4 * b_th + e * out["theta_min"]))
    return out, bnd


# ---------------------------------------------------------------------------- k_ip_kkt
def next_mu(mu, tol, dt):
    # tol / 10 is a constant of the settings, formed in fp64 as the kernel forms it: the loop's
    # mus[q + 1] == mus[q] test is an equality with this very number
    return max(dt(np.float64(tol) / np.float64(10.0)), min(dt(I.KAPPA_MU) * mu, mu ** dt(I.THETA_MU)))


def kkt_ld(state, data, k, st, mg=None, dt=LD):
    """Iteration k's error, termination test, barrier update and the reduced Newton system's
    diagonal data (IPRef.solve lines 179-216).  Returns dict(err, viol_max, status (None: the
    solve continues), mu, ndec (barrier decreases of this call), W, rhat, qs, c, bs, sig, ...) and
    bnd."""
    mg = mg or Margins()
    g, lbg, ubg = np.asarray(data["g"], dt), data["lbg"], data["ubg"]
    eq, hl, hu = _classes(lbg, ubg)
    iq = ~eq
    m = g.size
    nb = int(hl.sum() + hu.sum())
    s, lam, zl, zu = (_in(state[q], dt) for q in ("s", "lam", "zl", "zu"))
    mu = dt(np.float64(state["mu"]))
    tol = st["tol"]
    grad, J = np.asarray(data["grad"], dt), data["J"]
    lb, ub, sl, su = _slacks(s, lbg, ubg, hl, hu, dt)
    c = _c(g, s, lbg, eq, dt)                                             # c = 1
    rx = grad + _jt(J, lam, dt)                                           # column sum: terms + 1
    rs = np.where(iq, -lam - zl + zu, dt(0.0))                            # c = 2
    S_MAX = dt(I.S_MAX)
    sd = max(S_MAX, (np.sum(np.abs(lam)) + np.sum(zl) + np.sum(zu)) / max(m + nb, 1)) / S_MAX  # sums of m terms
    sc = max(S_MAX, (np.sum(zl) + np.sum(zu)) / max(nb, 1)) / S_MAX
    cl, cu = np.where(hl, sl * zl, dt(0.0)), np.where(hu, su * zu, dt(0.0))    # c = 2

    def nlp_err(mu_):
        comp = max(np.max(np.abs(np.where(hl, cl - mu_, dt(0.0))), initial=dt(0.0)),
                   np.max(np.abs(np.where(hu, cu - mu_, dt(0.0))), initial=dt(0.0)))
        return max(np.max(np.abs(rx)) / sd, np.max(np.abs(rs)) / sd, np.max(np.abs(c)), comp / sc)

    with np.errstate(all="ignore"):
        err = nlp_err(dt(0.0))
    lf = np.where(np.isfinite(lbg), lbg, 0.0)
    uf = np.where(np.isfinite(ubg), ubg, 0.0)
    viol = max(dt(0.0), np.max(np.where(np.isfinite(lbg), lf - g, dt(0.0))),
               np.max(np.where(np.isfinite(ubg), g - uf, dt(0.0))))        # c = 1
    status = None
    if not np.isfinite(err):
        status = I.ST_NONFINITE
        mg.tag("kkt_nonfinite")
    elif mg.cmp("kkt err <= tol", err, "<=", dt(tol)):
        status = I.ST_CONVERGED
        mg.tag("kkt_converged")
    elif k == st["max_iter"]:
        status = I.ST_MAX_ITER
        mg.tag("kkt_max_iter")
    ndec = 0
    if status is None:
        mg.tag("kkt_continue")
        if sd > 1:
            mg.tag("kkt_sd_gt_1")
        if sc > 1:
            mg.tag("kkt_sc_gt_1")
        for _ in range(4):
            if mg.cmp("kkt E_mu > kappa_eps mu", nlp_err(mu), ">", dt(I.KAPPA_EPS) * mu):
                mg.tag("mu_break_error")
                break
            mu_new = next_mu(mu, tol, dt)
            if mu_new == mu:  # both are tol / 10, the same constant: exact on either side
                mg.tag("mu_break_fixed")
                break
            mu = mu_new
            ndec += 1
        else:
            mg.tag("mu_four_decreases")
        mg.tag(f"mu_decreases_{ndec}")
    out = dict(err=err, viol_max=viol, status=status, mu=mu, ndec=ndec, sd=sd, sc=sc, c=c, rx=rx, eq=eq, hl=hl, hu=hu)
    e = LD(EPS64)
    ncol = np.diff(J.tocsc().indptr)
    b_qs = (ncol + 2) * e * (np.abs(np.asarray(data["grad"], LD)) + _jtabs(J, lam))
    with np.errstate(all="ignore"):
        b_comp = 3 * e * (np.abs(cl) + np.abs(cu) + mu)
        b_err = (max(np.max(b_qs) / sd, 3 * e * np.max(np.abs(lam) + zl + zu), e * np.max(np.abs(g) + np.abs(s)),
                     np.max(b_comp) / sc) + (2 * m + 10) * e * err)
    bnd = dict(qs=_f64(b_qs), err=float(b_err) if np.isfinite(b_err) else 0.0,
               viol_max=float(2 * e * np.max(np.abs(g) + np.abs(lf) + np.abs(uf))),
               mu=float(3 * max(ndec, 1) * e * mu) if ndec else 0.0)
    if status is not None:
        return out, bnd
    # ---- reduced Newton system
    dc = dt(st["delta_c"])
    with np.errstate(all="ignore"):
        sig = np.where(hl, zl / sl, dt(0.0)) + np.where(hu, zu / su, dt(0.0))       # c = 5
        W = np.where(eq, dt(1.0) / dc, sig / (dt(1.0) + dc * sig))                 # c = 8 with sig
        if np.any(W < dt(I.W_MIN)):
            mg.tag("kkt_w_min")
        W = np.maximum(W, dt(I.W_MIN))
        bs = np.where(iq, lam + np.where(hl, mu / sl, dt(0.0)) - np.where(hu, mu / su, dt(0.0)), dt(0.0))  # c = 6
        sig_safe = np.where(iq, sig, dt(1.0))
        rhat = np.where(eq, c, c - bs / sig_safe)                                  # c = 14 + 3 per decrease
        mag = np.where(eq, np.abs(g) + np.abs(lb), np.abs(g) + np.abs(s) +
                       (np.abs(lam) + np.where(hl, mu / sl, 0) + np.where(hu, mu / su, 0)) / sig_safe)
    out.update(W=W, rhat=rhat, bs=bs, sig=sig, qs=rx)
    bnd.update(W=_f64(8 * e * W), rhat=_f64((14 + 3 * ndec) * e * mag))
    return out, bnd


# ---------------------------------------------------------------------------- k_ip_inertia
def inertia_ref(F, dw, cap=INERTIA_CAP):
    """One launch of the inertia state machine on (F[0..3] = not-SPD seen, refactor, resolved,
    tries; dw = [this system's shift, the last nonzero one]).  Returns (F, dw, shift): shift is
    the value added to P (Ps = P + shift) or None when Ps stays.  fp64 on purpose: see
    test_ip_stages_gpu.py on exactness."""
    F, dw = [int(v) for v in F], [float(v) for v in dw]
    shift = None
    if F[2]:
        F[1] = 0
    elif not F[0]:
        F[2], F[1] = 1, 0
        if dw[0] > 0.0:
            dw[1] = dw[0]
    elif F[3] >= cap:
        F[0], F[1], F[2] = 0, 0, 1
    else:
        F[0] = 0
        if dw[0] == 0.0:
            nd = 1e-4 if dw[1] == 0.0 else max(1e-20, dw[1] / 3.0)
        else:
            nd = dw[0] * (100.0 if dw[1] == 0.0 else 8.0)
        dw[0] = nd
        F[1] = 1
        F[3] += 1
        shift = nd
    return F, dw, shift


def inertia_class(F, dw, cap=INERTIA_CAP):
    """The branch a launch takes (the transition table's classes)."""
    if F[2]:
        return "resolved"
    if not F[0]:
        return "clean_keep" if dw[0] > 0.0 else "clean_zero"
    if F[3] >= cap:
        return "cap"
    if dw[0] == 0.0:
        return "first_1e-4" if dw[1] == 0.0 else ("third_floor" if dw[1] / 3.0 < 1e-20 else "third")
    return "x100" if dw[1] == 0.0 else "x8"


# ---------------------------------------------------------------------------- the direction
def newton_dir(kk, data, state, st, x_for_hess=None, ev=None, pd=None):
    """dx of the reduced Newton system in fp64 as IPRef.solve computes it (lines 217-256,
    "regularized"), with the inertia correction driven through inertia_ref.  Returns
    dict(dx, jdx, dwi, tries, dw_last)."""
    J = data["J"]
    n = J.shape[1]
    dw = st["delta_w"]
    H = _f64(data["P"]) + dw
    W, rhat, rx = _f64(kk["W"]), _f64(kk["rhat"]), _f64(kk["rx"])
    lam, grad = _f64(state["lam"]), _f64(data["grad"])
    exact = st["hessian"] == "exact"
    Kb = sp.diags(H) + J.T @ sp.diags(W) @ J
    Hl = ev.lag_hess(x_for_hess, lam) if exact else sp.csr_matrix((n, n))
    Kb = (Kb + Hl).tocsc()
    F, dwv = [0, 0, 0, 0], [0.0, float(state["dw_last"])]
    if exact:
        for _ in range(st["inertia_cap"] + 1):
            F[0] = 0 if I.is_pd(Kb + dwv[0] * sp.eye(n)) else 1
            F, dwv, _ = inertia_ref(F, dwv, st["inertia_cap"])
            if F[2]:
                break
    dwi = dwv[0]
    K = (Kb + dwi * sp.eye(n)).tocsc()
    rhs = -rx - J.T @ (W * rhat)
    lu = spla.splu(K)
    dx = lu.solve(rhs)
    for _ in range(st["n_refine"]):
        res = -(grad + J.T @ (lam + W * (J @ dx + rhat))) - (H + dwi) * dx - Hl @ dx
        dx = dx + lu.solve(res)
    return dict(dx=dx, jdx=J @ dx, dwi=dwi, tries=F[3], dw_last=dwv[1])


# ---------------------------------------------------------------------------- k_ip_step
def _ftb(v, dv, tau, mask, dt):
    neg = mask & (dv < 0)
    if not np.any(neg):
        return dt(1.0), -1
    r = -tau * v / np.where(neg, dv, dt(-1.0))
    r = np.where(neg, r, dt(np.inf))
    q = int(np.argmin(r))
    return min(dt(1.0), r[q]), q


def step_ld(state, data, kk, direc, values, st, mg=None, dt=LD, it=0):
    """Directions, fraction-to-boundary, filter line search and update (IPRef.solve lines
    257-316) from the direction direc = dict(dx, jdx[, xa, za, done, ref_last, ref_solves]).
    values(x) -> (f, g) at a trial point (fp64).  Returns (out, bnd): out has status (None:
    accepted), alpha, alpha_z, trials, ftype, f, dl, ds, the new state and the trial log."""
    mg = mg or Margins()
    g, lbg, ubg = np.asarray(data["g"], dt), data["lbg"], data["ubg"]
    eq, hl, hu = _classes(lbg, ubg)
    iq = ~eq
    x, s, lam, zl, zu = (_in(state[q], dt) for q in ("x", "s", "lam", "zl", "zu"))
    mu = dt(np.float64(state["mu"]))
    grad = np.asarray(data["grad"], dt)
    W, rhat = _in(kk["W"], dt), _in(kk["rhat"], dt)
    dx, jdx = _in(direc["dx"], dt).copy(), _in(direc["jdx"], dt).copy()
    ref_solves = int(direc.get("ref_solves", 0))
    cjd = 2
    if "xa" in direc:  # the pending correction of the last refinement sweep (k_ip_step's first block)
        pending = not direc.get("done", 1)
        xa, za = np.asarray(direc["xa"], dt), np.asarray(direc["za"], dt)
        app = True
        if pending and st["n_refine"] >= 2:
            app = mg.cmp("step |xa| <= ref_last", np.max(np.abs(xa)), "<=", dt(direc["ref_last"]))
        mg.tag("step_pending_applied" if (pending and app) else "step_pending_grew" if pending else "step_no_pending")
        if pending and app:
            ref_solves += 1
        if app:
            dx, jdx = dx + xa, jdx + za                                          # c = 1
            cjd = 3
    else:
        mg.tag("step_no_pending")
    lb, ub, sl, su = _slacks(s, lbg, ubg, hl, hu, dt)
    e = LD(EPS64)
    with np.errstate(all="ignore"):
        sig = np.where(hl, zl / sl, dt(0.0)) + np.where(hu, zu / su, dt(0.0))
        sig_safe = np.where(iq, sig, dt(1.0))
        bs = np.where(iq, lam + np.where(hl, mu / sl, dt(0.0)) - np.where(hu, mu / su, dt(0.0)), dt(0.0))
        dl = W * (jdx + rhat)                                                    # c = 2 (3 with xa)
        ds = np.where(iq, (bs + dl) / sig_safe, dt(0.0))                         # c = 12 with sig, bs
        dzl = np.where(hl, mu / sl - zl - zl / sl * ds, dt(0.0))                 # c = 8
        dzu = np.where(hu, mu / su - zu + zu / su * ds, dt(0.0))
        b_dl = cjd * e * np.abs(W) * (np.abs(jdx) + np.abs(rhat))
        mag_bs = np.abs(lam) + np.where(hl, mu / sl, 0) + np.where(hu, mu / su, 0)
        b_ds = np.where(iq, (12 * e * (mag_bs + np.abs(dl)) + b_dl) / sig_safe, LD(0))
        b_dzl = np.where(hl, 8 * e * (mu / sl + zl + zl / sl * np.abs(ds)) + zl / sl * b_ds, LD(0))
        b_dzu = np.where(hu, 8 * e * (mu / su + zu + zu / su * np.abs(ds)) + zu / su * b_ds, LD(0))
    out = dict(dl=dl, ds=ds, ref_solves=ref_solves, status=None, trials=0, alpha=dt(0.0), alpha_z=dt(0.0), log=[])
    bnd = dict(dl=_f64(b_dl), ds=_f64(b_ds))
    if not (np.all(np.isfinite(dx)) and np.all(np.isfinite(dl)) and np.all(np.isfinite(ds))):
        out["status"] = I.ST_NONFINITE
        mg.tag("step_nonfinite")
        return out, bnd
    tau = max(dt(I.TAU_MIN), dt(1.0) - mu)

    def bound(v, dv, b_dv, mask, sign=1):
        a, q = _ftb(v, sign * dv, tau, mask, dt)
        if q < 0 or a >= 1:
            return a, q, LD(0)
        return a, q, a * (4 * e + b_dv[q] / abs(dv[q]))                          # c = 4 + the direction's bound

    al, ql, b_al = bound(sl, ds, b_ds, hl)
    au, qu, b_au = bound(su, ds, b_ds, hu, -1)
    amax, b_amax = (al, b_al) if al <= au else (au, b_au)
    if amax < 1:
        mg.tag("step_amax_lower" if al <= au else "step_amax_upper")
    azl, _, b_azl = bound(zl, dzl, b_dzl, hl)
    azu, _, b_azu = bound(zu, dzu, b_dzu, hu)
    az, b_az = (azl, b_azl) if azl <= azu else (azu, b_azu)
    if az < 1:
        mg.tag("step_az_bound")
    m = g.size
    c = _c(g, s, lbg, eq, dt)
    theta = dt(np.sum(np.abs(c)))
    f0 = dt(data["f"])
    lsum = np.sum(np.log(sl[hl])) + np.sum(np.log(su[hu]))
    phi = f0 - mu * lsum
    dphi = dt(grad @ dx + np.sum(np.where(hl, -mu / sl, dt(0.0)) * ds + np.where(hu, mu / su, dt(0.0)) * ds))
    gmax = float(np.max(np.abs(g)))
    b_theta = ROW_BAR * gmax * m + (m + 2) * e * np.sum(np.abs(g) + np.abs(s))
    nlog = int(hl.sum() + hu.sum())
    b_phi = ROW_BAR * max(1.0, abs(float(f0))) + mu * (3 * nlog + 2) * e * (np.sum(np.abs(np.log(sl[hl]))) +
                                                                         np.sum(np.abs(np.log(su[hu]))) + nlog)
    theta_max, theta_min = dt(np.float64(state["theta_max"])), dt(np.float64(state["theta_min"]))
    filt = [(dt(np.float64(tf)), dt(np.float64(pf))) for tf, pf in state["filt"]]
    accepted, ftype, a, t = False, False, amax, 0
    for t in range(st["ls_max"]):
        a = amax * dt(0.5) ** t
        xt = x + a * dx
        stt = s + a * ds
        ft, gt = values(_f64(xt))
        ft, gt = dt(ft), np.asarray(gt, dt)
        slt = np.where(hl, stt - lb, dt(1.0))
        sut = np.where(hu, ub - stt, dt(1.0))
        with np.errstate(all="ignore"):
            th_t = dt(np.sum(np.abs(_c(gt, stt, lbg, eq, dt))))
            ph_t = ft - mu * (np.sum(np.log(slt[hl])) + np.sum(np.log(sut[hu])))
        out["log"].append(dict(a=a, theta=th_t, phi=ph_t, f=ft))
        if not (np.isfinite(th_t) and np.isfinite(ph_t)):
            mg.tag("trial_nonfinite")
            continue
        if mg.cmp(f"trial {t} theta > theta_max", th_t, ">", theta_max):
            mg.tag("trial_theta_max")
            continue
        dominated = False
        for q, (tf, pf) in enumerate(filt):
            d1, d2 = mg.dist(th_t, tf), mg.dist(ph_t, pf)
            a1, a2 = th_t >= dt(tf), ph_t >= dt(pf)
            dom = bool(a1 and a2)
            mg.note(f"trial {t} filter entry {q}", min(d1, d2) if dom else max(d for d, v in ((d1, a1), (d2, a2)) if not v), dom)
            if dom:
                dominated = True
                break
        if dominated:
            mg.tag("trial_filter_rejected")
            continue
        sw = False
        if dphi < 0:
            sw = mg.cmp(f"trial {t} switching", a * (-dphi) ** dt(I.S_PHI), ">", dt(I.DELTA) * theta ** dt(I.S_THETA))
        small = mg.cmp("theta <= theta_min", theta, "<=", theta_min)
        if small and sw:
            if mg.cmp(f"trial {t} armijo", ph_t, "<=", phi + dt(I.ETA_PHI) * a * dphi):
                accepted, ftype = True, True
                mg.tag("accept_ftype")
                break
            mg.tag("trial_armijo_failed")
        else:
            d1, d2 = mg.dist(th_t, (1 - dt(I.GAMMA_THETA)) * theta), mg.dist(ph_t, phi - dt(I.GAMMA_PHI) * theta)
            a1 = th_t <= (1 - dt(I.GAMMA_THETA)) * theta
            a2 = ph_t <= phi - dt(I.GAMMA_PHI) * theta
            ok = bool(a1 or a2)
            mg.note(f"trial {t} sufficient decrease", max(d for d, v in ((d1, a1), (d2, a2)) if v) if ok else min(d1, d2), ok)
            if ok:
                accepted = True
                mg.tag("accept_htype_theta" if a1 else "accept_htype_phi")
                break
            mg.tag("trial_htype_failed")
    out["trials"] = t + 1
    out.update(theta=theta, phi=phi, dphi=dphi, amax=amax, az=az)
    bnd.update(theta=float(b_theta), phi=float(b_phi), alpha=float(b_amax), alpha_z=float(b_az))
    if not accepted:
        out["status"] = I.ST_LS_FAIL
        mg.tag("step_ls_fail")
        return out, bnd
    if t > 0:
        mg.tag("accept_after_backtrack")
    new = dict(state)
    if not ftype:
        if len(filt) < MAXFILT:
            filt.append(((1 - dt(I.GAMMA_THETA)) * theta, phi - dt(I.GAMMA_PHI) * theta))
            mg.tag("filter_append")
        else:
            mg.tag("filter_full")
    xn = x + a * dx                                                              # c = 2
    sn = s + a * ds
    lamn = lam + a * dl
    zln = zl + az * dzl
    zun = zu + az * dzu
    b_a = b_amax * float(dt(0.5) ** t)
    b_x = 2 * e * (np.abs(x) + np.abs(a * dx)) + b_a * np.abs(dx)
    b_s = np.where(iq, 2 * e * (np.abs(s) + np.abs(a * ds)) + b_a * np.abs(ds) + a * b_ds, LD(0))
    b_lam = 2 * e * (np.abs(lam) + np.abs(a * dl)) + b_a * np.abs(dl) + a * b_dl
    b_zl = 2 * e * (np.abs(zl) + np.abs(az * dzl)) + b_az * np.abs(dzl) + az * b_dzl
    b_zu = 2 * e * (np.abs(zu) + np.abs(az * dzu)) + b_az * np.abs(dzu) + az * b_dzu
    _, _, sln, sun = _slacks(sn, lbg, ubg, hl, hu, dt)
    KS = dt(I.KAPPA_SIGMA)
    with np.errstate(all="ignore"):
        lo_l, hi_l = mu / (KS * sln), KS * mu / sln                              # c = 3 on the cancelling sn - l
        lo_u, hi_u = mu / (KS * sun), KS * mu / sun
        for nm, z, lo, hi, mask in (("zl", zln, lo_l, hi_l, hl), ("zu", zun, lo_u, hi_u, hu)):
            if np.any(mask & (z < lo)):
                mg.tag(f"clamp_{nm}_low")
            if np.any(mask & (z > hi)):
                mg.tag(f"clamp_{nm}_high")
            for r in direc.get("clamp_rows", ()):  # the rows a case is built around
                if mask[r]:
                    mg.cmp(f"clamp {nm}[{r}] low", z[r], "<", lo[r])
                    mg.cmp(f"clamp {nm}[{r}] high", z[r], ">", hi[r])
        czl = np.where(hl, np.clip(zln, lo_l, hi_l), dt(0.0))
        czu = np.where(hu, np.clip(zun, lo_u, hi_u), dt(0.0))
        b_zl = np.where(czl != zln, np.abs(czl) * (3 * e + (b_s + e * np.abs(sn)) / np.abs(sln)), b_zl)
        b_zu = np.where(czu != zun, np.abs(czu) * (3 * e + (b_s + e * np.abs(sn)) / np.abs(sun)), b_zu)
    new.update(x=xn, s=np.where(iq, sn, dt(0.0)), lam=lamn, zl=czl, zu=czu, filt=filt)
    ft = out["log"][-1]["f"]
    out.update(alpha=a, alpha_z=az, ftype=ftype, f=ft, state=new)
    bnd.update(alpha=float(b_a), x=_f64(b_x), s=_f64(b_s), lam=_f64(b_lam), zl=_f64(np.where(hl, b_zl, 0)),
               zu=_f64(np.where(hu, b_zu, 0)),
               f=float(ROW_BAR * max(1.0, abs(float(ft))) + 2 * np.sum(np.abs(grad) * b_x)),
               filt=(float((1 + e) * b_theta), float(b_phi + I.GAMMA_PHI * b_theta)))
    return out, bnd


# ---------------------------------------------------------------------------- the chain
def chain(ev, x0, st, lam0=None, dt=LD, mg=None, max_iter=None):
    """init, then kkt, direction (inertia inside) and step per iteration: IPRef.solve on the stage
    functions.  Returns (x, lam, info); info["states"][k] is the iterate that enters iteration k
    and info["calls"][k] what its stages returned."""
    mg = mg or Margins()
    x = np.asarray(x0, dt).copy()
    d0 = ev.data(_f64(x))
    state, _ = init_ld(d0["g"], d0["lbg"], d0["ubg"], st, lam0, dt)
    state["x"] = x
    status, it = I.ST_MAX_ITER, 0
    alphas, trials, mus, ndecs, states, calls = [], [], [], [], [], []
    err, f = np.inf, np.nan
    K = st["max_iter"] if max_iter is None else max_iter
    for k in range(K + 1):
        it = k
        data = ev.data(_f64(state["x"]))
        f = data["f"]
        states.append(dict(state))
        kk, kb = kkt_ld(state, data, k, dict(st, max_iter=K), mg, dt)
        err = kk["err"]
        ndecs.append(kk["ndec"])
        if kk["status"] is not None:
            status = kk["status"]
            calls.append(dict(data=data, kkt=kk, kkt_bnd=kb))
            break
        if kk["ndec"]:
            state = dict(state, mu=kk["mu"], filt=[])
        mus.append(float(state["mu"]))
        nd = newton_dir(kk, data, state, st, _f64(state["x"]), ev)
        state = dict(state, dw_last=nd["dw_last"])
        so, sb = step_ld(state, data, kk, nd, ev.values, st, mg, dt, it=k)
        calls.append(dict(data=data, kkt=kk, kkt_bnd=kb, dir=nd, step=so, step_bnd=sb, step_in=state))
        trials.append(so["trials"])
        if so["status"] is not None:
            status = so["status"]
            if status == I.ST_LS_FAIL:
                alphas.append(0.0)
            break
        alphas.append(float(so["alpha"]))
        state = so["state"]
    return _f64(state["x"]), _f64(state["lam"]), dict(
        status=status, iter=it, err=float(err), mu=float(state["mu"]), f=float(f), alphas=np.array(alphas),
        trials=np.array(trials, dtype=int), mus=mus, ndecs=ndecs, states=states, calls=calls, state=state, margins=mg)


# ---------------------------------------------------------------------------- crafted cases
# The problems of the CPU pin test (tag, N, synthetic problem) and its second settings: with
# mu_init = 1e-1, tol = 1e-6 problem PIN_PROBLEMS[0] takes two barrier decreases in one k_ip_kkt
# call (0.1 -> 0.02 -> 0.0028 at iteration 8); PIN_PROBLEMS[1] takes an inertia shift there.
PIN_PROBLEMS = (("cv24", 2, 1), ("rnea36", 2, 0))
PIN_SETTINGS = ({}, dict(mu_init=1e-1, tol=1e-6))

INIT_KINDS = ("eq", "lo_in", "lo_on", "lo_out", "up_in", "up_out", "two_wide_in", "two_narrow_out", "two_narrow_in",
              "lo_big_on", "two_big_out", "up_on")
INIT_LAM0 = (3.0, -2.0, 5e-8, -5e-8, 0.0, 1e-3, -1e-7 * 1.5)  # both signs, either side of warm_push = 1e-7


def init_case(m, seed=5):
    """g, lbg, ubg, lam0 of m rows cycling through INIT_KINDS (period 12) against INIT_LAM0 (period
    7): every row kind meets every multiplier class within 84 rows."""
    rng = np.random.default_rng(seed)
    g, l, u = np.zeros(m), np.zeros(m), np.zeros(m)
    inf = np.inf
    for r in range(m):
        kind = INIT_KINDS[r % len(INIT_KINDS)]
        j = 0.1 * rng.random()
        l[r], u[r], g[r] = {
            "eq": (0.3 + j, 0.3 + j, rng.normal()),
            "lo_in": (-0.5 - j, inf, 0.7), "lo_on": (-0.5 - j, inf, -0.5 - j), "lo_out": (-0.5 - j, inf, -0.9 - j),
            "up_in": (-inf, 0.8 + j, 0.1), "up_out": (-inf, 0.8 + j, 1.1 + j), "up_on": (-inf, 0.8 + j, 0.8 + j),
            "two_wide_in": (-1.0 - j, 2.0, 0.5), "two_narrow_out": (0.25 + j, 0.25 + j + 1e-6, 0.1),
            "two_narrow_in": (0.25 + j, 0.25 + j + 1e-6, 0.25 + j + 5e-7),
            "lo_big_on": (-250.0 - j, inf, -250.0 - j), "two_big_out": (-300.0, 400.0 + j, 401.0 + j)}[kind]
    lam0 = np.array([INIT_LAM0[r % len(INIT_LAM0)] for r in range(m)]) * (1.0 + 0.01 * rng.random(m))
    return g, l, u, lam0


def _near_converged(state, data, base, comp, mu):
    """A crafted KKT input near a solution: the inequality rows' g on their slacks, one equality
    row off by ``base`` (max |c| = base), the gradient balancing J^T lam up to 1e-3 base, lam
    balancing the bound multipliers, every complementarity product = comp."""
    eq, hl, hu = _classes(data["lbg"], data["ubg"])
    lbg, ubg = data["lbg"], data["ubg"]
    with np.errstate(all="ignore"):  # slacks well inside, so that the multipliers stay of comp's order (sd = sc = 1)
        s = np.where(hl & hu, 0.5 * (lbg + ubg), np.where(hl, lbg + 1.0, np.where(hu, ubg - 1.0, 0.0)))
    lb, ub, sl, su = _slacks(s, lbg, ubg, hl, hu, np.float64)
    zl = np.where(hl, comp / sl, 0.0)
    zu = np.where(hu, comp / su, 0.0)
    lam = np.where(eq, _f64(state["lam"]), zu - zl)
    g = np.where(eq, data["lbg"], s)
    r0 = int(np.flatnonzero(eq)[3])
    g[r0] += base
    rng = np.random.default_rng(3)
    grad = -(data["J"].T @ lam) + 1e-3 * base * rng.uniform(-1, 1, data["J"].shape[1])
    return dict(state, s=s, lam=lam, zl=zl, zu=zu, mu=mu), dict(data, g=g, grad=grad)


def kkt_cases(state, data, st):
    """(name, state, data, k, settings, expected tags) from a chain iterate."""
    out = [("continue", state, data, 1, st, {"kkt_continue"}),
           ("max_iter", state, data, st["max_iter"], st, {"kkt_max_iter"})]
    kk, _ = kkt_ld(state, data, 1, st)
    tol_c = float(10.0 ** np.ceil(np.log10(float(kk["err"]) * 3)))
    out.append(("converged", state, data, 1, dict(st, tol=tol_c), {"kkt_converged"}))
    lam = _f64(state["lam"]).copy()
    lam[lam.size // 2] = np.nan
    out.append(("nonfinite", dict(state, lam=lam), data, 1, st, {"kkt_nonfinite"}))
    big = dict(state, lam=_f64(state["lam"]) * 1e5 + 1e3, zl=_f64(state["zl"]) * 1e9, zu=_f64(state["zu"]) * 1e9)
    out.append(("big_multipliers", big, data, 1, st, {"kkt_sd_gt_1", "kkt_sc_gt_1", "kkt_continue"}))
    eq, hl, hu = _classes(data["lbg"], data["ubg"])
    zl = _f64(state["zl"]).copy()
    zl[int(np.flatnonzero(hl & ~hu)[0])] = 1e-30
    out.append(("w_min", dict(state, zl=zl), data, 1, st, {"kkt_w_min"}))
    tight = dict(st, tol=1e-9)
    # (E_mu of mu_0_error and mu_1 sits 25 % above and 20 % below kappa_eps mu = 1: the constant itself is seen)
    for name, base, comp, mu, stt, tags in (
            ("mu_0_error", 1.25, 1e-4, 1e-1, tight, {"mu_decreases_0", "mu_break_error"}),
            ("mu_1", 0.8, 1e-4, 1e-1, tight, {"mu_decreases_1", "mu_break_error"}),
            ("mu_2", 0.1, 1e-4, 1e-1, tight, {"mu_decreases_2", "mu_break_error"}),
            ("mu_4", 1e-5, 1e-4, 1e-1, tight, {"mu_decreases_4", "mu_four_decreases"}),
            ("mu_fixed", 1e-5, 1.05e-3, 1e-3 / 10.0, dict(st, tol=1e-3), {"mu_decreases_0", "mu_break_fixed"}),
            ("mu_to_floor", 1e-5, 2.1e-3, 1e-3, dict(st, tol=2e-3), {"mu_decreases_1", "mu_break_fixed"})):
        s2, d2 = _near_converged(state, data, base, comp, mu)
        s2["filt"] = [(1.0, 2.0), (3.0, 4.0)]  # an uploaded filter: reset exactly when mu changes
        out.append((name, s2, d2, 1, stt, tags))
    return out


def _trial_log(state, data, kk, direc, values, st):
    """(theta_t, phi_t, a_t) of every trial, none accepted: a filter entry that dominates all."""
    so, _ = step_ld(dict(state, filt=[(-1.0, -np.inf)]), data, kk, direc, values, st)
    return so


def step_cases(state, data, kk, nd, values, st):
    """(name, state, data, kkt, direction, settings, expected tags) from a chain iterate and the
    reference's own direction (dx, J dx; xa = za = 0, done = 1)."""
    base = dict(dx=_f64(nd["dx"]), jdx=_f64(nd["jdx"]))
    rev = dict(dx=-base["dx"], jdx=-base["jdx"])
    eq, hl, hu = _classes(data["lbg"], data["ubg"])
    n = base["dx"].size
    out = [("natural", state, data, kk, base, st, set())]
    lg = _trial_log(state, data, kk, base, values, st)
    th = [float(t["theta"]) for t in lg["log"]]
    ph = [float(t["phi"]) for t in lg["log"]]
    a = [float(t["a"]) for t in lg["log"]]
    # 3: f-type.  theta_min is raised above theta and the uploaded dx gets a multiple of the
    # steepest-descent direction: dx' = dx - t grad with t = k t* / alpha_max, t* = |grad|^2 /
    # grad^T P grad the minimiser of the (quadratic) objective along -grad.  dphi = dphi - t |grad|^2
    # is then large and negative (the switching condition holds), the full step overshoots the
    # minimiser k-fold, so Armijo fails there, and a shorter step passes it.  The first k that
    # does this in the reference with every margin kept is taken
    phi0, theta0 = float(lg["phi"]), float(lg["theta"])
    gr, Pd = _f64(data["grad"]), _f64(data["P"])
    tstar = float(gr @ gr) / float(gr @ (Pd * gr))
    for kf in (4.0, 8.0, 3.0, 16.0):
        d3 = dict(dx=base["dx"] - (kf * tstar / float(lg["amax"])) * gr, jdx=base["jdx"])
        s3 = dict(state, theta_min=10.0 * theta0 + 1.0)
        mg3 = Margins()
        step_ld(s3, data, kk, d3, values, st, mg3)
        if {"accept_ftype", "trial_armijo_failed"} <= mg3.tags and mg3.ok():
            out.append(("ftype_armijo", s3, data, kk, d3, st, {"accept_ftype", "trial_armijo_failed"}))
            break
    # 4: a filter entry between trial 0 and trial 1
    if th[0] > th[1]:
        ent = (0.5 * (th[0] + th[1]), min(ph) - 1.0 - abs(min(ph)))
    else:
        ent = (-1.0, 0.5 * (ph[0] + ph[1]))
    if th[0] != th[1] and (th[0] > th[1] or ph[0] > ph[1]):
        out.append(("filter_trial0", dict(state, filt=[ent]), data, kk, base, st, {"trial_filter_rejected"}))
    # 5: theta_max between two trials' theta (the reversed direction where the full step lowers theta)
    d5, th5 = (base, th) if th[0] > th[1] else (rev, [float(t["theta"]) for t in _trial_log(state, data, kk, rev, values, st)["log"]])
    if th5[0] > th5[1]:
        out.append(("theta_max", dict(state, theta_max=0.5 * (th5[0] + th5[1])), data, kk, d5, st, {"trial_theta_max"}))
    # 6: every trial rejected
    out.append(("all_rejected", dict(state, filt=[(-1.0, min(ph) - 1.0 - abs(min(ph)))]), data, kk, base,
                dict(st, ls_max=5), {"step_ls_fail", "trial_filter_rejected"}))
    # 7: a full filter of entries nothing reaches
    out.append(("filter_full", dict(state, filt=[(1e300, 1e300 - q) for q in range(MAXFILT)]), data, kk, base, st, set()))
    # 8: a NaN in the direction
    bad = base["dx"].copy()
    bad[n // 3] = np.nan
    out.append(("nan_direction", state, data, kk, dict(dx=bad, jdx=base["jdx"]), st, {"step_nonfinite"}))
    # pending correction: ref_last on either side of |xa|_inf
    rng = np.random.default_rng(9)
    xa = 1e-3 * np.max(np.abs(base["dx"])) * rng.uniform(-1, 1, n)
    za = data["J"] @ xa
    for name, fac, tag in (("pending_applied", 2.0, "step_pending_applied"), ("pending_grew", 0.5, "step_pending_grew")):
        out.append((name, state, data, kk, dict(base, xa=xa, za=za, done=0, ref_last=fac * float(np.max(np.abs(xa))),
                                                ref_solves=4), st, {tag}))
    # 9: alpha_max bound by a lower slack (the upper slacks and alpha_z bind in the chain's own steps
    # and in the clamp case): a lower-only row with zl = 1, W = 1e-20 (dl ~ 0) and lam so negative
    # that ds = (lam + mu / sl + dl) sl / zl < 0 with tau sl / |ds| = tau zl / |lam + ...| a tenth of
    # the step bound the other rows give
    r9 = int(np.flatnonzero(hl & ~hu)[-1])
    lam9, zl9, W9 = _f64(state["lam"]).copy(), _f64(state["zl"]).copy(), _f64(kk["W"]).copy()
    sl9 = float(_f64(state["s"])[r9] - data["lbg"][r9])
    zl9[r9], W9[r9] = 1.0, 1e-20
    lam9[r9] = -(10.0 / float(lg["amax"]) + 2.0 * float(state["mu"]) / sl9)
    out.append(("amax_lower", dict(state, lam=lam9, zl=zl9), data, dict(kk, W=W9), base, st, {"step_amax_lower"}))
    # 10: both sides of the kappa_sigma clamp for zl and zu, at mu = 1e-10 (tau = 1 - 1e-10).
    # Row q (lower only: slack 2^-50, zl = 1e-8, lam = 1e5, W = 1e-20 so that dl ~ 0) has
    # dz = -(z + lam + dl) and bounds alpha_z at ~1e-13 while its own ds = lam sl / z + mu / z stays
    # ~2e-2.  Two two-sided rows at mid-interval carry zl (zu) = 1e-40: z + alpha_z mu / slack ~
    # 1e-23 / slack stays below the lower clamp mu / (1e10 slack) = 1e-20 / slack.  Two more carry
    # zl (zu) = 1e12, above the upper clamp 1e10 mu / slack = 1 / slack, and barely move
    lo_only = np.flatnonzero(hl & ~hu)
    two = np.flatnonzero(hl & hu)
    q, p1, p2, h1, h2 = int(lo_only[0]), int(two[0]), int(two[1]), int(two[2]), int(two[3])
    s, lam, zl, zu = (_f64(state[k]).copy() for k in ("s", "lam", "zl", "zu"))
    W = _f64(kk["W"]).copy()
    s[q] = data["lbg"][q] + 2.0 ** -50
    zl[q], lam[q], W[q] = 1e-8, 1e5, 1e-20
    for r in (p1, p2):
        s[r] = 0.5 * (data["lbg"][r] + data["ubg"][r])
    zl[p1], zu[p2], zl[h1], zu[h2] = 1e-40, 1e-40, 1e12, 1e12
    out.append(("clamps", dict(state, s=s, lam=lam, zl=zl, zu=zu, mu=1e-10), data, dict(kk, W=W),
                dict(base, clamp_rows=(p1, p2, h1, h2)), st,
                {"clamp_zl_low", "clamp_zl_high", "clamp_zu_low", "clamp_zu_high", "step_az_bound"}))
    return out


STEP_BRANCHES = {"accept_htype_theta", "accept_htype_phi", "accept_ftype", "trial_armijo_failed", "trial_filter_rejected",
                 "accept_after_backtrack", "trial_theta_max", "step_ls_fail", "filter_full", "filter_append",
                 "step_nonfinite", "step_amax_lower", "step_amax_upper", "step_az_bound", "clamp_zl_low",
                 "clamp_zl_high", "clamp_zu_low", "clamp_zu_high", "step_pending_applied", "step_pending_grew",
                 "step_no_pending"}
KKT_BRANCHES = {"kkt_continue", "kkt_converged", "kkt_max_iter", "kkt_nonfinite", "kkt_sd_gt_1", "kkt_sc_gt_1",
                "kkt_w_min", "mu_break_error", "mu_break_fixed", "mu_four_decreases", "mu_decreases_0",
                "mu_decreases_1", "mu_decreases_2", "mu_decreases_4"}
INERTIA_CLASSES = ("resolved", "clean_zero", "clean_keep", "cap", "first_1e-4", "third", "third_floor", "x100", "x8")


def inertia_table(cap=INERTIA_CAP):
    """Every reachable (F, dw) class as a start state [(F, dw)]: each is stepped by single launches
    until it resolves (with the factor flag F[0] re-raised after every shift, as a factor that
    keeps failing does), so the walk passes x100 / x8 growth and the cap."""
    starts = []
    for F0 in (0, 1):
        for dw0 in (0.0, 1e-4, 0.37):
            for dw1 in (0.0, 3e-3, 2.4e-20):
                for tries in (0, 3, cap - 1, cap):
                    for res in (0, 1):
                        starts.append(([F0, F0, res, tries], [dw0, dw1]))
    return starts


def case_set(ev, x0, st, iters=None, crafted_at=1):
    """One problem's cases with the reference's answers: the long-double chain over ``iters``
    iterations (every iteration is a teacher-forced KKT and STEP case) and the crafted KKT and
    STEP cases built on the iterate that enters iteration ``crafted_at``."""
    _, _, info = chain(ev, x0, st, dt=LD, max_iter=iters)
    call = info["calls"][crafted_at]
    kkt, step = [], []
    for name, s2, d2, k, st2, expect in kkt_cases(info["states"][crafted_at], call["data"], st):
        mg = Margins()
        out, bnd = kkt_ld(s2, d2, k, st2, mg)
        kkt.append(dict(name=name, state=s2, data=d2, k=k, st=st2, expect=expect, out=out, bnd=bnd, margins=mg))
    for name, s2, d2, kk2, dir2, st2, expect in step_cases(call["step_in"], call["data"], call["kkt"], call["dir"],
                                                           ev.values, st):
        mg = Margins()
        out, bnd = step_ld(s2, d2, kk2, dir2, ev.values, st2, mg, it=crafted_at)
        if name == "clamps" and out["status"] is not None:  # the clamps need an accepted step
            expect = {"step_ls_fail"}
        step.append(dict(name=name, state=s2, data=d2, kkt=kk2, dir=dir2, st=st2, expect=expect, out=out, bnd=bnd,
                         margins=mg))
    return dict(chain=info, kkt=kkt, step=step, values=ev.values)
