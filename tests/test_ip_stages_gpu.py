"""The interior-point kernels of k_ip.hip one by one on the MI355X against the long-double
reference of tests/ip_stage_ref.py: k_ip_init, k_ip_kkt, k_ip_inertia and k_ip_step (with the
line search and the update), each launched alone by debug_ip_stage on uploaded buffers.

Problems: stage_ref.make_problem / make_handle, B = 3, solver "fatrop", cv24 and rnea36 at N = 2
and 3, aba36 and rnea48 (m > 256: the rows wrap the 256-thread stride) at N = 2, accnb at N = 3:
the smallest horizons with a first, an interior and a last node, four k_ip_step<DYN> variants (CV,
RNEA, ABA, ACCNB).

Inputs.  Per problem a long-double reference chain (ip_stage_ref.chain, Gauss-Newton direction by
a sparse LU) whose gradient, Jacobian and rows at each iterate come from the library's own
evaluation kernels, read back (DeviceEval): every chain iteration is a teacher-forced KKT and STEP
case, and the crafted cases of ip_stage_ref.kkt_cases / step_cases are built on the iterate that
enters iteration 1.  One (case, problem) runs at a time: the other problems of the batch are
uploaded inactive.  Row and objective values at the trial points of the reference come from the
numpy oracle in fp64.

Bars (ip_stage_ref's ``bnd``, derived there, none fitted to the device): an output passes when
|gpu - ref| <= bound elementwise; a bound of zero means bit equality.  Decisions, counts,
statuses, flags, the zeroed and the untouched buffers are exact.  Every reference run must keep
its branch decisions 1e-9 away from their thresholds (asserted here too) and take the branches
its case was built for.  The worst |gpu - ref| / bound per stage and quantity goes to
ip_stage_errors.json in the directory PL_TEST_OUT names (default: test_out/).

k_ip_inertia is exact to the bit: a launch performs at most one fp64 multiplication (x 100, x 8)
or one division by 3.0 and one comparison on the shift, then one addition P + shift per column;
each is a single correctly rounded IEEE operation on both sides (the library is built without
fast-math, and no second operation stands next to any of them that a fused multiply-add could
absorb), so numpy's fp64 gives the same bits.
"""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import ip_stage_ref as ir
import stage_ref as sr
from oracle import ip_ref as I
from oracle.ocp import OracleOCP

pytestmark = pytest.mark.gpu

CASES = [("cv24", 2), ("cv24", 3), ("rnea36", 2), ("rnea36", 3), ("aba36", 2), ("accnb", 3), ("rnea48", 2)]
CHAIN_ITERS = {("cv24", 2): 6}  # teacher-forced chain iterations (default 2: the crafted cases sit on iterate 1)
# problems of the batch that carry cases (default: all three).  The numpy oracle needs 0.2 s per
# trial point of accnb (its forward dynamics), 20 x the other cases: one problem keeps its test short
NPROB = {("accnb", 3): 1}
B = sr.BATCH
POISON = 7.25  # written into every output buffer before a launch
# worst |gpu - ref| / bound over all cases on the MI355X (ip_stage_errors.json), per stage
MEASURED = {"init": 0.24, "kkt": 0.20, "step": 0.44}  # (profiles/ip_stages/ip_stage_errors.json has every quantity)

_RECORDS = {}
OUT = os.path.join(os.environ.get("PL_TEST_OUT") or os.path.join(sr.ROOT, "test_out"), "ip_stage_errors.json")


@pytest.fixture(scope="module", autouse=True)
def _write_records():
    yield
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    by_stage = {}
    for (stage, q), r in _RECORDS.items():
        by_stage[stage] = max(by_stage.get(stage, 0.0), r["ratio"])
    with open(OUT, "w") as f:
        json.dump({"worst_ratio_by_stage": by_stage,
                   "worst_by_quantity": {f"{s}.{q}": r for (s, q), r in sorted(_RECORDS.items())}}, f, indent=1)
    for c in list(_CTX.values()):
        c["bo"].close()
    _CTX.clear()


def _close(fails, stage, quantity, where, got, ref, bnd):
    """|got - ref| <= bnd elementwise (bnd 0: equal; NaN and inf must coincide)."""
    got = np.atleast_1d(np.asarray(got, np.float64))
    ref = np.atleast_1d(np.asarray(ref, sr.LD))
    bnd = np.broadcast_to(np.atleast_1d(np.asarray(bnd, np.float64)), ref.shape)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin) or not np.array_equal(got[~fin], np.asarray(ref[~fin], np.float64),
                                                                         equal_nan=True):
        fails.append(f"{where} {stage} {quantity}: non-finite pattern differs")
        return
    err = np.asarray(np.abs(np.asarray(got[fin], sr.LD) - ref[fin]), np.float64)
    b = bnd[fin]
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / b)
    worst = float(ratio.max()) if ratio.size else 0.0
    key = (stage, quantity)
    if key not in _RECORDS or worst > _RECORDS[key]["ratio"]:
        k = int(np.argmax(ratio)) if ratio.size else 0
        _RECORDS[key] = dict(ratio=worst, where=where, err=float(err[k]) if err.size else 0.0,
                             bound=float(b[k]) if b.size else 0.0)
    if not worst <= 1.0:
        k = int(np.argmax(ratio))
        fails.append(f"{where} {stage} {quantity}[{np.flatnonzero(fin)[k]}]: |gpu - ref| {err[k]:.3e} > bound {b[k]:.3e} "
                     f"(gpu {got[fin][k]!r})")


# ---------------------------------------------------------------------------- handles and references
class DeviceEval(ir.OracleEval):
    """Derivative data at a point from the library's evaluation kernels (read back); row and
    objective values at trial points from the numpy oracle, cached by the point's bits."""

    def __init__(self, bo, b, o, p, X0):
        super().__init__(o, p)
        self.bo, self.b, self.X0 = bo, b, X0
        self.rows, self.cols = bo.pattern()
        self.P = bo.debug("P", bo.batch * bo.n).reshape(bo.batch, bo.n)[b].copy()
        self._val = {}

    def values(self, x):
        key = np.asarray(x, np.float64).tobytes()
        if key not in self._val:
            self._val[key] = super().values(x)
        return self._val[key]

    def data(self, x):
        bo, b = self.bo, self.b
        X = self.X0.copy()
        X[b] = x
        bo.set_x(X)
        grad, Jv, g, lbg, ubg = bo.eval_sqp_data()
        f = bo.eval_f()
        J = sp.csr_matrix((Jv[b], (self.rows, self.cols)), shape=(bo.m, bo.n))
        return dict(g=g[b].copy(), lbg=lbg[b].copy(), ubg=ubg[b].copy(), grad=grad[b].copy(), J=J, f=float(f[b]), P=self.P)


_CTX = {}


def _ctx(tag, N):
    """The case's handle and, per problem, its evaluator and case set (built once per module)."""
    if (tag, N) not in _CTX:
        R, dyn, kw, P, X = sr.make_problem(tag, N, B)
        bo = sr.make_handle(tag, N, B)
        bo.set_solver("fatrop")
        o = OracleOCP(R, dyn, N, **kw)
        st = ir.settings(hessian="gauss_newton")
        evs = [DeviceEval(bo, b, o, P[b], X) for b in range(NPROB.get((tag, N), B))]
        nodes = bo.node_table()
        rows, cols = bo.pattern()
        cpl = []
        for nd in nodes:
            sel = (rows >= nd[3]) & (rows < nd[3] + nd[4]) & (cols >= nd[2] + nd[0])
            cpl.append(np.unique(rows[sel]))
        _CTX[(tag, N)] = dict(bo=bo, X=X, evs=evs, st=st, nodes=nodes, cpl=cpl, rows=rows, cols=cols, key=(tag, N))
    return _CTX[(tag, N)]


def _sets(c):
    """The problems' case sets with the reference's answers (built at the first KKT or STEP test)."""
    if "sets" not in c:
        c["sets"] = [ir.case_set(ev, c["X"][b], c["st"], iters=CHAIN_ITERS.get(c["key"], 2))
                     for b, ev in enumerate(c["evs"])]
    return c["sets"]


def _apply_settings(bo, st):
    bo.set_ip_settings(**{k: st[k] for k in ("max_iter", "tol", "mu_init", "bound_push", "bound_frac", "delta_w",
                                             "delta_c", "ls_max", "n_refine")}, hessian=st["hessian"])


def _put(bo, name, b, row, width):
    arr = np.zeros((bo.batch, width))
    arr[b] = np.asarray(row, np.float64)
    bo.debug_set(name, arr)


def _fill(bo, name, width, value=POISON):
    bo.debug_set(name, np.full((bo.batch, width), value))


def _get(bo, name, b, width):
    return bo.debug(name, bo.batch * width).reshape(bo.batch, width)[b]


def _info(b, **fields):
    """ipinfo records with problem b active and every other problem inactive."""
    info = {k: np.zeros(B) for k in sr_fields()}
    info["filt"] = np.zeros((B, 32, 2))
    info["alphas"] = np.zeros((B, 32))
    info["status"][:] = I.ST_MAX_ITER
    info["active"][b] = 1
    for k, v in fields.items():
        if k == "filt":
            for q, (tf, pf) in enumerate(v):
                info["filt"][b, q] = (float(tf), float(pf))
            info["nfilt"][b] = len(v)
        elif k == "alphas":
            info["alphas"][b] = v
        else:
            info[k][b] = float(v)
    return info


def sr_fields():
    from pinoloco.ocp import BatchedOCP
    return BatchedOCP.IPINFO_FIELDS


def _check_reference(fails, where, c):
    if not c["margins"].ok():
        fails.append(f"{where}: reference decision {c['margins'].worst()} within 1e-9 of its threshold")
    if not c["expect"] <= c["margins"].tags:
        fails.append(f"{where}: reference misses the branches {c['expect'] - c['margins'].tags}")


# ---------------------------------------------------------------------------- INIT
@pytest.mark.parametrize("tag,N", CASES)
def test_init_stage(tag, N):
    """Every row kind (equality, one-sided, wide, narrow enough for bound_frac to bind, |l| > 1; g
    inside, on and outside), cold at two barrier parameters and warm with multipliers of both signs
    on either side of warm_push: s, lam, zl, zu elementwise, theta_max / theta_min, the reset."""
    c = _ctx(tag, N)
    bo, m = c["bo"], c["bo"].m
    fails = []
    rows = [ir.init_case(m, 5 + b) for b in range(B)]
    for name, kw, warm in (("cold", {}, 0), ("cold_mu", dict(mu_init=1e-1, tol=1e-6), 0), ("warm", {}, 1)):
        st = ir.settings(hessian="gauss_newton", **kw)
        _apply_settings(bo, st)
        for key, k in (("g", 0), ("lbg", 1), ("ubg", 2), ("ip_lam0", 3)):
            bo.debug_set(key, np.array([r[k] for r in rows]))
        for key in ("ip_s", "ip_lam", "ip_zl", "ip_zu"):
            _fill(bo, key, m)
        junk = _info(0, mu=3.0, theta_max=1.0, theta_min=2.0, err=0.5, f=9.0, alpha=0.3, alpha_z=0.4, viol_max=1.0, iter=4,
                     status=1, trials=5, ref_solves=6, ref_last=0.1, filt=[(1.0, 2.0)], alphas=np.full(32, 0.5))
        junk["active"][:] = 0
        bo.debug_set_ipinfo(junk)
        bo.debug_set("info_done", np.ones(B))
        bo.debug_set("ip_dwi", np.full((B, 2), POISON))
        bo.debug_ip_stage("init", warm)
        ip = bo.debug_ipinfo()
        dwi = bo.debug("ip_dwi", 2 * B).reshape(B, 2)
        done = bo.debug("info_done", B)
        for b in range(B):
            g, l, u, lam0 = rows[b]
            ref, bnd = ir.init_ld(g, l, u, st, lam0 if warm else None)
            where = f"{tag} N={N} {name} problem {b}"
            for key, q in (("ip_s", "s"), ("ip_lam", "lam"), ("ip_zl", "zl"), ("ip_zu", "zu")):
                _close(fails, "init", q, where, _get(bo, key, b, m), ref[q], bnd[q])
            _close(fails, "init", "theta_max", where, ip["theta_max"][b], ref["theta_max"], bnd["theta_max"])
            _close(fails, "init", "theta_min", where, ip["theta_min"][b], ref["theta_min"], bnd["theta_min"])
            exact = dict(mu=st["mu_init"], err=np.inf, f=0.0, alpha=0.0, alpha_z=0.0, viol_max=0.0, iter=0,
                         status=I.ST_MAX_ITER, nfilt=0, trials=0, ref_solves=0, active=1)
            for k, v in exact.items():
                if ip[k][b] != v:
                    fails.append(f"{where}: ipinfo.{k} = {ip[k][b]} after init, expected {v}")
            if np.any(ip["alphas"][b] != 0) or done[b] != 0 or dwi[b, 1] != 0.0 or dwi[b, 0] != POISON:
                fails.append(f"{where}: alphas / done / the last inertia shift are not reset (or dwi[0] was touched)")
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------------------- KKT
def _kkt_run(c, b, case, where, fails):
    bo, st = c["bo"], case["st"]
    n, m, nnz = bo.n, bo.m, bo.nnz
    state, data, k = case["state"], case["data"], case["k"]
    _apply_settings(bo, st)
    Av = np.asarray(data["J"][c["rows"], c["cols"]]).ravel()
    work = np.zeros(8)
    work[0] = data["f"]
    for key, row, w in (("g", data["g"], m), ("lbg", data["lbg"], m), ("ubg", data["ubg"], m), ("grad", data["grad"], n),
                        ("Araw", Av, nnz), ("P", data["P"], n), ("work", work, 8), ("ip_s", state["s"], m),
                        ("ip_lam", state["lam"], m), ("ip_zl", state["zl"], m), ("ip_zu", state["zu"], m)):
        _put(bo, key, b, row, w)
    outs = (("rho", m), ("ip_rh", m), ("za", m), ("ya", m), ("ls", m), ("us", m), ("qs", n), ("Ps", n), ("xa", n),
            ("ip_dx", n), ("ip_jdx", m), ("As", nnz))
    for key, w in outs:
        _fill(bo, key, w)
    ncm = max(int(c["nodes"][:, 11].max()), 1)
    _fill(bo, "rhoc", len(c["nodes"]) * ncm)
    bo.debug_set("ip_dwi", np.full((B, 2), POISON))
    bo.debug_set("ip_iflag", np.full((B, 4), 3.0))
    bo.debug_set("info_done", np.zeros(B))
    bo.debug_set_ipinfo(_info(b, mu=state["mu"], theta_max=state["theta_max"], theta_min=state["theta_min"],
                              filt=state["filt"], iter=31, trials=2))
    bo.debug_ip_stage("kkt", k)
    ref, bnd = case["out"], case["bnd"]
    ip = bo.debug_ipinfo()
    done = bo.debug("info_done", B)
    got = {key: _get(bo, key, b, w) for key, w in outs}
    go = ref["status"] is None
    exp = dict(iter=k, status=I.ST_MAX_ITER if go else ref["status"], active=1 if go else 0, trials=2,
               nfilt=0 if ref["ndec"] else len(state["filt"]), f=data["f"])
    for key, v in exp.items():
        if ip[key][b] != v:
            fails.append(f"{where}: ipinfo.{key} = {ip[key][b]}, expected {v}")
    if done[b] != (0 if go else 1):
        fails.append(f"{where}: done = {done[b]}")
    if not ref["ndec"] and len(state["filt"]) and not np.array_equal(
            ip["filt"][b, :len(state["filt"])], np.array([[float(t), float(p)] for t, p in state["filt"]])):
        fails.append(f"{where}: the filter changed without a barrier update")
    if ref["status"] != I.ST_NONFINITE:  # there the oracle's err is NaN; the kernel's max-reductions drop a NaN
        _close(fails, "kkt", "err", where, ip["err"][b], ref["err"], bnd["err"])  # and it reports the rest (status -3 holds)
    _close(fails, "kkt", "viol_max", where, ip["viol_max"][b], ref["viol_max"], bnd["viol_max"])
    _close(fails, "kkt", "mu", where, ip["mu"][b], ref["mu"], bnd["mu"])
    dwi = bo.debug("ip_dwi", 2 * B).reshape(B, 2)[b]
    flag = bo.debug("ip_iflag", 4 * B).reshape(B, 4)[b]
    rhoc = bo.debug("rhoc", B * len(c["nodes"]) * ncm).reshape(B, len(c["nodes"]), ncm)[b]
    if not go:  # a terminated problem writes nothing
        if any(np.any(v != POISON) for v in got.values()) or dwi[0] != POISON or np.any(flag != 3) or np.any(rhoc != POISON):
            fails.append(f"{where}: a terminated problem wrote the Newton system")
        return
    _close(fails, "kkt", "rho", where, got["rho"], ref["W"], bnd["W"])
    _close(fails, "kkt", "ip_rh", where, got["ip_rh"], ref["rhat"], bnd["rhat"])
    _close(fails, "kkt", "qs", where, got["qs"], ref["qs"], bnd["qs"])
    same = (("za = -ip_rh", got["za"], -got["ip_rh"]), ("ya", got["ya"], 0.0), ("ls", got["ls"], -1e30),
            ("us", got["us"], 1e30), ("Ps = P", got["Ps"], np.asarray(data["P"], np.float64)), ("xa", got["xa"], 0.0),
            ("ip_dx", got["ip_dx"], 0.0), ("ip_jdx", got["ip_jdx"], 0.0), ("As = Araw", got["As"], Av),
            ("ip_dwi[0]", dwi[0], 0.0), ("ip_dwi[1]", dwi[1], POISON), ("ip_iflag", flag, 0.0))
    for nm, a, e in same:
        if not np.array_equal(np.asarray(a), np.broadcast_to(e, np.shape(a)), equal_nan=True):
            fails.append(f"{where}: {nm} is not exact")
    for i, cr in enumerate(c["cpl"]):
        assert cr.size == c["nodes"][i][11], (where, i, "coupling rows of the pattern against the node table")
        if not np.array_equal(rhoc[i, :cr.size], got["rho"][cr]):
            fails.append(f"{where} node {i}: rhoc is not rho of the coupling rows")
    if "kkt_w_min" in case["expect"] and not np.any(got["rho"] == I.W_MIN):
        fails.append(f"{where}: no row sits at W_MIN")


def _chain_cases(cs, kind):
    """The chain's iterations as teacher-forced cases."""
    info, out = cs["chain"], []
    for k, call in enumerate(info["calls"]):
        mg = ir.Margins()
        if kind == "kkt":
            st = dict(info_st(cs), max_iter=len(info["calls"]) - 1)
            ref, bnd = ir.kkt_ld(info["states"][k], call["data"], k, st, mg)
            out.append(dict(name=f"chain_it{k}", state=info["states"][k], data=call["data"], k=k, st=st, expect=set(),
                            out=ref, bnd=bnd, margins=mg))
        elif "step" in call:
            ref, bnd = ir.step_ld(call["step_in"], call["data"], call["kkt"], call["dir"], cs["values"], info_st(cs), mg)
            out.append(dict(name=f"chain_it{k}", state=call["step_in"], data=call["data"], kkt=call["kkt"],
                            dir=call["dir"], st=info_st(cs), expect=set(), out=ref, bnd=bnd, margins=mg, it=k))
    return out


def info_st(cs):
    return cs["st"]


@pytest.mark.parametrize("tag,N", CASES)
def test_kkt_stage(tag, N):
    """k_ip_kkt alone: continue / converged / max_iter / non-finite, sd and sc above 1, a row at
    W_MIN, barrier updates of 0, 1, 2 and 4 decreases and both breaks with the filter reset exactly
    when mu moved; err, viol_max, status, active, mu, rho, ip_rh, za, qs, Ps, ls / us, rhoc and the
    zeroed buffers."""
    c = _ctx(tag, N)
    fails, tags = [], set()
    for b, cset in enumerate(_sets(c)):
        cs = dict(cset, st=c["st"])
        for case in _chain_cases(cs, "kkt") + cs["kkt"]:
            where = f"{tag} N={N} kkt {case['name']} problem {b}"
            _check_reference(fails, where, case)
            tags |= case["margins"].tags
            _kkt_run(c, b, case, where, fails)
    assert ir.KKT_BRANCHES <= tags, ir.KKT_BRANCHES - tags
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------------------- INERTIA
def test_inertia_stage():
    """The whole transition table by single launches, three start states per launch: flags, both
    shifts and Ps = P + shift (or Ps untouched) to the bit (module docstring: why exact)."""
    c = _ctx("cv24", 2)
    bo, n = c["bo"], c["bo"].n
    rng = np.random.default_rng(2)
    P = rng.uniform(0.1, 50.0, (B, n))
    bo.debug_set("P", P)
    starts = ir.inertia_table()
    fails, seen = [], set()
    try:
        for s0 in range(0, len(starts), B):
            grp = [starts[(s0 + j) % len(starts)] for j in range(B)]
            F = [list(g[0]) for g in grp]
            dw = [list(g[1]) for g in grp]
            Ps = np.full((B, n), POISON)
            bo.debug_set("Ps", Ps)
            info = _info(0)
            info["active"][:] = 1
            bo.debug_set_ipinfo(info)
            for launch in range(ir.INERTIA_CAP + 2):
                bo.debug_set("ip_iflag", np.array(F, float))
                bo.debug_set("ip_dwi", np.array(dw))
                bo.debug_ip_stage("inertia")
                gF = bo.debug("ip_iflag", 4 * B).reshape(B, 4)
                gdw = bo.debug("ip_dwi", 2 * B).reshape(B, 2)
                gPs = bo.debug("Ps", B * n).reshape(B, n)
                for j in range(B):
                    seen.add(ir.inertia_class(F[j], dw[j]))
                    was = (list(F[j]), list(dw[j]))
                    F[j], dw[j], shift = ir.inertia_ref(F[j], dw[j])
                    if shift is not None:
                        Ps[j] = P[j] + shift
                    if list(gF[j]) != F[j] or list(gdw[j]) != dw[j] or not np.array_equal(gPs[j], Ps[j]):
                        fails.append(f"inertia from {was}: flags {list(gF[j])} shifts {list(gdw[j])}, expected {F[j]} {dw[j]}"
                                     f" (Ps equal: {np.array_equal(gPs[j], Ps[j])})")
                    if not F[j][2]:
                        F[j][0] = 1  # the refactor fails again
                if all(f[2] for f in F):
                    break
    finally:
        bo.debug_set("P", np.array([ev.P for ev in c["evs"]]))
    assert seen == set(ir.INERTIA_CLASSES), set(ir.INERTIA_CLASSES) ^ seen
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------------------- STEP
def _step_run(c, b, case, where, fails):
    bo, st = c["bo"], case["st"]
    n, m = bo.n, bo.m
    state, data, kk, direc = case["state"], case["data"], case["kkt"], case["dir"]
    it = case.get("it", 1)
    _apply_settings(bo, st)
    X = c["X"].copy()
    X[b] = np.asarray(state["x"], np.float64)
    bo.set_x(X)
    ins = dict(ip_s=state["s"], ip_lam=state["lam"], ip_zl=state["zl"], ip_zu=state["zu"], rho=kk["W"], ip_rh=kk["rhat"],
               ip_dx=direc["dx"], ip_jdx=direc["jdx"], xa=direc.get("xa", np.zeros(n)), za=direc.get("za", np.zeros(m)))
    for key, row in ins.items():
        _put(bo, key, b, row, n if key in ("ip_dx", "xa") else m)
    for key in ("ip_dl", "ip_ds"):
        _fill(bo, key, m)
    done = np.ones(B)
    done[b] = direc.get("done", 1)
    bo.debug_set("info_done", done)
    alph = np.full(32, 0.125)
    bo.debug_set_ipinfo(_info(b, mu=state["mu"], theta_max=state["theta_max"], theta_min=state["theta_min"],
                              filt=state["filt"], iter=it, trials=3, f=-5.0, ref_solves=direc.get("ref_solves", 0),
                              ref_last=direc.get("ref_last", 0.0), alphas=alph))
    bo.debug_ip_stage("step")
    ref, bnd = case["out"], case["bnd"]
    ip = bo.debug_ipinfo()
    gdone = bo.debug("info_done", B)[b]
    gx = bo.get_x()[b]
    got = {key: _get(bo, key, b, m) for key in ("ip_s", "ip_lam", "ip_zl", "ip_zu", "ip_dl", "ip_ds")}
    f64 = lambda v: np.asarray(v, np.float64)  # noqa: E731
    nf0 = len(state["filt"])
    if ip["ref_solves"][b] != ref["ref_solves"]:
        fails.append(f"{where}: ref_solves {ip['ref_solves'][b]}, expected {ref['ref_solves']}")
    _close(fails, "step", "ip_dl", where, got["ip_dl"], ref["dl"], bnd["dl"])
    _close(fails, "step", "ip_ds", where, got["ip_ds"], ref["ds"], bnd["ds"])
    if ref["status"] is not None:  # -3: nothing but the status; -2: alpha = alphas[iter] = 0, trials
        ls = ref["status"] == I.ST_LS_FAIL
        alph_e = alph.copy()
        if ls:
            alph_e[it] = 0.0
        exp = dict(status=ref["status"], active=0, trials=3 + (ref["trials"] if ls else 0), nfilt=nf0, f=-5.0)
        if ls:
            exp["alpha"] = 0.0
        for key, v in exp.items():
            if ip[key][b] != v:
                fails.append(f"{where}: ipinfo.{key} = {ip[key][b]}, expected {v}")
        unchanged = (np.array_equal(gx, X[b]) and all(np.array_equal(got[k], f64(ins[k]), equal_nan=True)
                                                      for k in ("ip_s", "ip_lam", "ip_zl", "ip_zu")))
        if not unchanged or gdone != 1 or not np.array_equal(ip["alphas"][b], alph_e):
            fails.append(f"{where}: a failed step changed the iterate (or done / alphas are wrong)")
        return
    t = ref["trials"]
    exp = dict(status=I.ST_MAX_ITER, active=1, trials=3 + t, nfilt=len(ref["state"]["filt"]), iter=it)
    for key, v in exp.items():
        if ip[key][b] != v:
            fails.append(f"{where}: ipinfo.{key} = {ip[key][b]}, expected {v}")
    if gdone != 0 or ip["alphas"][b, it] != ip["alpha"][b] or np.any(np.delete(ip["alphas"][b], it) != 0.125):
        fails.append(f"{where}: done / alphas[iter] after an accepted step")
    _close(fails, "step", "alpha", where, ip["alpha"][b], ref["alpha"], bnd["alpha"])
    _close(fails, "step", "alpha_z", where, ip["alpha_z"][b], ref["alpha_z"], bnd["alpha_z"])
    _close(fails, "step", "f", where, ip["f"][b], ref["f"], bnd["f"])
    if nf0 and not np.array_equal(ip["filt"][b, :nf0], np.array([[float(a), float(p)] for a, p in state["filt"]])):
        fails.append(f"{where}: the old filter entries changed")
    if len(ref["state"]["filt"]) > nf0:
        tf, pf = ref["state"]["filt"][-1]
        _close(fails, "step", "filt_theta", where, ip["filt"][b, nf0, 0], tf, bnd["filt"][0])
        _close(fails, "step", "filt_phi", where, ip["filt"][b, nf0, 1], pf, bnd["filt"][1])
    new = ref["state"]
    _close(fails, "step", "x", where, gx, new["x"], bnd["x"])
    for key, q in (("ip_s", "s"), ("ip_lam", "lam"), ("ip_zl", "zl"), ("ip_zu", "zu")):
        _close(fails, "step", q, where, got[key], new[q], bnd[q])


@pytest.mark.parametrize("tag,N", CASES)
def test_step_stage(tag, N):
    """k_ip_step with the line search and the update on uploaded directions: the chain's own
    steps and the crafted cases (f-type with an Armijo failure first, a filter entry between two
    trials, theta_max between two trials, every trial rejected, a full filter, a NaN direction, alpha_max bound by a lower slack, a
    pending correction on either side of ref_last, both sides of the kappa_sigma clamp); alpha,
    alpha_z, trials, the filter, f, ip_dl, ip_ds, x, s, lam, zl, zu, ref_solves."""
    c = _ctx(tag, N)
    fails, tags, names = [], set(), set()
    for b, cset in enumerate(_sets(c)):
        cs = dict(cset, st=c["st"])
        for case in _chain_cases(cs, "step") + cs["step"]:
            where = f"{tag} N={N} step {case['name']} problem {b}"
            _check_reference(fails, where, case)
            tags |= case["margins"].tags
            names.add(case["name"])
            _step_run(c, b, case, where, fails)
    need = {"all_rejected", "filter_full", "nan_direction", "pending_applied", "pending_grew", "amax_lower", "clamps"}
    assert need <= names, need - names
    if (tag, N) == ("cv24", 2):  # the case with the long chain reaches every branch by itself
        assert ir.STEP_BRANCHES <= tags, ir.STEP_BRANCHES - tags
    assert not fails, "\n".join(fails[:20])
