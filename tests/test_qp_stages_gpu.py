"""The stages on either side of the factor and the sweeps, one by one on the MI355X against the
long-double reference of tests/qp_stage_ref.py: the QP setup (k_ruiz_fused and the per-pass
k_ruiz_init / k_ruiz_norms / k_ruiz_update, k_qp_finish), k_admm_init's right-hand side, the
termination check (k_check_part's residual partials, k_check's thresholds, certificates and
x10 pass), k_unscale and the delta stores of every ADMM kernel.  test_stage_kernels_gpu.py holds
the factor and the iterates; this file reuses its cases (stage_ref.CASES at N = 2 and 3 or 4,
B = 3 synthetic problems), its variants and its references.

The debug entry points: debug_admm(0) evaluates and scales, debug_qp_setup() scales whatever raw
data debug_set wrote, debug_check() runs one termination check on whatever iterates, deltas and
scaled data debug_set wrote, debug_admm(k, delta=True) runs k iterations with the last one
storing delta x / delta y.  A failure names a stage, a problem and a node.

Bars.  Continuous quantities: e_gpu <= K * e64 + floor with the project's K = 16, e64 the error
of the fp64 oracle route (OSQPRef._scale / _info themselves, numpy for the right-hand side,
BlockReduced for the deltas) against the long-double reference on the same bits.  D, E, cs, As,
Ps, qs, ls, us are products, so their error is taken ENTRYWISE (|a - ref| / |ref|, stricter than
the inf-norm measure, and a zero must be a zero) with the floor scaling_passes * 4 * 2^-52: the
device keeps D and E cumulatively against the raw data, the oracle rescales the matrix every
pass.  Sums (rhs, the residuals, the chk partials) use stage_ref.rel and floor(1, longest row or
column + 2); dxs / dys are taken relative to the inf-norm of the iterate (the difference cancels)
with floor(k, nw_max).  Exact quantities (rho, rhoc, statuses, NaN / zero patterns, bits between
the Ruiz paths and between stores on and off): no tolerance.  Margins (asserted on the reference,
proved without a GPU by test_qp_stage_ref.py): every _limit argument outside t (1 +- 1e-9), every
rho-class decision 1e6 roundings wide, every comparison of the check 1e-6 wide; the one argument
not held to it is the cost scale's second clamp where it is the constant MAX_SCALING itself
(qp_stage_ref.scale_ld).  Every run writes e_gpu, e64 and the ratio to qp_stage_errors.json in
the directory PL_TEST_OUT names (default: test_out/ in the repository root).
"""
import json
import os

import numpy as np
import pytest

import qp_stage_ref as qr
import stage_ref as sr
import test_stage_kernels_gpu as tsk
from oracle import osqp_ref as O

pytestmark = pytest.mark.gpu

K_BAR = 16.0
EXCEPTIONS = {}  # (case, stage, quantity) -> (allowed factor, measured ratio, reason); at most two
# worst e_gpu / max(e64, floor) per quantity over all cases on the MI355X (qp_stage_errors.json)
MEASURED = {"D": 0.105, "E": 0.107, "cs": 0.035, "As": 0.135, "Ps": 0.205, "qs": 0.077, "ls": 0.101, "us": 0.101,
            "rhs": 0.030, "pri_res": 0.027, "dua_res": 0.022, "chk_pri": 0.047, "chk_nz": 0.014, "chk_nax": 0.038,
            "chk_dua": 0.032, "chk_nq": 0.012, "chk_naty": 0.034, "chk_npx": 0.015, "dxs": 5.6, "dys": 6.6}
# (below 1: the floor is the larger term of the bar.  Against e64 alone the scaled data are at most
# 3.9 x the oracle's own entrywise error, 2e-15 at the worst, and the sums at most 5.2 x, 7e-16.)

TAGS = ("cv24", "cv30", "rnea36", "fd36", "aba36", "rnea48")
CASES = [(t, N) for t in TAGS for N in sr.case(t)[4][:2]]
RUIZ_PATHS = {"fused": (), "per_pass": ("ruiz_per_pass",)}
ALL_STATUSES = {1, 2, -2, -3, 3, -4, 4, -7, -10}
BAD = (O.PRIMAL_INFEASIBLE, O.PRIMAL_INFEASIBLE_INACCURATE, O.DUAL_INFEASIBLE, O.DUAL_INFEASIBLE_INACCURATE, O.NON_CVX)
CLAMP_MARGIN, RHO_MARGIN, CHECK_MARGIN = 1e-9, 1e6, 1e-6
SEED = 11
SETUP_KEYS = ("D", "E", "cs", "As", "Ps", "qs", "ls", "us", "rho")

_RECORDS = []
OUT = os.path.join(os.environ.get("PL_TEST_OUT") or os.path.join(sr.ROOT, "test_out"), "qp_stage_errors.json")


@pytest.fixture(scope="module", autouse=True)
def _write_records():
    yield
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    worst = {}
    for r in _RECORDS:
        w = worst.get(r["quantity"])
        if w is None or r["ratio"] > w["ratio"]:
            worst[r["quantity"]] = r
    with open(OUT, "w") as f:
        json.dump({"K": K_BAR, "worst_by_quantity": worst, "records": _RECORDS}, f, indent=1)


def _judge(fails, case, stage, quantity, where, e_gpu, e64, fl):
    exc = EXCEPTIONS.get((case, stage, quantity))
    factor = exc[0] if exc else K_BAR
    bar = factor * e64 + fl
    _RECORDS.append(dict(case=case, stage=stage, quantity=quantity, where=where, e_gpu=e_gpu, e64=e64, floor=fl,
                         ratio=e_gpu / max(e64, fl), bar=bar))
    print(f"{case} {stage} {quantity} {where}: e_gpu {e_gpu:.3e} e64 {e64:.3e} floor {fl:.1e}")
    if not (e_gpu <= bar):  # also catches NaN
        fails.append(f"{case} {stage} {where} {quantity}: e_gpu {e_gpu:.3e} > {factor:g} * e64 {e64:.3e} + floor {fl:.1e}")


def _read(bo, names):
    B = bo.batch
    ln = dict(D=bo.n, E=bo.m, cs=1, As=bo.nnz, Ps=bo.n, qs=bo.n, ls=bo.m, us=bo.m, rho=bo.m, rhs=bo.n, xa=bo.n,
              za=bo.m, ya=bo.m, dxs=bo.n, dys=bo.m, step=bo.n, chk=(bo.layout.N + 1) * 8)
    return {k: bo.debug(k, B * ln[k]).reshape(B, ln[k]) for k in names}


def _where(raw, quantity, k):
    if quantity in ("D", "Ps", "qs"):
        return f"node {qr.node_of_col(raw, k)} column {k}"
    if quantity in ("E", "ls", "us"):
        return f"node {qr.node_of_row(raw, k)} row {k}"
    if quantity == "As":
        r, c = int(raw["rows"][k]), int(raw["cols"][k])
        return f"node {qr.node_of_row(raw, r)} entry ({r}, {c})"
    return ""


def _coupling_rows(raw, nodes):
    """Per node the rows with an entry in a dx_{i+1} column, ascending (the rows of rhoc)."""
    out = []
    for (o, w, _), rr in zip(raw["blocks"], raw["node_rows"]):
        sel = np.isin(raw["rows"], rr) & (raw["cols"] >= o + w)
        out.append(np.unique(raw["rows"][sel]))
    return out


def _setup_reference(raw, s):
    sc = qr.scale_ld(raw["P"], raw["q"], (raw["rows"], raw["cols"], raw["A"], raw["m"]), s)
    fin = qr.finish_ld(raw["lbg"], raw["ubg"], raw["g"], sc["E"], s)
    s64 = qr.scale64(raw, s)
    f64 = qr.finish64(raw, s64["E"], s)
    assert qr.clamp_margin(sc["clamps"]) >= CLAMP_MARGIN
    assert qr.rho_margin(fin["decisions"]) >= RHO_MARGIN
    ref = dict(D=sc["D"], E=sc["E"], cs=sc["c"], As=sc["A"], Ps=sc["P"], qs=sc["q"], ls=fin["ls"], us=fin["us"])
    r64 = dict(D=s64["D"], E=s64["E"], cs=s64["c"], As=s64["A"], Ps=s64["P"], qs=s64["q"], ls=f64["ls"], us=f64["us"])
    return ref, r64, fin["rho"]


def _compare_setup(fails, bo, case, stage, b, raw, dev, refs, s):
    ref, r64, rho = refs
    fl = qr.floor_products(s)
    for k in ("D", "E", "cs", "As", "Ps", "qs", "ls", "us"):
        e_gpu, at = qr.rel_entry(dev[k][b], ref[k])
        _judge(fails, case, stage, k, f"problem {b} {_where(raw, k, at)}", e_gpu, qr.rel_entry(r64[k], ref[k])[0], fl)
    bad = np.flatnonzero(dev["rho"][b] != rho)
    if bad.size:
        r = int(bad[0])
        fails.append(f"{case} {stage} problem {b} node {qr.node_of_row(raw, r)} row {r}: rho {dev['rho'][b][r]} != "
                     f"{rho[r]} ({bad.size} rows)")
    nodes = bo.node_table()
    ncm = max(int(nodes[:, 11].max()), 1)
    rhoc = bo.debug("rhoc", bo.batch * len(nodes) * ncm).reshape(bo.batch, len(nodes), ncm)[b]
    for i, cr in enumerate(_coupling_rows(raw, nodes)):
        assert cr.size == nodes[i][11], (case, i, "coupling rows of the pattern against the node table")
        if not np.array_equal(rhoc[i, :cr.size], rho[cr]):
            fails.append(f"{case} {stage} problem {b} node {i}: rhoc is not rho of the coupling rows")


def _both_paths(tag, N, stage, prepare):
    """Runs ``prepare(bo) -> [raw per problem]`` and the comparison on both Ruiz paths; the
    device's outputs must agree bit for bit between them."""
    fails, outs, refs = [], {}, None
    for path, dp in RUIZ_PATHS.items():
        bo = sr.make_handle(tag, N, sr.BATCH, debug_paths=dp)
        try:
            s = qr.settings_of(bo)
            raws = prepare(bo)
            dev = _read(bo, SETUP_KEYS)
            if refs is None:
                refs = [_setup_reference(raw, s) for raw in raws]
            for b, raw in enumerate(raws):
                _compare_setup(fails, bo, f"{tag}-{N}", f"{stage}/{path}", b, raw, dev, refs[b], s)
            outs[path] = dev
        finally:
            bo.close()
    for k in SETUP_KEYS:
        assert np.array_equal(outs["fused"][k], outs["per_pass"][k]), (k, "fused against per-pass Ruiz")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------- (a) natural scaling
@pytest.mark.parametrize("tag,N", CASES)
def test_natural_scaling(tag, N):
    """D, E, cs, As, Ps, qs, ls, us, rho and rhoc of the evaluated problem, from the raw bits."""
    def prepare(bo):
        bo.debug_admm(0)
        arrays = qr.read_raw(bo)
        return [qr.raw_from_device(bo, b, arrays) for b in range(bo.batch)]
    _both_paths(tag, N, "natural", prepare)


# ---------------------------------------------------------------------------- (b) crafted raw data
@pytest.mark.parametrize("tag,N", CASES)
def test_crafted_scaling(tag, N):
    """qp_stage_ref.craft_raw on the evaluated data (problem b: gradient variant b): zero and
    extreme columns and rows, every clamp of limit_scaling, every rho class and both sides of
    PL_RHO_TOL, in node 0, a middle node and node N - 1."""
    def prepare(bo):
        bo.debug_admm(0)
        arrays = qr.read_raw(bo)
        s = qr.settings_of(bo)
        raws = []
        for b in range(bo.batch):
            cr, what = qr.craft_raw(qr.raw_from_device(bo, b, arrays), s, SEED, b % 3)
            fin = qr.finish_ld(cr["lbg"], cr["ubg"], cr["g"],
                               qr.scale_ld(cr["P"], cr["q"], (cr["rows"], cr["cols"], cr["A"], cr["m"]), s)["E"], s)
            qr.check_crafted(cr, what, fin, b % 3, s)
            raws.append(cr)
        for name, key in (("Araw", "A"), ("P", "P"), ("grad", "q"), ("lbg", "lbg"), ("ubg", "ubg")):
            bo.debug_set(name, np.stack([r[key] for r in raws]))
        bo.debug_qp_setup()
        return raws
    _both_paths(tag, N, "crafted", prepare)


# ---------------------------------------------------------------------------- (c) k_admm_init
def _scaled_qps(bo):
    """Per problem (raw pattern data, scaled QP dict, D, E, c) as the device holds them."""
    dev = _read(bo, ("D", "E", "cs", "As", "Ps", "qs", "ls", "us", "rho"))
    arrays = qr.read_raw(bo)
    out = []
    for b in range(bo.batch):
        raw = qr.raw_from_device(bo, b, arrays)
        qp = dict(A=dev["As"][b], P=dev["Ps"][b], q=dev["qs"][b], l=dev["ls"][b], u=dev["us"][b], rho=dev["rho"][b])
        out.append((raw, qp, dev["D"][b], dev["E"][b], float(dev["cs"][b][0])))
    return out


def _longest(raw):
    return int(max(np.bincount(raw["rows"]).max(), np.bincount(raw["cols"]).max())) + 2


@pytest.mark.parametrize("tag,N", CASES)
def test_admm_init_rhs(tag, N):
    """rhs = sigma x - q + A^T (rho z - y) from seeded random iterates (the zero-iteration path)."""
    fails = []
    bo = sr.make_handle(tag, N, sr.BATCH)
    try:
        s = qr.settings_of(bo)
        rng = np.random.default_rng(7)
        start = [0.1 * rng.standard_normal((bo.batch, ln)) for ln in (bo.n, bo.m, bo.m)]
        for nm, v in zip(("xa", "za", "ya"), start):
            bo.debug_set(nm, v)
        bo.debug_admm(0, reset=False)
        rhs = _read(bo, ("rhs",))["rhs"]
        for b, (raw, qp, _, _, _) in enumerate(_scaled_qps(bo)):
            x, z, y = (v[b] for v in start)
            want = qr.rhs_any(raw, qp, x, z, y, s["sigma"], sr.LD)
            e64 = sr.rel(qr.rhs_any(raw, qp, x, z, y, s["sigma"], np.float64), want)
            at = int(np.argmax(np.abs(rhs[b] - want)))
            _judge(fails, f"{tag}-{N}", "admm_init", "rhs", f"problem {b} node {qr.node_of_col(raw, at)} column {at}",
                   sr.rel(rhs[b], want), e64, sr.floor(1, _longest(raw)))
    finally:
        bo.close()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------- (d) residuals
@pytest.mark.parametrize("tag,N", CASES)
def test_residuals(tag, N):
    """pri_res, dua_res and the seven per-node partial maxima of k_check_part (node N included)
    on the natural scaled QP with seeded random iterates."""
    fails = []
    bo = sr.make_handle(tag, N, sr.BATCH)
    try:
        s = qr.settings_of(bo)
        bo.debug_admm(0)
        rng = np.random.default_rng(9)
        start = [0.1 * rng.standard_normal((bo.batch, ln)) for ln in (bo.n, bo.m, bo.m)]
        for nm, v in zip(("xa", "za", "ya"), start):
            bo.debug_set(nm, v)
        st = bo.debug_check()
        chk = _read(bo, ("chk",))["chk"].reshape(bo.batch, N + 1, 8)
        for b, (raw, qp, D, E, c) in enumerate(_scaled_qps(bo)):
            x, z, y = (v[b] for v in start)
            assert st["status"][b] == O.UNSOLVED
            ld = qr.info_ld(raw, qp, x, z, y, D, E, c)
            i64 = qr.info64(raw, qp, x, z, y, D, E, c, s)
            fl, case = sr.floor(1, _longest(raw)), f"{tag}-{N}"
            for nm in ("pri_res", "dua_res"):
                _judge(fails, case, "check", nm, f"problem {b}", sr.rel(st[nm][b], ld[nm]), sr.rel(i64[nm], ld[nm]), fl)
            for k, nm in enumerate(qr.CHK):
                at = int(np.argmax(np.abs(chk[b][:, k] - ld["part"][:, k])))
                _judge(fails, case, "check_part", "chk_" + nm, f"problem {b} node {at}",
                       sr.rel(chk[b][:, k], ld["part"][:, k]), sr.rel(i64["part"][:, k], ld["part"][:, k]), fl)
            assert np.all(chk[b][N, :3] == 0), "node N has no rows"
    finally:
        bo.close()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------- (e) statuses, (g) k_unscale
@pytest.mark.parametrize("tag,N", CASES)
def test_statuses_and_unscale(tag, N):
    """Every construction of qp_stage_ref.craft_state on the device's scaled QP: the status of
    k_check equals the long-double reference's, whose comparisons all have a 1e-6 margin; the
    reference reaches every status; k_unscale then writes step = D x and leaves the iterates,
    or NaN and cold iterates after a certificate or NON_CVX."""
    bo = sr.make_handle(tag, N, sr.BATCH)
    seen, fails = set(), []
    try:
        s = qr.settings_of(bo)
        bo.debug_admm(0)
        base = _scaled_qps(bo)
        for name in qr.STATE_NAMES:
            built = [qr.craft_state(name, raw, qp, D, E, c, s, SEED + b) for b, (raw, qp, D, E, c) in enumerate(base)]
            final = built[0][2]
            want = []
            for (q2, it, fin, expect), (raw, _, D, E, c) in zip(built, base):
                got, comps, _ = qr.terminate_ld(raw, q2, it, D, E, c, s, fin)
                assert got == expect, (name, "the reference misses the construction's status", got, expect)
                assert qr.margin(comps) >= CHECK_MARGIN, (name, qr.margin(comps))
                want.append(got)
                seen.add(got)
            for dn, key in (("As", "A"), ("Ps", "P"), ("qs", "q"), ("ls", "l"), ("us", "u")):
                bo.debug_set(dn, np.stack([bt[0][key] for bt in built]))
            for dn, key in (("xa", "x"), ("za", "z"), ("ya", "y"), ("dxs", "dx"), ("dys", "dy")):
                bo.debug_set(dn, np.stack([bt[1][key] for bt in built]))
            st = bo.debug_check(final=final, unscale=True)
            after = _read(bo, ("step", "xa", "za", "ya"))
            for b, (raw, _, D, _, _) in enumerate(base):
                it = built[b][1]
                if st["status"][b] != want[b]:
                    fails.append(f"{tag}-{N} {name} problem {b}: status {st['status'][b]}, reference {want[b]}")
                    continue
                if want[b] in BAD:
                    ok = np.all(np.isnan(after["step"][b])) and not any(after[k][b].any() for k in ("xa", "za", "ya"))
                else:
                    ok = np.array_equal(after["step"][b], D * it["x"]) and all(
                        np.array_equal(after[k][b], it[v]) for k, v in (("xa", "x"), ("za", "z"), ("ya", "y")))
                if not ok:
                    fails.append(f"{tag}-{N} {name} problem {b}: k_unscale after status {want[b]}")
    finally:
        bo.close()
    assert seen == ALL_STATUSES, seen
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------- (f) delta stores
def _delta_compare(fails, case, stage, k, b, ref, dxs, dys, nw_max, key="cold"):
    ld = ref.iterates("ld", k, key=key)
    b64 = ref.iterates("block64", k, key=key)
    for nm, j, got in (("dxs", 0, dxs), ("dys", 2, dys)):
        prev_ld = ld[k - 2][j] if k > 1 else 0
        prev_64 = b64[k - 2][j] if k > 1 else 0
        want = ld[k - 1][j] - prev_ld
        scale = max(float(np.abs(ld[k - 1][j]).max()), 1e-300)
        e_gpu = float(np.abs(np.asarray(got, sr.LD) - want).max()) / scale
        e64 = float(np.abs((b64[k - 1][j] - prev_64) - want).max()) / scale
        _judge(fails, case, stage, nm, f"problem {b} k={k}", e_gpu, e64, sr.floor(k, nw_max))


@pytest.mark.parametrize("tag,N", CASES)
def test_delta_stores(tag, N):
    """dxs = x_k - x_{k-1} and dys = y_k - y_{k-1} of the long-double iterates after k = 1, 2, 10
    iterations from cold with the stores on, for every ADMM kernel variant; the iterates are
    bit-equal to the run with the stores off."""
    fails = []
    for variant in tsk.VARIANTS:
        if tag == "fd36" and tsk.VARIANTS[variant][0] == "chain":
            continue  # the general coupling has no chain kernel (test_chain_kernel_from_cold)
        bo = sr.make_handle(tag, N, sr.BATCH, debug_paths=tsk.VARIANTS[variant][2])
        try:
            tsk._configure(bo, variant)
            nw_max = bo.sizes()["nw_max"]
            raw = None
            for k in sorted(tsk.KS, reverse=True):
                bo.debug_admm(k, reset=True)
                off = tsk._iterates(bo)
                bo.debug_admm(k, reset=True, delta=True)
                on = tsk._iterates(bo)
                for j, nm in enumerate(("xa", "za", "ya")):
                    assert np.array_equal(off[j], on[j]), (variant, k, nm, "stores on against off")
                d = _read(bo, ("dxs", "dys"))
                raw = raw or sr.read_scaled(bo)
                for b in range(bo.batch):
                    ref = tsk._get_reference(bo, tag, N, b, raw)
                    _delta_compare(fails, f"{tag}-{N}", variant, k, b, ref, d["dxs"][b], d["dys"][b], nw_max)
        finally:
            bo.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("tag,N", [("cv24", 3), ("rnea36", 2)])
def test_delta_after_solve_per_pass_ruiz(tag, N):
    """After a full solve() on the per-pass Ruiz path, where k_ruiz_norms' scratch and the delta
    stores share dxs / dys: the deltas of each problem's last check iteration, and the same bits
    as on the fused path."""
    fails, outs = [], {}
    for path, dp in RUIZ_PATHS.items():
        bo = sr.make_handle(tag, N, sr.BATCH, debug_paths=dp)
        try:
            st = bo.solve()
            d = _read(bo, ("dxs", "dys"))
            outs[path] = (st["admm_iters"].copy(), d["dxs"], d["dys"])
            if path == "per_pass":
                raw = sr.read_scaled(bo)
                nw_max = bo.sizes()["nw_max"]
                for b in range(bo.batch):
                    k = int(st["admm_iters"][b])
                    assert k > 0 and k % 25 == 0, st
                    ref = tsk._get_reference(bo, tag, N, b, raw)  # the same scaled QP as debug_admm's
                    _delta_compare(fails, f"{tag}-{N}", "solve/per_pass", k, b, ref, d["dxs"][b], d["dys"][b], nw_max)
        finally:
            bo.close()
    for a, b in zip(outs["fused"], outs["per_pass"]):
        assert np.array_equal(a, b), "fused against per-pass Ruiz after solve()"
    assert not fails, "\n".join(fails)
