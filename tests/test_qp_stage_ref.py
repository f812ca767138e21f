"""The QP stage reference (tests/qp_stage_ref.py) without a GPU, on the numpy oracle's data of two
cases: the long-double scaling and residuals agree with OSQPRef._scale / _info, the crafted raw
data of test_qp_stages_gpu.py (b) and its crafted termination states (e) meet their margin
conditions on the reference alone, and the states reach every status through OSQPRef._check
itself.  This pins the reference and the constructions before anyone has a GPU.
"""
import numpy as np
import pytest

import qp_stage_ref as qr
import stage_ref as sr
from oracle import osqp_ref as O

CASES = [("cv24", 3), ("rnea36", 2)]
ALL_STATUSES = {1, 2, -2, -3, 3, -4, 4, -7, -10}
CLAMP_MARGIN = 1e-9
CHECK_MARGIN = 1e-6
RHO_MARGIN = 1e6
SEED = 11

_DATA = {}


def _data(tag, N):
    if (tag, N) not in _DATA:
        _DATA[tag, N] = qr.raw_from_oracle(tag, N)
    return _DATA[tag, N]


def _scaled(raw, settings):
    """The long-double scaling rounded to fp64: the scaled QP the state constructions work on."""
    sc = qr.scale_ld(raw["P"], raw["q"], (raw["rows"], raw["cols"], raw["A"], raw["m"]), settings)
    fin = qr.finish_ld(raw["lbg"], raw["ubg"], raw["g"], sc["E"], settings)
    f = lambda v: np.asarray(v, float)
    return dict(A=f(sc["A"]), P=f(sc["P"]), q=f(sc["q"]), l=f(fin["ls"]), u=f(fin["us"])), f(sc["D"]), f(sc["E"]), float(
        sc["c"])


@pytest.mark.parametrize("tag,N", CASES)
def test_scaling_matches_oracle(tag, N):
    raw, s = _data(tag, N)
    sc = qr.scale_ld(raw["P"], raw["q"], (raw["rows"], raw["cols"], raw["A"], raw["m"]), s)
    s64 = qr.scale64(raw, s)
    for k in ("D", "E", "c", "P", "q", "A"):
        e, where = qr.rel_entry(s64[k], sc[k])
        assert e < 1e-12, (k, e, where)
    assert qr.clamp_margin(sc["clamps"]) >= CLAMP_MARGIN
    fin = qr.finish_ld(raw["lbg"], raw["ubg"], raw["g"], sc["E"], s)
    f64 = qr.finish64(raw, s64["E"], s)
    for k in ("ls", "us"):
        assert qr.rel_entry(f64[k], fin[k])[0] < 1e-12, k
    assert qr.rho_margin(fin["decisions"]) >= RHO_MARGIN
    # the rho classes are the oracle's (stage_ref.oracle_qp restates update_and_solve lines 201-205)
    qp, _, _ = sr.oracle_qp(tag, N)
    assert np.array_equal(fin["rho"], qp["rho"])


@pytest.mark.parametrize("tag,N", CASES)
def test_residuals_match_oracle(tag, N):
    raw, s = _data(tag, N)
    qp, D, E, c = _scaled(raw, s)
    rng = np.random.default_rng(5)
    x, z, y = (0.1 * rng.standard_normal(k) for k in (raw["n"], raw["m"], raw["m"]))
    ld = qr.info_ld(raw, qp, x, z, y, D, E, c)
    i64 = qr.info64(raw, qp, x, z, y, D, E, c, s)
    assert abs(i64["pri_res"] / float(ld["pri_res"]) - 1) < 1e-12
    assert abs(i64["dua_res"] / float(ld["dua_res"]) - 1) < 1e-12
    assert sr.rel(i64["part"], ld["part"]) < 1e-12
    assert np.all(ld["part"][-1, :3] == 0) and np.all(ld["part"][-1, 3:5] > 0)  # node N: columns, no rows
    r64 = qr.rhs_any(raw, dict(qp, rho=np.full(raw["m"], s["rho"])), x, z, y, s["sigma"], np.float64)
    rld = qr.rhs_any(raw, dict(qp, rho=np.full(raw["m"], s["rho"])), x, z, y, s["sigma"], sr.LD)
    assert sr.rel(r64, rld) < 1e-12


@pytest.mark.parametrize("tag,N", CASES)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_crafted_raw_meets_margins(tag, N, variant):
    raw, s = _data(tag, N)
    cr, what = qr.craft_raw(raw, s, SEED, variant)
    sc = qr.scale_ld(cr["P"], cr["q"], (cr["rows"], cr["cols"], cr["A"], cr["m"]), s)
    fin = qr.finish_ld(cr["lbg"], cr["ubg"], cr["g"], sc["E"], s)
    qr.check_crafted(cr, what, fin, variant, s)
    assert qr.clamp_margin(sc["clamps"]) >= CLAMP_MARGIN
    assert qr.rho_margin(fin["decisions"]) >= RHO_MARGIN
    assert np.all(np.isfinite(np.asarray(sc["D"], float))) and np.all(np.isfinite(np.asarray(sc["E"], float)))
    # the clamps are exercised: arguments on both outer sides of both thresholds
    cl = sc["clamps"]
    assert (cl < O.MIN_SCALING).any() and (cl > O.MAX_SCALING).any()
    s64 = qr.scale64(cr, s)
    for k in ("D", "E", "c", "P", "q", "A"):
        assert qr.rel_entry(s64[k], sc[k])[0] < 1e-11, k


@pytest.mark.parametrize("tag,N", CASES)
def test_crafted_states_reach_every_status(tag, N):
    raw, s = _data(tag, N)
    qp, D, E, c = _scaled(raw, s)
    seen = set()
    for name in qr.STATE_NAMES:
        q2, st, final, want = qr.craft_state(name, raw, qp, D, E, c, s, SEED)
        got, comps, _ = qr.terminate_ld(raw, q2, st, D, E, c, s, final)
        assert got == want, (name, got, want)
        assert qr.margin(comps) >= CHECK_MARGIN, (name, qr.margin(comps))
        got64, _ = qr.terminate64(raw, q2, st, D, E, c, s, final)
        assert got64 == want, (name, "OSQPRef._check", got64, want)
        seen.add(got)
    assert seen == ALL_STATUSES
