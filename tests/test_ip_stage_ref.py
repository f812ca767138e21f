"""Pins tests/ip_stage_ref.py (the reference of test_ip_stages_gpu.py) without a GPU.

* chain(dt = fp64), the stage functions run one after the other, reproduces IPRef.solve on two
  small synthetic problems at the default settings and at mu_init = 1e-1, tol = 1e-6: status,
  iteration count, trial counts and every accepted alpha to the bit, x and lam to 1e-12 (they
  are bit-equal too); the long-double chain follows it;
* with the second settings the barrier parameter of ip_stage_ref.PIN_PROBLEMS[0] decreases twice
  in ONE k_ip_kkt call, and PIN_PROBLEMS[1] takes an inertia shift;
* every crafted case (the GPU tests' inputs, built here from the oracle alone) keeps every
  branch decision further than 1e-9 relative from its threshold and takes the branches it was
  built for, and the case set reaches every branch of k_ip_kkt, k_ip_step and k_ip_inertia.
"""
import functools

import numpy as np
import pytest

import ip_stage_ref as ir
import stage_ref as sr
from oracle import ip_ref as I
from oracle.ip_ref import IPRef
from oracle.ocp import OracleOCP

LD = sr.LD


@functools.lru_cache(maxsize=None)
def _evaluator(tag, N, prob):
    R, dyn, kw, P, X = sr.make_problem(tag, N, 1, prob)
    return ir.OracleEval(OracleOCP(R, dyn, N, **kw), P[0]), X[0]


@functools.lru_cache(maxsize=None)
def _pin(ip, iset):
    ev, x0 = _evaluator(*ir.PIN_PROBLEMS[ip])
    st = ir.settings(**ir.PIN_SETTINGS[iset])
    ref = IPRef(ir.CachedOracle(ev), st)
    x, lam, info = ref.solve(x0, ev.p)
    return (x, lam, info, ref.trace), ir.chain(ev, x0, st, dt=np.float64)


@pytest.mark.parametrize("iset", (0, 1))
@pytest.mark.parametrize("ip", (0, 1))
def test_chain_reproduces_ipref(ip, iset):
    (x, lam, info, trace), (xc, lamc, ic) = _pin(ip, iset)
    assert ic["status"] == info["status"] and ic["iter"] == info["iter"]
    assert np.array_equal(ic["alphas"], info["alphas"]), (ic["alphas"], info["alphas"])
    assert np.array_equal(ic["trials"], info["trials"])
    assert np.abs(xc - x).max() <= 1e-12 * max(1.0, np.abs(x).max())
    assert np.abs(lamc - lam).max() <= 1e-12 * max(1.0, np.abs(lam).max())
    assert ic["mus"] == [t["mu"] for t in trace]
    assert [c["dir"]["dwi"] for c in ic["calls"] if "dir" in c] == [t["dwi"] for t in trace]


def test_second_settings_reach_the_barrier_update_and_the_inertia_shift():
    _, (_, _, ic) = _pin(0, 1)
    assert sum(ic["ndecs"]) >= 2 and max(ic["ndecs"]) >= 2, ic["ndecs"]
    assert len(set(ic["mus"])) >= 2 and ic["mus"][-1] < 1e-1
    _, (_, _, ic) = _pin(1, 1)
    assert any(c["dir"]["dwi"] > 0 for c in ic["calls"] if "dir" in c)
    for ip in (0, 1):  # the default settings never move mu: the gap this work closes
        assert sum(_pin(ip, 0)[1][2]["ndecs"]) == 0


def test_long_double_chain_follows_the_fp64_chain():
    """The same code in long double (what the GPU is compared with) takes the same steps over
    the first iterations; later ones drift by the problem's own sensitivity."""
    ev, x0 = _evaluator(*ir.PIN_PROBLEMS[0])
    st = ir.settings(hessian="gauss_newton", **ir.PIN_SETTINGS[1])
    _, _, a = ir.chain(ev, x0, st, dt=np.float64, max_iter=4)
    _, _, b = ir.chain(ev, x0, st, dt=LD, max_iter=4)
    assert np.array_equal(a["trials"], b["trials"])
    assert np.abs(a["alphas"] - b["alphas"]).max() < 1e-10
    assert b["margins"].ok(), b["margins"].worst()


@functools.lru_cache(maxsize=None)
def _case_set(tag, N, prob):
    ev, x0 = _evaluator(tag, N, prob)
    return ir.case_set(ev, x0, ir.settings(hessian="gauss_newton"))


COVER = [(t, N, b) for t, N in (("cv24", 2), ("rnea36", 2)) for b in range(3)]


@pytest.mark.parametrize("tag,N,prob", COVER)
def test_crafted_cases_meet_the_margin_rule(tag, N, prob):
    cs = _case_set(tag, N, prob)
    assert cs["chain"]["margins"].ok(), cs["chain"]["margins"].worst()
    for kind in ("kkt", "step"):
        for c in cs[kind]:
            assert c["margins"].ok(), (kind, c["name"], c["margins"].worst())
            assert c["expect"] <= c["margins"].tags, (kind, c["name"], c["expect"] - c["margins"].tags)


def test_case_set_reaches_every_branch():
    kkt, step = set(), set()
    names = set()
    for key in COVER:
        cs = _case_set(*key)
        kkt |= cs["chain"]["margins"].tags
        step |= cs["chain"]["margins"].tags
        for c in cs["kkt"]:
            kkt |= c["margins"].tags
        for c in cs["step"]:
            step |= c["margins"].tags
            names.add(c["name"])
    assert ir.KKT_BRANCHES <= kkt, ir.KKT_BRANCHES - kkt
    assert ir.STEP_BRANCHES <= step, ir.STEP_BRANCHES - step
    assert {"ftype_armijo", "filter_trial0", "theta_max", "all_rejected", "filter_full", "nan_direction",
            "pending_applied", "pending_grew", "amax_lower", "clamps"} <= names
    # the step cases the list names one by one
    for key in COVER:
        for c in _case_set(*key)["step"]:
            o = c["out"]
            if c["name"] == "all_rejected":
                assert o["status"] == I.ST_LS_FAIL and o["trials"] == c["st"]["ls_max"]
            if c["name"] == "filter_trial0":
                assert o["trials"] >= 2
            if c["name"] == "nan_direction":
                assert o["status"] == I.ST_NONFINITE
            if c["name"] == "filter_full":
                assert o["status"] is None and len(o["state"]["filt"]) == ir.MAXFILT


def test_inertia_table_reaches_every_class():
    seen = set()
    for F, dw in ir.inertia_table():
        for _ in range(ir.INERTIA_CAP + 2):
            seen.add(ir.inertia_class(F, dw))
            F, dw, shift = ir.inertia_ref(F, dw)
            if F[2]:
                break
            F[0] = 1  # the refactor fails again
        assert F[2] == 1 and F[3] <= ir.INERTIA_CAP
    assert seen == set(ir.INERTIA_CLASSES), set(ir.INERTIA_CLASSES) ^ seen


def test_init_case_has_every_row_kind_and_multiplier_class():
    g, l, u, lam0 = ir.init_case(196)
    st = ir.settings()
    eq, hl, hu = I.row_classes(l, u)
    assert eq.any() and (hl & ~hu).any() and (hu & ~hl).any() and (hl & hu).any()
    two = hl & hu
    assert np.any(two & (st["bound_frac"] * (u - l) < st["bound_push"])) and np.any(two & (st["bound_frac"] * (u - l) > 1e-3))
    assert np.any(hl & (np.abs(l) > 1)) and np.any(hl & (g == l)) and np.any(hl & (g < l)) and np.any(hu & (g > u))
    wp = st["warm_start_mult_bound_push"]
    for mask in (hl, hu):
        assert np.any(mask & (lam0 > wp)) and np.any(mask & (lam0 < -wp)) and np.any(mask & (np.abs(lam0) < wp))
    cold, _ = ir.init_ld(g, l, u, st)
    ref = I.push_slacks(g, l, u, eq, hl, hu, st["bound_push"], st["bound_frac"])
    assert np.abs(np.asarray(cold["s"], float) - ref).max() < 1e-15 * 500
    warm, _ = ir.init_ld(g, l, u, st, lam0)
    zl, zu = np.asarray(warm["zl"], float), np.asarray(warm["zu"], float)
    both = hl & hu & (np.abs(lam0) > wp)
    assert np.allclose((zu - zl)[both], lam0[both], rtol=0, atol=1.01 * wp)  # z_u - z_l = lam up to the push
