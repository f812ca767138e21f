"""The adaptive-rho rule of the kernel on the host (csrc/rho_adapt.h through
pl_osqp_rho_estimate_host) against a long-double evaluation of the formulas of
include/pinoloco.h, and the ctypes bindings of the three new handle functions (CPU).

Bar: 4 ulp of the double result -- the estimate is three divisions-or-products and one square
root on correctly rounded inputs, each within 1/2 ulp, the square root halving what is under
it: at most ~2.5 ulp.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import make_robot
from pinoloco import _lib
from pinoloco.ocp import BatchedOCP

LD = np.longdouble
RHO_MIN, RHO_MAX = 1e-6, 1e6


def host(norms, rho, tol):
    a = np.ascontiguousarray(norms, dtype=np.float64)
    est, upd = C.c_double(), C.c_int()
    _lib.check(_lib.lib().pl_osqp_rho_estimate_host(_lib.dptr(a), rho, tol, C.byref(est), C.byref(upd)))
    return est.value, upd.value


def nmax(*v):
    """max that keeps a NaN (a NaN norm must reach the estimate)."""
    v = [LD(x) for x in v]
    return LD(np.nan) if any(np.isnan(x) for x in v) else max(v)


def ref(norms, rho, tol):
    n = [LD(x) for x in norms]
    with np.errstate(all="ignore"):
        pri = n[0] / (nmax(n[1], n[2]) + LD(1e-10))
        dua = n[3] / (nmax(n[4], n[5], n[6]) + LD(1e-10))
        est = LD(rho) * np.sqrt(pri / (dua + LD(1e-10)))
    if est < RHO_MIN:
        est = LD(RHO_MIN)
    elif est > RHO_MAX:
        est = LD(RHO_MAX)
    upd = bool(est > LD(rho) * LD(tol) or est < LD(rho) / LD(tol))
    return est, upd


def check(norms, rho, tol, decision=True):
    est, upd = host(norms, rho, tol)
    e_ld, u_ld = ref(norms, rho, tol)
    if np.isnan(e_ld):
        assert np.isnan(est) and upd == 0
        return est, upd
    err = abs(LD(est) - e_ld)
    assert err <= 4 * np.spacing(float(e_ld)), (norms, rho, tol, est, float(e_ld), float(err))
    if decision:
        assert upd == int(u_ld), (norms, rho, tol, est, upd)
    return est, upd


def test_random_grid():
    rng = np.random.default_rng(11)
    n_upd = 0
    for _ in range(4000):
        norms = 10.0 ** rng.uniform(-9, 3, 7)
        rho = 10.0 ** rng.uniform(-5, 4)
        tol = rng.choice([1.5, 5.0, 10.0, 1e30])
        # a decision within 8 ulp of a threshold may differ from the long-double one: none of
        # these random draws is that close (checked), so every decision is compared
        e_ld, _ = ref(norms, rho, tol)
        for thr in (LD(rho) * LD(tol), LD(rho) / LD(tol)):
            assert abs(e_ld - thr) > 8 * np.spacing(float(thr))
        n_upd += check(norms, rho, tol)[1]
    assert 0 < n_upd < 4000


def norms_for_ratio(t):
    """Norms whose estimate is (to a few ulp) rho * t: pri / (dua + 1e-10) = t^2."""
    dua = LD(1.0) / (LD(1.0) + LD(1e-10))
    pri = LD(t) ** 2 * (dua + LD(1e-10))
    return [float(pri * (LD(1.0) + LD(1e-10))), 1.0, 0.3, 1.0, 1.0, 0.2, 0.1]


@pytest.mark.parametrize("tol", [5.0, 2.0])
@pytest.mark.parametrize("side", [1.0, -1.0])
@pytest.mark.parametrize("gap", [1e-3, 1e-6, 1e-9, 1e-12])
def test_thresholds_from_either_side(tol, side, gap):
    rho = 0.02
    for thr, beyond in ((tol, 1.0), (1.0 / tol, -1.0)):  # upper: update above; lower: update below
        est, upd = check(norms_for_ratio(thr * (1.0 + side * gap)), rho, tol)
        assert upd == int(side == beyond), (thr, side, gap, est)


def test_clips_and_zeros():
    rho, tol = 0.02, 5.0
    assert check([1e9, 1.0, 1.0, 1e-9, 1.0, 1.0, 1.0], rho, tol) == (RHO_MAX, 1)   # upper clip
    assert check([1e-12, 1.0, 1.0, 1e6, 1.0, 1.0, 1.0], rho, tol) == (RHO_MIN, 1)  # lower clip
    assert check([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], rho, tol) == (RHO_MIN, 1)    # pri = 0
    est, upd = check([1e-3, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0], rho, tol)               # dua = 0
    assert upd == 1 and est == pytest.approx(rho * np.sqrt(1e-3 / (1 + 1e-10) / 1e-10), rel=1e-12)
    assert check([0.0] * 7, rho, tol) == (RHO_MIN, 1)                              # all zero: 0 / 1e-10
    assert check([0.0] * 7, 2e-6, tol) == (RHO_MIN, 0)                             # ... inside the band
    assert check([1e-3, 1.0, 1.0, 1e-3, 1.0, 1.0, 1.0], rho, tol)[1] == 0          # balanced: no update


@pytest.mark.parametrize("k", range(7))
def test_nan_norm_gives_no_update(k):
    norms = [1e-2, 1.0, 1.0, 1e-4, 1.0, 1.0, 1.0]
    norms[k] = np.nan
    est, upd = host(norms, 0.02, 5.0)
    assert upd == 0 and np.isnan(est)
    check(norms, 0.02, 5.0)


def test_inf_norm_gives_no_nan_update():
    # inf / inf = NaN: no update; inf alone clips
    assert host([np.inf, np.inf, 1.0, 1.0, 1.0, 1.0, 1.0], 0.02, 5.0)[1] == 0
    assert host([np.inf, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 0.02, 5.0) == (RHO_MAX, 1)


# ---------------------------------------------------------------- bindings (host-only handle)
@pytest.fixture(scope="module")
def host_handle():
    bo = BatchedOCP(make_robot("go2"), "whole_body_rnea", 6, batch=2, device=-1)
    yield bo
    bo.close()


def test_set_get_round_trip(host_handle):
    bo = host_handle
    assert bo.adaptive_rho() == (False, 0, 5.0)  # the default: off, OSQP's tolerance
    bo.set_adaptive_rho(True, 50, 3.5)
    assert bo.adaptive_rho() == (True, 50, 3.5)
    assert bo.settings["adaptive_rho"] is True and bo.settings["adaptive_rho_interval"] == 50
    bo.set_adaptive_rho(False)
    assert bo.adaptive_rho() == (False, 0, 5.0)


@pytest.mark.parametrize("interval", [-25, 10, 30])
def test_bad_interval_refused(host_handle, interval):
    before = host_handle.adaptive_rho()
    with pytest.raises(_lib.PinolocoError, match="adaptive_rho_interval"):
        host_handle.set_adaptive_rho(True, interval, 5.0)
    assert host_handle.adaptive_rho() == before


@pytest.mark.parametrize("tol", [1.0, 0.5, -2.0, float("nan")])
def test_bad_tolerance_refused(host_handle, tol):
    before = host_handle.adaptive_rho()
    with pytest.raises(_lib.PinolocoError, match="adaptive_rho_tolerance"):
        host_handle.set_adaptive_rho(True, 0, tol)
    assert host_handle.adaptive_rho() == before


def test_get_rho_needs_a_device(host_handle):
    with pytest.raises(_lib.PinolocoError, match="no device"):
        host_handle.osqp_rho()


def test_osqp_settings_are_honoured():
    R = make_robot("go2")
    bo = BatchedOCP(R, "whole_body_rnea", 6, batch=1, device=-1,
                    osqp_settings={"adaptive_rho": True, "adaptive_rho_interval": 25, "adaptive_rho_tolerance": 4.0})
    assert bo.adaptive_rho() == (True, 25, 4.0)
    bo.close()
    with pytest.raises(_lib.PinolocoError, match="adaptive_rho_interval"):
        BatchedOCP(R, "whole_body_rnea", 6, batch=1, device=-1,
                   osqp_settings={"adaptive_rho": True, "adaptive_rho_interval": 7})
