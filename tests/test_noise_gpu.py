"""Per-step random state noise and base wrench of the device MPC loop on the MI355X (pl_mpc_set_noise,
k_mpc_prepare's draw lanes, csrc/noise.h).

The integer part of the generator (pl_debug_rng) equals the numpy twin (tests/noise_ref.py) bit for
bit, the three published Random123 known answers among them.  The drawn normals are compared with
pl_mpc_noise_host, the same header on the host, whose log, cos and sin are another libm: over the
draws of test_draws_equal_the_host (sigma = 1, both streams, k = 0, 1, 5, Go2, B2G and Go2
centroidal_vel) the largest distance between the device's z and the host's was 2 ulp.  The bar is four
times that, DEV_MEASURED_ULP * 4 = 8 ulp, under the same cap as on the host (a relative 2**-46;
tests/test_noise_host.py).  Everything else is an identity between two runs on the device and is
compared bit for bit, as uint64 words (tests/test_rollout_gpu.py).

Shapes: Go2 whole_body_rnea, N = 6, batch 4, at most 6 steps, synthetic problems, each with its own
dt_min; one Go2 centroidal_vel case and one B2G rnea case (ndx = 48, the widest lane map; an odd /
even component pair shares a block at every width)."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libpinoloco.so, so both share one HIP runtime)

import noise_ref as nr
import rollout_ref as rr
from conftest import make_robot
from test_noise_host import CAP_REL
from test_timeline_gpu import _run, _same, _start

pytestmark = pytest.mark.gpu

N, B, STEPS = 6, 4, 5
DEV_MEASURED_ULP = 2      # device against the host, see the module docstring
DEV_BAR_ULP = 4 * DEV_MEASURED_ULP
CASES = [("go2", "whole_body_rnea"), ("b2g", "whole_body_rnea"), ("go2", "centroidal_vel")]
CASE_IDS = ["go2-rnea", "b2g-rnea", "go2-cv"]


def _seeds(batch=B, first=0):
    from pinoloco.synthetic import noise_seeds
    return noise_seeds(first, batch)


def _sigmas(ndx, batch=B):
    """Per-problem, per-component sigmas: a few mrad / mm on the state, newtons on the wrench."""
    rng = np.random.default_rng(21)
    return rng.uniform(0.002, 0.01, (batch, ndx)), rng.uniform(2.0, 10.0, (batch, 6))


def _x_init(bo, lay):
    o = lay.poff["x_init"][0]
    return bo.get_params()[:, o:o + lay.nx]


def _logs_equal(la, lb, steps=STEPS):
    for f in rr.FIELDS:
        assert la[f].shape[0] == steps and _same(la[f], lb[f]), f


# ---------------------------------------------------------------- 1. the integers
def test_device_blocks_equal_the_twin():
    R, lay, P, X, T0, bo = _start()
    try:
        seeds = _seeds()
        bo.mpc_set_noise(seeds, 0.01)
        for stream in (nr.STREAM_STATE, nr.STREAM_WRENCH):
            for k in (0, 1, 5):
                got = bo.debug_rng(k, stream, 24)
                assert got.shape == (B, 24, 4) and np.array_equal(got, nr.blocks(seeds, k, stream, 24)), (stream, k)
        # the published known answers, by keys and counters that hit them
        kat = np.array([(key[1] << 32) | key[0] for _, key, _ in nr.KNOWN] + [5], dtype=np.uint64)
        bo.mpc_set_noise(kat, None, 1.0)
        for b, (ctr, key, out) in enumerate(nr.KNOWN):
            got = bo.debug_rng(ctr[0], ctr[2], 1, i0=ctr[1], c3=ctr[3])
            assert got[b, 0].tolist() == list(out), b
        # i0 offsets the block index, n_blocks past one wave of lanes
        got = bo.debug_rng(3, 1, 70, i0=2)
        assert np.array_equal(got, nr.blocks(kat, 3, 1, 70, i0=2))
    finally:
        bo.close()


# ---------------------------------------------------------------- 2. the draws against the host
@pytest.mark.parametrize("rname,dyn", CASES, ids=CASE_IDS)
def test_draws_equal_the_host(rname, dyn):
    """sigma = 1 returns z itself.  The second half draws with small sigmas and compares the x_init
    the launch planned with against the host's, which differs by the normals' libm distance
    carried through state_integrate."""
    R, lay, P, X, T0, bo = _start(rname, dyn)
    try:
        assert DEV_BAR_ULP * 2.0 ** -52 <= CAP_REL
        seeds, ndx = _seeds(), lay.ndx
        xs = bo.mpc_state()
        bo.mpc_set_noise(seeds, 1.0, 1.0)
        assert bo.mpc_get_noise() == {"state": True, "wrench": True}
        worst = 0
        for k in (0, 1, 5):
            bo.debug_mpc_prepare(k)
            z, w = bo.mpc_noise_state()
            for b in range(B):
                zh, wh, _ = bo.mpc_noise_host(k, int(seeds[b]), 1.0, 1.0)
                worst = max(worst, nr.ulp_distance(z[b], zh), nr.ulp_distance(w[b], wh))
            assert np.abs(z).max() < 6.0 and not _same(z[0], z[1]) and not _same(z[:, :6], w)
        print(f"{rname} {dyn}: normals, device against the host: {worst} ulp; bar {DEV_BAR_ULP} ulp")
        assert worst <= DEV_BAR_ULP, worst
        sig, wsig = _sigmas(ndx)
        bo.mpc_set_noise(seeds, sig, wsig)
        for k in (0, 3):
            bo.debug_mpc_prepare(k)
            z, w = bo.mpc_noise_state()
            xi = _x_init(bo, lay)
            for b in range(B):
                zh, wh, xih = bo.mpc_noise_host(k, int(seeds[b]), sig[b], wsig[b], None, xs[b])
                # sigma z: the normals' bar plus the product's own rounding on either side
                rel = (DEV_BAR_ULP + 1) * 2.0 ** -52
                assert np.all(np.abs(z[b] - zh) <= rel * np.abs(zh)) and np.all(np.abs(w[b] - wh) <= rel * np.abs(wh))
                assert np.abs(xi[b] - xih).max() <= 1e-13 and not _same(xi[b], xs[b]), (k, b)
        assert _same(bo.mpc_state(), xs)       # the true state is not touched
    finally:
        bo.close()


# ---------------------------------------------------------------- 3. drawn noise = fed noise
@pytest.mark.parametrize("rname,dyn", CASES, ids=CASE_IDS)
def test_drawn_noise_plans_like_fed_noise(rname, dyn):
    """Handle A draws; handle B gets A's drawn vectors through mpc_set_disturbance.  Both plan from
    the same x_init, parameters and iterate: the draw lanes add nothing but the values."""
    R, lay, P, X, T0, a = _start(rname, dyn)
    _, _, _, _, _, b = _start(rname, dyn)
    try:
        sig, _ = _sigmas(lay.ndx)
        a.mpc_set_noise(_seeds(), sig)
        assert a.mpc_get_noise() == {"state": True, "wrench": False}
        seen = []
        for k in (0, 1, 5):
            a.debug_mpc_prepare(k)
            z, w = a.mpc_noise_state()
            assert not w.any() and np.all(z != 0.0)
            b.mpc_set_disturbance(state_noise=z)
            b.debug_mpc_prepare(k)
            assert _same(_x_init(a, lay), _x_init(b, lay)), k
            assert _same(a.get_params(), b.get_params()) and _same(a.get_x(), b.get_x()), k
            assert not _same(_x_init(a, lay), a.mpc_state())
            seen.append(z)
        assert not _same(seen[0], seen[1]) and not _same(seen[1], seen[2])
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 4. rollout identity
def _window(batch=B):
    k0 = np.array([2, 2, 3, 0][:batch], dtype=np.int32)
    k1 = np.array([4, 3, 4, 0][:batch], dtype=np.int32)     # the last problem: an empty window
    W = np.random.default_rng(22).normal(0.0, 15.0, (batch, 6))
    return k0, k1, W


@pytest.mark.parametrize("push", [False, True], ids=["noise", "noise+push"])
def test_run_equals_stepwise_equals_host_fed(push):
    """(a) mpc_run(0, 5) with the random noise and wrench on; (b) the same stepped one by one, the
    drawn vectors read after every step; (c) no random draw, the host feeds (b)'s noise and the sum
    window + drawn wrench through mpc_set_disturbance before every step.  One log, three times.  The
    "aba" plant with contact consumes the wrench."""
    R, lay, P, X, T0, a = _start(plant=2, contact=True)
    _, _, _, _, _, b = _start(plant=2, contact=True)
    _, _, _, _, _, c = _start(plant=2, contact=True)
    try:
        seeds = _seeds()
        sig, wsig = _sigmas(lay.ndx)
        k0, k1, W = _window()
        for bo in (a, b):
            bo.mpc_set_noise(seeds, sig, wsig)
            if push:
                bo.mpc_set_push(k0, k1, W)
            bo.mpc_log_start(capacity=STEPS)
        _run(a, 0, STEPS)
        la = a.mpc_log_read()
        Z, Wd = [], []
        for k in range(STEPS):
            b.mpc_step(k)
            b.sync()
            z, w = b.mpc_noise_state()
            Z.append(z)
            Wd.append(w)
        lb = b.mpc_log_read()
        _logs_equal(la, lb)
        # the drawn part alone, from (a) once its run is read: no window, wrench = 0 + sigma_w z
        a.mpc_set_push()
        c.mpc_log_start(capacity=STEPS)
        for k in range(STEPS):
            a.debug_mpc_prepare(k)
            _, wn = a.mpc_noise_state()
            det = np.where(((k0 <= k) & (k < k1))[:, None], W, 0.0) if push else np.zeros((B, 6))
            assert _same(det + wn, Wd[k]), k          # the host adds the window itself
            c.mpc_set_disturbance(base_wrench=det + wn, state_noise=Z[k])
            c.mpc_step(k)
            c.sync()
        lc = c.mpc_log_read()
        _logs_equal(la, lc)
        assert np.all(np.isfinite(la["x_state"]))
        assert not _same(Z[0], Z[1]) and not _same(Wd[0], Wd[1]) and not _same(la["x_init"], la["x_state"])
    finally:
        a.close()
        b.close()
        c.close()


# ---------------------------------------------------------------- 5. slot and batch independence
def _start_rows(rows, plant=None):
    """A handle whose slot s holds synthetic problem rows[s], with that problem's own dt_min."""
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import DT_MIN, build_batch
    R = make_robot("go2")
    lay, P, X, XS, T0 = build_batch(R, "whole_body_rnea", N, B, 0)
    P = P.copy()
    P[:, lay.poff["dt_min"][0]] = DT_MIN * (1.0 + 0.1 * np.arange(B))
    rows = list(rows)
    bo = BatchedOCP(R, "whole_body_rnea", N, batch=len(rows), device=0, gait_type="trot", gait_period=0.8)
    bo.set_params(P[rows])
    bo.set_x(X[rows])
    bo.init_solver()
    bo.mpc_setup(XS[rows], T0[rows])
    if plant is not None:
        bo.mpc_set_plant("aba", plant)
    return lay, bo


def test_a_draw_does_not_depend_on_slot_or_batch():
    rows_a, rows_b = [0, 1, 2, 3], [2, 3, 0]
    lay, a = _start_rows(rows_a)
    _, b = _start_rows(rows_b)
    try:
        seeds = _seeds()
        sig, wsig = _sigmas(lay.ndx)
        a.mpc_set_noise(seeds[rows_a], sig[rows_a], wsig[rows_a])
        b.mpc_set_noise(seeds[rows_b], sig[rows_b], wsig[rows_b])
        for k in range(4):
            a.debug_mpc_prepare(k)
            b.debug_mpc_prepare(k)
            za, wa = a.mpc_noise_state()
            zb, wb = b.mpc_noise_state()
            xa, xb = _x_init(a, lay), _x_init(b, lay)
            for sb, g in enumerate(rows_b):             # problem 0: slot 0 of 4 and slot 2 of 3
                assert _same(za[g], zb[sb]) and _same(wa[g], wb[sb]) and _same(xa[g], xb[sb]), (k, g)
    finally:
        a.close()
        b.close()


def test_run_in_parts_equals_run_at_once():
    lay, a = _start_rows(range(B), plant=2)
    _, b = _start_rows(range(B), plant=2)
    try:
        sig, wsig = _sigmas(lay.ndx)
        for bo in (a, b):
            bo.mpc_set_noise(_seeds(), sig, wsig)
            bo.mpc_log_start(capacity=4)
        _run(a, 0, 4)
        _run(b, 0, 2)
        _run(b, 2, 2)
        _logs_equal(a.mpc_log_read(), b.mpc_log_read(), 4)
        za, wa = a.mpc_noise_state()
        zb, wb = b.mpc_noise_state()
        assert _same(za, zb) and _same(wa, wb) and _same(a.mpc_state(), b.mpc_state())
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 6. no re-capture
def test_set_noise_never_recaptures():
    R, lay, P, X, T0, bo = _start(plant=2)
    try:
        sig, wsig = _sigmas(lay.ndx)
        caps, drawn = [], []
        for k in range(6):
            if k == 2:    # on
                bo.mpc_set_noise(_seeds(), sig, wsig)
            if k == 3:    # new seeds, the wrench stream off
                bo.mpc_set_noise(_seeds(first=100), 2.0 * sig)
            if k == 4:    # off
                bo.mpc_set_noise(None)
            bo.mpc_step(k)
            bo.sync()
            caps.append(bo.mpc_graph_info())
            drawn.append(bo.mpc_noise_state())
        # step 0 eager (first sighting), step 1 captures, everything after replays
        assert [c["captures"] for c in caps] == [0, 1, 1, 1, 1, 1], caps
        assert [c["replays"] for c in caps] == [0, 1, 2, 3, 4, 5], caps
        assert all(c["eager_fallback"] == 0 for c in caps), caps
        assert not drawn[1][0].any() and not drawn[1][1].any()
        assert drawn[2][0].all() and drawn[2][1].all()
        assert drawn[3][0].all() and not drawn[3][1].any()      # the wrench stream went off: zeroed
        assert not _same(drawn[2][0], drawn[3][0]) and not drawn[5][1].any()
    finally:
        bo.close()


# ---------------------------------------------------------------- 7. off is off
def test_off_is_off():
    """A draws once (the launch of step 0 alone: x_init, the noise and the wrench buffers written),
    then switches the noise off: its log of the next steps is that of a handle that never had it,
    and the base wrench reads zero."""
    R, lay, P, X, T0, a = _start(plant=2, contact=True)
    _, _, _, _, _, b = _start(plant=2, contact=True)
    try:
        sig, wsig = _sigmas(lay.ndx)
        a.mpc_set_noise(_seeds(), sig, wsig)
        a.debug_mpc_prepare(0)
        z, w = a.mpc_noise_state()
        assert z.all() and w.all() and not _same(_x_init(a, lay), a.mpc_state())
        a.mpc_set_noise(None)
        assert a.mpc_get_noise() == {"state": False, "wrench": False}
        assert not a.mpc_noise_state()[1].any()
        for bo in (a, b):
            bo.mpc_log_start(capacity=3)
            _run(bo, 0, 3)
        la, lb = a.mpc_log_read(), b.mpc_log_read()
        _logs_equal(la, lb, 3)
        assert not a.mpc_noise_state()[1].any()
        assert _same(a.get_params(), b.get_params()) and _same(a.get_x(), b.get_x())
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 8. the interior-point solver
def test_interior_point_loop_draws_alike():
    R, lay, P, X, T0, a = _start(solver="fatrop")
    _, _, _, _, _, b = _start(solver="fatrop")
    try:
        sig, _ = _sigmas(lay.ndx)
        a.mpc_set_noise(_seeds(), sig)
        for bo in (a, b):
            bo.mpc_log_start(capacity=2)
        for k in range(2):
            a.mpc_step(k)
            a.sync()
            z, _ = a.mpc_noise_state()
            b.mpc_set_disturbance(state_noise=z)
            b.mpc_step(k)
            b.sync()
        la, lb = a.mpc_log_read(), b.mpc_log_read()
        _logs_equal(la, lb, 2)
        assert not _same(la["x_init"], la["x_state"]) and np.all(np.isfinite(la["x_state"]))
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 9. ownership
def test_ownership_of_the_noise_and_the_wrench():
    from pinoloco import _lib
    R, lay, P, X, T0, bo = _start(plant=2)
    try:
        sig, wsig = _sigmas(lay.ndx)
        seeds = _seeds()
        zero_z, W = np.zeros((B, lay.ndx)), np.ones((B, 6))
        bo.mpc_set_noise(seeds, sig, wsig)
        with pytest.raises(_lib.PinolocoError, match="random state noise"):
            bo.mpc_set_disturbance(state_noise=zero_z)
        with pytest.raises(_lib.PinolocoError, match="random base wrench"):
            bo.mpc_set_disturbance(base_wrench=W)
        bo.mpc_set_disturbance()                       # neither: allowed, the streams stay
        assert bo.mpc_get_noise() == {"state": True, "wrench": True}
        bo.mpc_set_noise(seeds, sig)                   # the wrench stream off: the static wrench is free again
        bo.mpc_set_disturbance(base_wrench=W)
        with pytest.raises(_lib.PinolocoError, match="random state noise"):
            bo.mpc_set_disturbance(base_wrench=W, state_noise=zero_z)
        with pytest.raises(_lib.PinolocoError, match="base_wrench of pl_mpc_set_disturbance"):
            bo.mpc_set_noise(seeds, sig, wsig)         # the static wrench is active: clear it first
        assert bo.mpc_get_noise() == {"state": True, "wrench": False}
        bo.mpc_set_noise(None)
        bo.mpc_set_disturbance(state_noise=zero_z)
        with pytest.raises(_lib.PinolocoError, match="state_noise of pl_mpc_set_disturbance"):
            bo.mpc_set_noise(seeds, sig)
        bo.mpc_set_noise(seeds, None, wsig)            # the other stream is free
        bo.mpc_set_disturbance()
        bo.mpc_set_push(0, 2, W)                       # a push schedule and the random wrench combine
        bo.mpc_set_noise(seeds, sig, wsig)
        bo.debug_mpc_prepare(1)
        _, w = bo.mpc_noise_state()
        _, wh, _ = bo.mpc_noise_host(1, int(seeds[0]), None, wsig[0], W[0])
        assert np.abs(w[0] - wh).max() <= 1e-12 and np.abs(w[0] - 1.0).max() > 1e-3
        with pytest.raises(_lib.PinolocoError, match="problem 1.*wrench_sigma\\[2\\]"):
            bad = wsig.copy()
            bad[1, 2] = -1.0
            bo.mpc_set_noise(seeds, sig, bad)
        assert bo.mpc_get_noise() == {"state": True, "wrench": True}    # a refusal leaves the settings
    finally:
        bo.close()
