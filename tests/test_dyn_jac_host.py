"""Jacobians of the Dynamics plugin's point functions (PointFunction.jacobian over pl_dyn_jac,
csrc/dyn_jac.h) on a host handle (device = -1), against the oracle and the project's own values.

1. Complex-step parity, every supported function, Go2 (rnea W = 66) and B2G (external-force
   frame, nf = 15, the arm's relative_to_base velocity), at the three golden points and a fourth
   with the base yawed 170 degrees (tests/dyn_jac_ref.py).  Bars: 1e-12 of max(1, max |block|),
   1e-10 for the solve-based functions (aba, the base accelerations, base_vel_cv): the bars of the
   same functions' values in tests/test_dynamics.py.  Measured worst cases over both robots and all
   four points: rnea / nle / gaps_wb 8.7e-16, frame_pos 2.2e-16, frame_vel 3.1e-16, frame_vel
   relative to the base 4.9e-16, com_dyn 7.4e-16, gaps_cv 6.6e-16, com 5.6e-16, gaps_ca 5.6e-15,
   base_acc_wb 9.1e-15, base_vel_cv 8.4e-15, base_acc_cv 8.9e-15, aba 4.0e-12 -- no bar had to be
   widened.  The reference of base_acc_cv is the oracle's arithmetic-only form of the same
   expression (rbd.base_acc_ca): rbd.base_acc_cv takes dA v from a complex step of its own, which
   an outer complex step in q or v cannot pass through.
2. Identities with the value functions the project already pins (crba, frame Jacobian, centroidal map).
3. Every single-input wrt equals the full Jacobian's block, and with_value equals pl_dyn_eval,
   bit for bit.  4. Batches equal point-by-point calls; 1-D inputs broadcast.
5. Every refusal names the function.  6. tests/native/dyn_jac_host.cpp, the same columns in a
   stand-alone program built with the address and undefined-behaviour sanitizers, prints the
   blocks the host handle returns, bit for bit.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dyn_jac_ref as dr
from conftest import ROOT


def _rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(got))
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


@pytest.fixture(scope="module", params=dr.ROBOTS)
def setup(request):
    name = request.param
    P, R, frames = dr.points(name)
    cs, _ = dr.cases(name)
    return name, P, R, frames, cs


def _args(P, keys, b):
    return [P[k][b] for k in keys]


def test_complex_step_parity(setup):
    name, P, R, frames, cs = setup
    for cname, pf, keys, cfg in cs:
        fun, Mo = dr.oracle_fn(cname, R, frames)
        bar = 1e-10 if cname in dr.SOLVE else 1e-12
        worst = 0.0
        for b in range(4):
            args = _args(P, keys, b)
            ref = dr.complex_step_blocks(fun, Mo, args, cfg)
            got = pf.jacobian()(*args)
            assert len(got) == len(ref)
            worst = max([worst] + [_rel(g, r) for g, r in zip(got, ref)])
        print(f"{name} {cname}: worst {worst:.2e} (bar {bar:.0e})")
        assert worst <= bar, (name, cname, worst)


def test_identities(setup):
    from pinoloco.dynamics import DynamicsCentroidalVel, DynamicsWholeBodyAcc, DynamicsWholeBodyTorque
    name, P, R, frames, cs = setup
    ext = R.ext_force_frame
    wb, acc, cv = DynamicsWholeBodyTorque(R), DynamicsWholeBodyAcc(R), DynamicsCentroidalVel(R)
    for b in range(4):
        q, v, a, f, h, tj = (P[k][b] for k in ("q", "v", "a", "f", "h", "tau_j"))
        Jq, Jv, Ja, Jf = wb.rnea_dynamics(ext).jacobian()(q, v, a, f)
        Mq = wb.crba()(q)
        assert _rel(Ja, Mq) <= 1e-10
        for e, fid in enumerate(frames):
            assert _rel(Jf[:, 3 * e:3 * e + 3], -wb.frame_jacobian(fid)(q)[:3].T) <= 1e-10
        foot = R.foot_frames[0]
        assert _rel(wb.get_frame_velocity(foot).jacobian(wrt=[1])(q, v)[0], wb.frame_jacobian(foot)(q)) <= 1e-12
        Gh, _, Gv = cv.dynamics_gaps().jacobian()(h, q, v)
        assert _rel(Gv, cv.centroidal_map()(q)) <= 1e-12
        assert _rel(Gh, -R.mass * np.eye(6)) <= 1e-12
        At = wb.aba_dynamics(ext).jacobian(wrt=[2])(q, v, tj, f)[0]
        assert _rel(At, np.linalg.inv(Mq)[:, 6:]) <= 1e-10
        for g, r in zip(acc.dynamics_gaps(ext).jacobian()(q, v, a, f), (Jq, Jv, Ja, Jf)):
            assert _rel(g, r[:6]) <= 1e-12
        z = np.zeros(R.nv)
        N = wb.nonlinear_effects().jacobian()(q, v)
        Z = wb.rnea_dynamics(ext).jacobian(wrt=[0, 1])(q, v, z, np.zeros_like(f))
        assert _rel(N[0], Z[0]) <= 1e-12 and _rel(N[1], Z[1]) <= 1e-12


def test_wrt_blocks_and_value_bitwise(setup):
    name, P, R, frames, cs = setup
    for cname, pf, keys, cfg in cs:
        args = _args(P, keys, 1)
        full = pf.jacobian(with_value=True)(*args)
        assert np.array_equal(full[0], pf(*args)), cname
        for k in range(len(keys)):
            one = pf.jacobian(wrt=[k])(*args)
            assert len(one) == 1 and np.array_equal(one[0], full[1 + k]), (cname, k)
        if len(keys) > 2:
            two = pf.jacobian(wrt=(2, 0))(*args)  # blocks come in input order
            assert np.array_equal(two[0], full[1]) and np.array_equal(two[1], full[3]), cname


def test_batches(setup):
    name, P, R, frames, cs = setup
    for cname, pf, keys, cfg in cs:
        args = [P[k] for k in keys]
        val, *blocks = pf.jacobian(with_value=True)(*args)
        assert val.shape == (4, pf.out_len)
        for b in range(4):
            one = pf.jacobian(with_value=True)(*_args(P, keys, b))
            assert one[0].shape == (pf.out_len,)
            assert np.array_equal(one[0], val[b]), cname
            for g, r in zip(blocks, one[1:]):
                assert g.shape[0] == 4 and np.array_equal(g[b], r), (cname, b)
        if len(keys) > 1:  # a 1-D last input broadcasts against the batch
            mixed = pf.jacobian()(*args[:-1], args[-1][0])
            for b in range(4):
                want = pf.jacobian()(*[a[b] for a in args[:-1]], args[-1][0])
                assert all(np.array_equal(m[b], w) for m, w in zip(mixed, want)), cname


def test_sizes():
    for name in dr.ROBOTS:
        cs, R = dr.cases(name)
        nq, nv, nj = R.nq, R.nv, R.nj
        nf = 12 + (3 if R.ext_force_frame is not None else 0)
        want = dict(rnea=[nv, nv, nv, nf], aba=[nv, nv, nj, nf], nle=[nv, nv], frame_pos=[nv], frame_vel=[nv, nv],
                    frame_vel_rel=[nv, nv], gaps_wb=[nv, nv, nv, nf], base_acc_wb=[nv, nv, nj, nf], com_dyn=[nv, nf],
                    base_vel_cv=[6, nv, nj], base_acc_cv=[nv, nv, nj, nf], gaps_cv=[6, nv, nv], com=[nv],
                    gaps_ca=[nv, nv, nv, nf])
        for cname, pf, keys, cfg in cs:
            tan, out_len = pf.jacobian_sizes()
            assert tan == want[cname] and out_len == pf.out_len, (name, cname, tan)
            assert pf.in_len[cfg] == nq and tan[cfg] == nv
    assert sum(want["rnea"]) == 87  # B2G: one full tile and 23 lanes; Go2 has 66


def test_refusals():
    from pinoloco import _lib
    from pinoloco.dynamics import FN, Dynamics, DynamicsCentroidalVel, DynamicsWholeBodyTorque
    P, R, frames = dr.points("go2")
    q, v, a, f = (P[k][0] for k in ("q", "v", "a", "f"))
    wb, cv = DynamicsWholeBodyTorque(R), DynamicsCentroidalVel(R)
    x = np.concatenate([q, v])
    xc = np.concatenate([np.zeros(6), q])
    refused = [("crba", wb.crba(), (q,)), ("frame_jac", wb.frame_jacobian(R.foot_frames[0]), (q,)),
               ("cmap", wb.centroidal_map(), (q,)),
               ("integrate_wb", wb.state_integrate(), (x, np.zeros(2 * R.nv))),
               ("difference_wb", wb.state_difference(), (x, x)),
               ("integrate_cv", cv.state_integrate(), (xc, np.zeros(6 + R.nv))),
               ("difference_cv", cv.state_difference(), (xc, xc))]
    for fname, pf, args in refused:
        with pytest.raises(_lib.PinolocoError, match=fname):
            pf.jacobian()(*args)
    rnea = wb.rnea_dynamics()
    with pytest.raises(_lib.PinolocoError, match="rnea"):  # wrt == 0
        rnea.jacobian(wrt=[])(q, v, a, f)
    with pytest.raises(_lib.PinolocoError, match="frame_pos"):  # a wrt bit on an input it does not take
        wb.get_frame_position(R.foot_frames[0]).jacobian(wrt=[1])(q)
    with pytest.raises(_lib.PinolocoError, match="frame_vel"):  # what pl_dyn_eval refuses: no base_link on Go2
        Dynamics(R).get_frame_velocity(R.foot_frames[0], relative_to_base=True).jacobian()(q, v)
    L, h = _lib.lib(), rnea._h.h
    jac = np.zeros(R.nv * 66)
    d = _lib.dptr
    for bad in ((d(q), d(v), None, d(f), None, d(jac)),  # a missing input
                (d(q), d(v), d(a), d(f), None, None)):   # jac == NULL
        assert L.pl_dyn_jac(h, FN["rnea"], 1, -1, 0, 15, *bad) != 0
        assert "rnea" in L.pl_last_error().decode()
    assert L.pl_dyn_jac(h, FN["rnea"], 1, -1, 1, 15, d(q), d(v), d(a), d(f), None, d(jac)) != 0  # no ext frame
    assert "rnea" in L.pl_last_error().decode()
    assert L.pl_dyn_jac(h, FN["frame_pos"], 1, 99999, 0, 1, d(q), None, None, None, None, d(jac)) != 0
    assert "frame_pos" in L.pl_last_error().decode()
    assert L.pl_dyn_jac(h, FN["rnea"], 0, -1, 0, 15, d(q), d(v), d(a), d(f), None, d(jac)) == 0  # batch == 0
    with pytest.raises(_lib.PinolocoError, match="rnea"):  # device pointers on a host handle
        rnea.jacobian_device(1, [8, 8, 8, 8], 8)


# ---- the stand-alone program under the sanitizers
FRAME_KIND = {"frame_pos": 1, "frame_vel": 1, "frame_vel_rel": 2}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and shutil.which(hipcc) is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("dynjac") / "dyn_jac_host"
    # host code only: the sanitizers are host options (-Xarch_host), no device code is instrumented
    cmd = [hipcc, "-std=c++17", "-O3", "-x", "hip", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Wno-unused-result", "-Wno-comment",
           "-I", os.path.join(ROOT, "pino-locoman_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "dyn_jac_host.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return str(out)


@pytest.mark.slow
@pytest.mark.parametrize("name,N", [("go2", 20), ("b2g", 50)])
def test_sanitized_program_prints_the_same_blocks(program, tmp_path, name, N):
    from pinoloco import _lib
    from pinoloco.dynamics import FN
    from pinoloco.ocp import BatchedOCP
    P, R, frames = dr.points(name)
    cs, _ = dr.cases(name)
    bo = BatchedOCP(R, "whole_body_rnea", N, batch=1, device=-1)  # its tables carry the plugin's contact frames
    L = _lib.lib()
    sizes = (C.c_int * 2)()
    _lib.check(L.pl_debug_consts(bo.h, None, None, sizes))
    mb, ob = C.create_string_buffer(sizes[0]), C.create_string_buffer(sizes[1])
    _lib.check(L.pl_debug_consts(bo.h, mb, ob, None))
    bo.close()
    want = []
    path = tmp_path / "in.bin"
    with open(path, "wb") as f:
        f.write(np.array([sizes[0], sizes[1], 2 * len(cs)], dtype=np.int32).tobytes() + mb.raw + ob.raw)
        for b, (cname, pf, keys, cfg) in [(b, c) for b in (0, 3) for c in cs]:
            args = _args(P, keys, b)
            wrt = (1 << len(keys)) - 1
            f.write(np.array([FN[pf.name], pf._flags, FRAME_KIND.get(cname, 0), wrt], dtype=np.int32).tobytes())
            for a in args:
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
            want.append(np.concatenate(pf.jacobian()(*args), axis=1).ravel())
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    got = np.array([float(t) for t in r.stdout.split()])
    want = np.concatenate(want)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.abs(got - want).max()
