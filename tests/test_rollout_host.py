"""The rollout log of the device MPC loop without a GPU: refusals, the row layout, the record
step on the host against the numpy twin (tests/rollout_ref.py), the public metrics struct against
the header, and the record step's host code under AddressSanitizer / UBSan in a stand-alone program.

pl_mpc_record_host runs the inline code k_mpc_record runs (csrc/record.h: row assembly, metrics
update, slot rule).  Bars: row contents, integer metrics, max_dz (a subtraction and an abs) and
max_viol (a comparison) exact; min_cz within 1e-15 (three multiplies / adds on values <= 1, where a
fused multiply-add may round once less than numpy)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rollout_ref as rr
from conftest import ROOT, make_robot

N = 6
SHAPES = [("go2", "whole_body_rnea"), ("b2g", "whole_body_rnea"), ("go2", "centroidal_vel")]


def _host(rname="go2", dyn="whole_body_rnea", batch=3):
    from pinoloco.ocp import BatchedOCP
    return BatchedOCP(make_robot(rname), dyn, N, batch=batch, device=-1)


def _err(fn, *a, **kw):
    from pinoloco import _lib
    with pytest.raises(_lib.PinolocoError) as e:
        fn(*a, **kw)
    return str(e.value)


# ---------------------------------------------------------------- refusals
def test_log_start_refusals():
    bo = _host()
    assert "negative" in _err(bo.mpc_log_start, capacity=-1)
    assert "every" in _err(bo.mpc_log_start, capacity=4, every=0)
    assert "not finite" in _err(bo.mpc_log_start, capacity=4, dz_tol=[0.1, np.nan, 0.1])
    assert "not finite" in _err(bo.mpc_log_start, capacity=4, cz_min=[0.5, 0.5, -np.inf])
    assert "does not fit" in _err(bo.mpc_log_start, capacity=2 ** 62)   # an error return, not a crash
    # valid arguments: the handle has no device
    assert "no device" in _err(bo.mpc_log_start, capacity=4, every=2, dz_tol=0.1, cz_min=0.5)
    assert "no device" in _err(bo.mpc_log_read)
    assert "no device" in _err(bo.mpc_metrics)
    assert "no device" in _err(bo.mpc_run, 0, 1)
    bo.mpc_log_stop()
    bo.close()


def test_set_push_refusals():
    bo = _host()
    W = np.ones((3, 6))
    assert "ends before" in _err(bo.mpc_set_push, [0, 3, 0], [1, 2, 1], W)
    assert "negative" in _err(bo.mpc_set_push, [0, -1, 0], [1, 2, 1], W)
    assert "negative" in _err(bo.mpc_set_push, [0, 0, 0], [1, 2, -1], W)
    Wn = W.copy()
    Wn[2, 4] = np.inf
    assert "not finite" in _err(bo.mpc_set_push, 0, 1, Wn)
    assert "together" in _err(bo.mpc_set_push, 0, None, W)
    assert "shape" in _err(bo.mpc_set_push, 0, 1, np.ones((3, 5)))
    # valid schedules, and switching off: the handle has no device
    assert "no device" in _err(bo.mpc_set_push, [1, 0, 0], [2, 0, 5], W)
    assert "no device" in _err(bo.mpc_set_push)
    bo.close()


def test_record_host_refusals():
    bo = _host(batch=1)
    step = _steps(bo, 1)[0]
    assert "cursor" in _err(bo.mpc_record_host, [step], 0.3, capacity=-1)
    assert "cursor" in _err(bo.mpc_record_host, [step], 0.3, capacity=1, every=0)
    assert "not finite" in _err(bo.mpc_record_host, [step], 0.3, dz_tol=np.nan)
    assert "shape" in _err(bo.mpc_record_host, [dict(step, u0=np.zeros(3))], 0.3)
    bo.close()


# ---------------------------------------------------------------- layout
@pytest.mark.parametrize("rname,dyn", SHAPES)
def test_log_sizes_on_a_host_handle(rname, dyn):
    bo = _host(rname, dyn)
    R, lay = bo.robot, bo.layout
    nx = 6 + R.nq if dyn == "centroidal_vel" else R.nq + R.nv
    assert lay.nx == nx
    nu0 = int(bo.node_table()[0, 1])
    assert nu0 == lay.nu[0]
    sz = bo.mpc_log_sizes()
    off, total = rr.offsets(nx, nu0)
    w = rr.widths(nx, nu0)
    for f in rr.FIELDS:
        assert (sz[f]["width"], sz[f]["offset"]) == (w[f], off[f]), f
    assert sz["row"] == total == 2 * nx + nu0 + 8 + 12 + 4
    assert (sz["capacity"], sz["every"], sz["recorded"], sz["dropped"]) == (0, 0, 0, 0)
    if rname == "b2g":  # the external-force frame and the arm widen u0
        assert nu0 > _host("go2", dyn).layout.nu[0]
    assert bo.LOG_FIELDS == rr.FIELDS and bo.LOG_STATS == rr.STATS
    bo.close()


# ---------------------------------------------------------------- record step against the twin
def _steps(bo, count, seed=0, qoff=0):
    """`count` hand-made steps of one problem: random rows whose base pose is set by the caller."""
    rng = np.random.default_rng(seed)
    sz = bo.mpc_log_sizes()
    nx, nu0 = sz["x_init"]["width"], sz["u0"]["width"]
    out = []
    for k in range(count):
        xs = rng.normal(size=nx) * 0.1
        xs[qoff + 2] = 0.30
        xs[qoff + 3:qoff + 7] = (0.0, 0.0, 0.0, 1.0)
        an = rng.normal(size=(4, 3))
        an[:, 2] = rng.integers(0, 2, 4)
        out.append({"k": 10 + k, "x_init": rng.normal(size=nx), "u0": rng.normal(size=nu0), "x_state": xs,
                    "stats": dict(status=1, admm_iters=25 + k, ls_accepted=1, ls_alpha=1.0, viol_max=1e-3 * (k + 1),
                                  f=rng.normal(), pri_res=1e-4, dua_res=1e-5),
                    "ground_f": rng.normal(size=(4, 3)), "anchors": an})
    return out


def _check(bo, steps, z_ref, capacity, every, dz_tol, cz_min, qoff=0):
    log, met, cur = bo.mpc_record_host(steps, z_ref, capacity, every, dz_tol, cz_min)
    keep, dropped = rr.slots(len(steps), capacity, every)
    assert (cur["seen"], cur["recorded"], cur["dropped"]) == (len(steps), len(keep), dropped)
    for f in rr.FIELDS:
        width = rr.row(steps[0])[f].size
        want = np.array([rr.row(steps[s])[f] for s in keep]).reshape(len(keep), width)
        assert log[f].shape == want.shape, f
        assert np.array_equal(log[f], want, equal_nan=True), f
    want = rr.metrics([s["k"] for s in steps], [s["x_state"] for s in steps],
                      [[s["stats"][k] for k in rr.STATS] for s in steps], z_ref, dz_tol, cz_min, qoff)
    rr.compare(met, want)
    return log, met, cur


@pytest.mark.parametrize("rname,dyn", SHAPES)
def test_record_host_branches(rname, dyn):
    bo = _host(rname, dyn, batch=1)
    qoff = 6 if dyn == "centroidal_vel" else 0
    z_ref = 0.30
    # a NaN in x_state (a velocity entry, then the height itself): first_nonfinite, not out, not in the extrema
    s = _steps(bo, 5, 1, qoff)
    s[1]["x_state"][qoff + 2] = 0.31
    s[2]["x_state"][-1] = np.nan
    s[2]["x_state"][qoff + 2] = 5.0   # would be out and the largest deviation if it counted
    s[3]["x_state"][qoff + 2] = np.inf
    s[3]["stats"]["viol_max"] = np.nan
    _, m, _ = _check(bo, s, z_ref, 5, 1, 0.5, 0.1, qoff)
    assert m["first_nonfinite"] == 12 and m["first_out"] == -1 and m["max_dz"] == abs(0.31 - z_ref)
    # out by height only (step 3 of 0..4), tilt well inside
    s = _steps(bo, 5, 2, qoff)
    s[3]["x_state"][qoff + 2] = 0.30 - 0.11
    _, m, _ = _check(bo, s, z_ref, 5, 1, 0.10, 0.5, qoff)
    assert m["first_out"] == 13 and m["first_nonfinite"] == -1 and m["min_cz"] == 1.0
    # out by tilt only: qx = sin(40 deg) -> c_z = cos(80 deg) = 0.17 < 0.5
    s = _steps(bo, 5, 3, qoff)
    a = np.deg2rad(40.0)
    s[2]["x_state"][qoff + 3:qoff + 7] = (np.sin(a), 0.0, 0.0, np.cos(a))
    s[4]["x_state"][qoff + 3:qoff + 7] = (0.0, np.sin(a / 2), 0.0, np.cos(a / 2))
    _, m, _ = _check(bo, s, z_ref, 5, 1, 0.10, 0.5, qoff)
    assert m["first_out"] == 12 and m["max_dz"] == 0.0 and abs(m["min_cz"] - np.cos(2 * a)) < 1e-12
    # the same rows with NULL tolerances: never out; one tolerance alone
    _, m, _ = _check(bo, s, z_ref, 5, 1, None, None, qoff)
    assert m["first_out"] == -1
    _, m, _ = _check(bo, s, z_ref, 5, 1, 0.10, None, qoff)
    assert m["first_out"] == -1
    _, m, _ = _check(bo, s, z_ref, 5, 1, None, 0.9, qoff)
    assert m["first_out"] == 12
    # status != 1 and a rejected line search
    s = _steps(bo, 5, 4, qoff)
    s[0]["stats"].update(status=-2)
    s[2]["stats"].update(status=2, ls_accepted=0, ls_alpha=0.0)
    s[4]["stats"].update(ls_accepted=0)
    _, m, _ = _check(bo, s, z_ref, 5, 1, None, None, qoff)
    assert (m["n_not_solved"], m["n_ls_rejected"], m["steps"]) == (2, 2, 5) and m["max_viol"] == 1e-3 * 5
    # every = 2 with capacity = 2 over 5 steps: steps 0 and 2, one dropped, metrics of all 5
    log, m, cur = _check(bo, s, z_ref, 2, 2, None, None, qoff)
    assert cur == {"seen": 5, "recorded": 2, "dropped": 1} and m["steps"] == 5
    assert np.array_equal(log["x_state"], np.array([s[0]["x_state"], s[2]["x_state"]]))
    # metrics only
    log, m, cur = _check(bo, s, z_ref, 0, 1, None, None, qoff)
    assert cur == {"seen": 5, "recorded": 0, "dropped": 5} and log["u0"].shape[0] == 0 and m["steps"] == 5
    # without contact buffers: zero forces, no anchor
    s = [{k: v for k, v in st.items() if k not in ("ground_f", "anchors")} for st in _steps(bo, 2, 5, qoff)]
    log, _, _ = _check(bo, s, z_ref, 2, 1, None, None, qoff)
    assert not log["ground_f"].any() and not log["anchor_active"].any()
    bo.close()


# ---------------------------------------------------------------- struct layout
def test_metrics_struct_matches_header(tmp_path):
    from pinoloco import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    names = [k for k, _ in _lib.MpcMetrics._fields_]
    body = 'printf("size %zu\\n", sizeof(pl_mpc_metrics_t));' + "".join(
        f'printf("{f} %zu\\n", offsetof(pl_mpc_metrics_t, {f}));' for f in names)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "pinoloco.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.split("\n") if line)
    assert int(out["size"]) == C.sizeof(_lib.MpcMetrics) == 48
    for f in names:
        assert int(out[f]) == getattr(_lib.MpcMetrics, f).offset, f


# ---------------------------------------------------------------- sanitized stand-alone program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and shutil.which(hipcc) is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("rollout") / "record_host"
    # host code only: the sanitizers are host options (-Xarch_host), no device code is instrumented
    cmd = [hipcc, "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Wno-unused-result", "-Wno-comment",
           "-I", os.path.join(ROOT, "pino-locoman_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "record_host.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return str(out)


@pytest.mark.slow
@pytest.mark.parametrize("capacity,every", [(5, 1), (2, 2), (0, 1)])
def test_record_step_is_clean_under_sanitizers(program, tmp_path, capacity, every):
    """The program's rows, metrics and cursor equal the library's (exactly: one code, two builds
    for the host; min_cz at the twin's bar, the builds may contract differently)."""
    bo = _host("b2g", "whole_body_rnea", batch=1)
    sz = bo.mpc_log_sizes()
    nx, nu0 = sz["x_init"]["width"], sz["u0"]["width"]
    s = _steps(bo, 5, 7)
    s[1]["x_state"][2] = 0.42
    s[2]["x_state"][5] = np.nan
    s[3]["stats"].update(status=-2, ls_accepted=0)
    z_ref, dz_tol, cz_min = 0.30, 0.10, 0.5
    path = tmp_path / "in.bin"
    with open(path, "wb") as f:
        f.write(np.array([nx, nu0, 4, 0, capacity, every, len(s), 3], dtype=np.int32).tobytes())
        f.write(np.array([z_ref, dz_tol, cz_min]).tobytes())
        for st in s:
            for a in ([st["k"]], st["x_init"], st["u0"], [st["stats"][k] for k in rr.STATS], st["x_state"],
                      st["ground_f"], st["anchors"]):
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    got = np.array([float(v) for v in r.stdout.split()])
    log, met, cur = bo.mpc_record_host(s, z_ref, capacity, every, dz_tol, cz_min)
    nrow = cur["recorded"] * sz["row"]
    assert got.shape == (nrow + 11,)
    rows = got[:nrow].reshape(cur["recorded"], sz["row"])
    for f in rr.FIELDS:
        assert np.array_equal(rows[:, sz[f]["offset"]:sz[f]["offset"] + sz[f]["width"]], log[f], equal_nan=True), f
    rr.compare(dict(zip(("steps", "first_nonfinite", "first_out", "n_not_solved", "n_ls_rejected", "max_dz", "min_cz",
                         "max_viol"), got[nrow:nrow + 8])), met)
    assert got[nrow + 8:].tolist() == [cur["seen"], cur["recorded"], cur["dropped"]]
    assert met["first_nonfinite"] == 12 and met["first_out"] == 11
    bo.close()
