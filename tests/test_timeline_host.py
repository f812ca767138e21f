"""Gait and command timelines of the device MPC loop without a GPU: pl_mpc_timeline_host against the
numpy twin (tests/timeline_ref.py), the refusals of pl_mpc_set_timeline, the parameters the step
must not touch, and the step's host code under AddressSanitizer / UBSan in a stand-alone program.

pl_mpc_timeline_host runs the inline code k_mpc_prepare runs with a timeline (csrc/timeline.h).
Bars: the governing keyframe, the gait scalars, the schedules, the warm start and held or clamped
commands exact (bit for bit); a ramped command within 2**-51 (|c_s| + |c_{s+1}|) per component, one
product rounding plus one sum rounding of c_s + a (c_{s+1} - c_s), which also covers a build that
fuses the two on one side only.  Every clock here is >= 0.

Shapes: Go2 and B2G (external-force and arm fields) whole_body_rnea, N = 6, synthetic problems,
k = 0..12."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import timeline_ref as tr
from conftest import ROOT, make_robot

N = 6
KS = range(13)


def _host(rname="go2", dyn="whole_body_rnea", batch=1):
    from pinoloco.ocp import BatchedOCP
    return BatchedOCP(make_robot(rname), dyn, N, batch=batch, device=-1)


def _problem(rname, dyn="whole_body_rnea", gidx=0):
    """(robot, layout, p, x, t0) of synthetic problem gidx, x an iterate with every entry non-zero."""
    from pinoloco.synthetic import build_batch
    R = make_robot(rname)
    lay, P, X, _, T0 = build_batch(R, dyn, N, 1, gidx)
    x = X[0] + 0.5 + np.arange(lay.n) * 1e-3
    return R, lay, P[0], x, float(T0[0])


def _err(fn, *a, **kw):
    from pinoloco import _lib
    with pytest.raises(_lib.PinolocoError) as e:
        fn(*a, **kw)
    return str(e.value)


def kf(k_start, gait, period, vel=0.0, ramp=0, t_shift=0.0, ext=(0, 0, 0), arm=(0, 0, 0)):
    from pinoloco.ocp import BatchedOCP
    v = np.array([vel, 0.3 * vel, 0.0, 0.0, 0.0, -0.7 * vel])
    return BatchedOCP.keyframe(k_start, gait, period, v, ext, arm, ramp, t_shift)


# before the first keyframe (k = 0, 1: clamped, and ramp = 1 there still holds), k equal to every
# k_start, a ramp across a one-step gap (2 -> 3), a ramp over thirds (6 -> 9), ramp = 1 on the
# last keyframe (holds), all three gaits, t_shift != 0
MIXED = [kf(2, "trot", 0.8, 0.1, ramp=1),
         kf(3, "walk", 0.6, 0.25, t_shift=0.05),
         kf(6, "stand", 0.5, 0.3, ramp=1, t_shift=0.0125),
         kf(9, "trot", 0.7, -0.2, ramp=1, t_shift=0.1)]
# the same with the external-force and arm fields moving (B2G)
MIXED_EE = [kf(0, "walk", 0.9, 0.1, ramp=1, ext=(1.0, -2.0, -20.0), arm=(0.01, 0.0, -0.03)),
            kf(7, "trot", 0.8, 0.3, ramp=1, t_shift=0.2, ext=(0.0, 3.0, -10.0), arm=(-0.02, 0.05, 0.0)),
            kf(8, "stand", 0.4, 0.0, ext=(0.5, 0.5, 0.5), arm=(0.1, 0.1, 0.1))]
SINGLE = [kf(5, "walk", 0.6, 0.15, ramp=1, t_shift=0.3)]
TIMELINES = {"mixed": ("go2", MIXED), "mixed-ee": ("b2g", MIXED_EE), "single-clamped": ("go2", SINGLE),
             "go2-ignores-ee": ("go2", MIXED_EE)}


def _structured(keys, n_key, garbage=True):
    """keys as a structured array [n_key] with the padding full of NaN and out-of-range integers."""
    from pinoloco import _lib
    bo = _host()
    arr, cnt = bo._keyframes([keys], 1)
    bo.close()
    out = np.zeros(n_key, dtype=_lib.timeline_dtype)
    out[:cnt[0]] = arr[0]
    if garbage:
        for j in range(cnt[0], n_key):
            out[j]["k_start"], out[j]["gait_type"], out[j]["ramp"] = -7 if j % 2 else 2 ** 31 - 1, 99, -3
            out[j]["gait_period"], out[j]["t_shift"] = np.nan, np.inf
            out[j]["base_vel_des"], out[j]["ext_force_des"], out[j]["arm_vel_des"] = np.nan, -np.inf, np.nan
    return out, int(cnt[0])


# ---------------------------------------------------------------- the step against the twin
@pytest.mark.parametrize("name", sorted(TIMELINES))
def test_timeline_host_equals_the_twin(name):
    rname, keys = TIMELINES[name]
    R, lay, p0, x0, t0 = _problem(rname)
    bo = _host(rname)
    worst = 0.0
    segs = []
    for k in KS:
        want = tr.prepare(R, lay, keys, k, t0, p0, x0)
        p, x, seg = bo.mpc_timeline_host(k, t0, keys, p0, x0)
        assert seg == want["seg"], (k, seg, want["seg"])
        worst = max(worst, tr.compare(p, want, lay, R, who=(name, k)))
        assert np.array_equal(x.view(np.uint64), want["x"].view(np.uint64)), k
        if k == 0:
            assert np.array_equal(x, x0)   # step 0 keeps the initial guess
        else:
            assert not np.array_equal(x, x0)
        # without x: the parameters alone, the same ones
        p2, x2, _ = bo.mpc_timeline_host(k, t0, keys, p0)
        assert x2 is None and np.array_equal(p2.view(np.uint64), p.view(np.uint64))
        segs.append(seg)
    print(f"{name}: segments {segs}, worst ramped command deviation {worst:.3f} of its bar")
    assert segs == [tr.segment(keys, k) for k in KS] and segs[0] == 0 and segs[-1] == len(keys) - 1
    bo.close()


def test_segments_and_ramp_values_of_the_mixed_timeline():
    """The hand-made cases, spelled out: clamping before the first keyframe, k equal to a k_start,
    the one-step ramp, the ramp in thirds, the holding last keyframe."""
    R, lay, p0, x0, t0 = _problem("go2")
    bo = _host()
    o = lay.poff["base_vel_des"][0]
    vx = {}
    for k in KS:
        p, _, seg = bo.mpc_timeline_host(k, t0, MIXED, p0)
        vx[k] = (seg, p[o], p[lay.poff["n_contacts"][0]], p[lay.poff["swing_period"][0]])
    assert [vx[k][0] for k in KS] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3]
    assert vx[0][1] == vx[1][1] == vx[2][1] == 0.1          # clamped, then a = 0 of the one-step ramp
    assert vx[3][1] == vx[5][1] == 0.25                      # held
    assert vx[6][1] == 0.3 and abs(vx[7][1] - (0.3 - 0.5 / 3)) <= 2.0 ** -51 * 0.5   # thirds towards -0.2
    assert vx[9][1] == vx[12][1] == -0.2                     # ramp = 1 on the last keyframe holds
    assert [vx[k][2] for k in (0, 3, 6, 9)] == [2.0, 3.0, 4.0, 2.0]
    assert [vx[k][3] for k in (0, 3, 6, 9)] == [0.4, 0.15, 0.5, 0.35]
    bo.close()


def test_padding_is_never_read():
    """count < n_key with NaN and out-of-range integers in the padding: the same bits as the plain
    list, for every k."""
    R, lay, p0, x0, t0 = _problem("b2g")
    bo = _host("b2g")
    arr, cnt = _structured(MIXED_EE, 6)
    assert cnt == 3 and np.isnan(arr[4]["gait_period"]) and arr[5]["gait_type"] == 99
    for k in KS:
        p, x, seg = bo.mpc_timeline_host(k, t0, MIXED_EE, p0, x0)
        pg, xg, sg = bo.mpc_timeline_host(k, t0, arr, p0, x0, count=cnt)
        assert sg == seg and np.array_equal(pg.view(np.uint64), p.view(np.uint64))
        assert np.array_equal(xg.view(np.uint64), x.view(np.uint64))
    # the garbage is refused once it is inside the count
    assert "keyframe 3" in _err(bo.mpc_timeline_host, 0, t0, arr, p0, count=4)
    bo.close()


def test_go2_never_writes_the_ee_parameters_nor_outside_p():
    """Go2 has no external-force and no arm frame: their parameter slots keep a guard pattern, and so
    do the doubles before and after p (the C call on a guarded buffer)."""
    from pinoloco import _lib
    R, lay, p0, x0, t0 = _problem("go2")
    bo = _host()
    arr, cnt = bo._keyframes([MIXED_EE], 1)
    guard, pad = -1234.5, 8
    for k in (0, 4, 7, 12):
        buf = np.full(lay.np + 2 * pad, guard)
        buf[pad:pad + lay.np] = p0
        for name in ("ext_force_des", "arm_vel_des"):
            o, w = lay.poff[name]
            buf[pad + o:pad + o + w] = guard
        inner = buf[pad:pad + lay.np]
        before = inner.copy()
        ptr = C.cast(buf.ctypes.data + 8 * pad, C.POINTER(C.c_double))
        seg = C.c_int()
        _lib.check(_lib.lib().pl_mpc_timeline_host(bo.h, k, t0, arr.ctypes.data_as(C.POINTER(_lib.Keyframe)), int(cnt[0]),
                                                   ptr, None, C.byref(seg)))
        assert np.all(buf[:pad] == guard) and np.all(buf[pad + lay.np:] == guard)
        for name in ("ext_force_des", "arm_vel_des"):
            o, w = lay.poff[name]
            assert np.all(inner[o:o + w] == guard), (k, name)
        # what may change: commands, gait scalars, schedules; nothing else
        may = np.zeros(lay.np, dtype=bool)
        for name in ("base_vel_des", "n_contacts", "swing_period", "contact_schedule", "swing_schedule"):
            o, w = lay.poff[name]
            may[o:o + w] = True
        assert np.array_equal(inner[~may], before[~may])
        assert not np.array_equal(inner[may], before[may])
    bo.close()


# ---------------------------------------------------------------- refusals
def _bad(keys, j, **kw):
    out = [dict(k) for k in keys]
    out[j].update(kw)
    return out


def test_set_timeline_refusals():
    """Every refusal comes back with the problem and keyframe in the message, before the handle's
    device is asked for; a valid timeline then meets the missing device."""
    from pinoloco import _lib
    bo = _host(batch=2)
    good = [MIXED, SINGLE]
    cases = [(0, dict(k_start=-1), "negative"),
             (2, dict(k_start=3), "does not increase"),
             (2, dict(k_start=2), "does not increase"),
             (1, dict(gait_type=3), "gait_type"),
             (1, dict(gait_type=-1), "gait_type"),
             (3, dict(gait_period=0.0), "gait_period"),
             (3, dict(gait_period=-0.5), "gait_period"),
             (3, dict(gait_period=np.nan), "gait_period"),
             (3, dict(gait_period=np.inf), "gait_period"),
             (0, dict(t_shift=np.nan), "t_shift"),
             (2, dict(ramp=2), "ramp"),
             (2, dict(ramp=-1), "ramp"),
             (1, dict(base_vel_des=[0, 0, np.inf, 0, 0, 0]), "base_vel_des[2]"),
             (1, dict(ext_force_des=[np.nan, 0, 0]), "ext_force_des[0]"),
             (1, dict(arm_vel_des=[0, 0, -np.inf]), "arm_vel_des[2]")]
    for j, change, what in cases:
        keys = _bad(MIXED, j, **change)
        msg = _err(bo.mpc_set_timeline, [SINGLE, keys])
        assert what in msg and "problem 1" in msg and f"keyframe {j}" in msg, (what, msg)
        # the one-problem host step validates alike
        assert what in _err(bo.mpc_timeline_host, 0, 0.0, keys, np.zeros(bo.np))
    arr = np.zeros((2, 65), dtype=_lib.timeline_dtype)
    assert "n_key 65" in _err(bo.mpc_set_timeline, arr)
    assert "n_key 0" in _err(bo.mpc_set_timeline, arr[:, :0])
    a4, _ = _structured(MIXED, 4, garbage=False)
    arr = np.stack([a4, a4])
    assert "count 0" in _err(bo.mpc_set_timeline, arr, count=[4, 0])
    assert "count 5" in _err(bo.mpc_set_timeline, arr, count=[5, 4])
    assert "count" in _err(bo.mpc_set_timeline, [MIXED, []])
    assert "unknown" in _err(bo.mpc_set_timeline, [MIXED, [dict(SINGLE[0], gait_type="gallop")]])
    assert "expected 2 lists" in _err(bo.mpc_set_timeline, [MIXED])
    # valid timelines, and switching off: the handle has no device
    assert "no device" in _err(bo.mpc_set_timeline, good)
    assert "no device" in _err(bo.mpc_set_timeline, arr, count=[4, 1])
    assert "no device" in _err(bo.mpc_set_timeline, None)
    assert "no device" in _err(bo.mpc_timeline_state)
    assert "no device" in _err(bo.debug_mpc_prepare, 0)
    assert bo.mpc_get_timeline() == {"on": False, "n_key": 0}
    assert _lib.lib().pl_version() >= 2
    bo.close()


def test_keyframe_struct_matches_header(tmp_path):
    from pinoloco import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    names = [k for k, _ in _lib.Keyframe._fields_]
    body = 'printf("size %zu\\n", sizeof(pl_mpc_keyframe));' + "".join(
        f'printf("{f} %zu\\n", offsetof(pl_mpc_keyframe, {f}));' for f in names)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "pinoloco.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.split("\n") if line)
    assert int(out["size"]) == C.sizeof(_lib.Keyframe) == _lib.timeline_dtype.itemsize == 128
    for f in names:
        assert int(out[f]) == getattr(_lib.Keyframe, f).offset == _lib.timeline_dtype.fields[f][1], f


# ---------------------------------------------------------------- sanitized stand-alone program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and shutil.which(hipcc) is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("timeline") / "timeline_host"
    # host code only: the sanitizers are host options (-Xarch_host), no device code is instrumented
    cmd = [hipcc, "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Wno-unused-result", "-Wno-comment",
           "-I", os.path.join(ROOT, "pino-locoman_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "timeline_host.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return str(out)


@pytest.mark.slow
@pytest.mark.parametrize("name", ["mixed-ee", "single-clamped", "go2-ignores-ee"])
def test_timeline_step_is_clean_under_sanitizers(program, tmp_path, name):
    """The program holds exactly `count` keyframes, np parameters and n iterate entries on the heap,
    so a padding read or a stray write is a sanitizer report; its output equals the twin's at the
    bars above (padding and clamp cases: k before, at and past every k_start)."""
    rname, keys = TIMELINES[name]
    R, lay, p0, x0, t0 = _problem(rname)
    bo = _host(rname)
    arr, cnt = bo._keyframes([keys], 1)
    po = [lay.poff[k][0] for k in ("x_init", "dt_min", "dt_max", "contact_schedule", "swing_schedule", "n_contacts",
                                   "swing_period", "base_vel_des", "ext_force_des", "arm_vel_des")]
    hd = [N, lay.nf, 0, lay.na, lay.ndx, int(R.ext_force_frame is not None), int(R.arm_ee_frame is not None), lay.np,
          lay.n, int(cnt[0]), len(KS)]
    path = tmp_path / "in.bin"
    with open(path, "wb") as f:
        f.write(np.array(hd + po + lay.x_off[:N], dtype=np.int32).tobytes())
        f.write(np.array([R.mass, t0]).tobytes())
        f.write(arr[0, :cnt[0]].tobytes())
        f.write(p0.tobytes())
        f.write(x0.tobytes())
        f.write(np.array(list(KS), dtype=np.int32).tobytes())
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    vals = r.stdout.split()
    per = 2 + lay.np + lay.n
    assert len(vals) == per * len(KS)
    for i, k in enumerate(KS):
        row = vals[i * per:(i + 1) * per]
        want = tr.prepare(R, lay, keys, k, t0, p0, x0)
        assert (int(row[0]), int(row[1])) == (want["seg"], want["gait_type"]), k
        p = np.array([float(v) for v in row[2:2 + lay.np]])
        x = np.array([float(v) for v in row[2 + lay.np:]])
        tr.compare(p, want, lay, R, who=(name, k))
        assert np.array_equal(x.view(np.uint64), want["x"].view(np.uint64)), k
        # and the library's own build of the same header
        pl, xl, _ = bo.mpc_timeline_host(k, t0, keys, p0, x0)
        tr.compare(pl, want, lay, R, who=(name, k, "library"))
    bo.close()
