"""The contact plant's host code under AddressSanitizer and UBSan, in a stand-alone program.

tests/native/contact_host.cpp has its own main around pl::plant_step with contact (csrc/plant.h,
the code k_plant runs); it is compiled for the host alone with the address and undefined-behaviour
sanitizers as host options and run directly on the CPU, nothing loaded into python and nothing
run on a GPU.  Its inputs are the host test's (contact_ref.case_inputs:
air, stick and slide at the first substep), on exactly sized heap buffers; three steps with the
anchors carried along.  Required: a clean exit with nothing on stderr, and the library's own
result (mpc_plant_host) to the bars of tests/test_contact_host.py.  The sanitized build takes
about a minute, hence the slow mark."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import contact_ref as cr
from conftest import ROOT
from test_contact_host import _host, _problems, _wrench

pytestmark = pytest.mark.slow


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and shutil.which(hipcc) is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("contact") / "contact_host"
    # host code only: the sanitizers are host options (-Xarch_host), no device code is instrumented
    cmd = [hipcc, "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Wno-unused-result", "-Wno-comment",
           "-I", os.path.join(ROOT, "pino-locoman_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "contact_host.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return str(out)


def test_plant_step_with_contact_is_clean(program, tmp_path):
    from pinoloco import _lib
    sub, calls = 4, 3
    bo = _host("b2g", "whole_body_rnea")
    lay, P, X, XS = _problems(bo.robot, "whole_body_rnea")
    W = _wrench()
    prm, GZ = cr.case_inputs(bo, XS)
    L = _lib.lib()
    sizes = (C.c_int * 2)()
    _lib.check(L.pl_debug_consts(bo.h, None, None, sizes))
    mb, ob = C.create_string_buffer(sizes[0]), C.create_string_buffer(sizes[1])
    _lib.check(L.pl_debug_consts(bo.h, mb, ob, None))
    xoff = np.ascontiguousarray(bo.node_table()[:, 2], dtype=np.int32)
    for b in range(len(XS)):
        c = cr.one(prm, b)
        head = np.array([sizes[0], sizes[1], lay.N, bo.np, bo.n, lay.nx, sub, calls], dtype=np.int32)
        c8 = np.array([c[k] for k in cr.FIELDS] + [0.0])
        path = tmp_path / f"in{b}.bin"
        with open(path, "wb") as f:
            for a in (head, mb.raw, ob.raw, xoff, P[b], X[b], XS[b], W[b], c8, GZ[b]):
                f.write(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
        r = subprocess.run([program, str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (b, r.returncode, r.stderr[-3000:])
        got = np.array([float(v) for v in r.stdout.split()])
        xs, anc = XS[b], None
        for _ in range(calls):
            xs, anc, forces = bo.mpc_plant_host(P[b], X[b], xs, sub, W[b], c, GZ[b], anc)
        assert got.shape == (lay.nx + 24,) and np.all(np.isfinite(got))
        bx, bf, ba = cr.bars(c, 1.0)
        ex = np.abs(got[:lay.nx] - xs).max()
        ea = np.abs(got[lay.nx:lay.nx + 12] - anc.ravel()).max()
        ef = np.abs(got[lay.nx + 12:] - forces.ravel()).max()
        print(f"sanitized program, problem {b}: state {ex:.2e}, anchors {ea:.2e}, forces {ef:.2e}")
        assert ex < bx and ea < ba and ef < bf, (b, ex, ea, ef)
    bo.close()
