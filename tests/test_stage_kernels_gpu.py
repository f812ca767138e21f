"""The block factor (k_fnode, k_fchain, k_fred) and the ADMM kernels (k_admm split / fused,
k_admm2, k_admm_rc with several groups and with one) stage by stage on the MI355X, against the
long-double reference of tests/stage_ref.py on the device's own scaled QP.

pl_debug_admm (BatchedOCP.debug_admm) evaluates, scales and factors, then runs exactly k ADMM
iterations with no termination check and no line search, so a failure names a stage (S_i, A', G,
C^-1 of a node, or the iterates after k = 1: one solve, 2: the first T0 turn-around, 10), a
problem and a node instead of a 1e-9 miss after a whole SQP step.  The cases (stage_ref.CASES,
checked by test_stage_ref.py) reach what the golden fixtures do not: horizons N = 2 .. 16, the
chain kernel's group boundaries (N = 7, 8, 16) and fewer nodes than waves, admm_asr = 32 with
whole_body_rnea's node types, two problems per workgroup.

The bar.  For every quantity q the test computes e64(q), the error of the fp64 numpy block route
(oracle.osqp_ref.BlockReduced: the same elimination in LAPACK arithmetic) against the long-double
reference on the same data and k, and asserts

    e_gpu(q) <= K * e64(q) + k * nw_max * 2^-52       (k = 1 for the factor's quantities)

with one K = 16 for every case and quantity: the floor is the rounding of the sums themselves
(it matters only where e64 is ~0, as on centroidal_vel), and K leaves room for another pivot and
summation order but not for a precision loss of the size the r05 4 x 4 pivot inverse cost (about
20 x, test_gpu.STEP_TOL), let alone an indexing or ordering bug (1e-3 .. 1).  EXCEPTIONS holds at
most two measured cases over K with their reason.  Every run writes e_gpu, e64 and their ratio
per case, kernel, k and quantity to stage_errors.json in the directory PL_TEST_OUT names
(default: test_out/ in the repository root).

What it found.  On the kernels as they were, x and z after 2 and 10 iterations missed the bar on
whole_body_rnea at N = 2, 3, 4 (Go2 and B2G) and on B2G whole_body_acc N = 3, with every ADMM
kernel alike: ratios 18 .. 66 (worst: rnea48 N = 2 problem 0, x after k = 2, 1.8e-11 against
e64 = 2.7e-13), while k = 1 and every S_i passed.  The stages located it at node 0, in k_fnode's
C^-1: the same entrywise error as a LAPACK inverse, but 60 x its residual |C^-1 C - I| (1.4e-11
against 2.3e-13).  sweep_split updated a pivot column as col - M_rP (e_q - Q_:q), and the
rounding of 1 - Q_qq costs eps / Q_qq where the pivots are large (the acceleration and torque
columns of a tau node).  k_fnode's sweep now forms M_rP Q_:q directly (the same change in
k_fchain's dx sweep, alone or as well, makes no difference here); the worst ratios since are
MEASURED.
"""
import json
import math
import os

import numpy as np
import pytest

import stage_ref as sr

pytestmark = pytest.mark.gpu

K_BAR = 16.0
# (tag, N, kernel, where) -> (allowed factor, measured ratios); at most two entries.  Both are
# entrywise errors of the u block's inverse on a plain node of Go2 whole_body_rnea, cond(C) =
# 2.4e5, so cond 2^-52 = 5e-11: backward-stable fp64 inverses of that very block (LAPACK LU,
# Gauss-Jordan, Cholesky) spread over 1.4e-13 .. 1.1e-11, LAPACK's own error moved from 1.2e-13
# to 4.5e-12 between two hosts, and the kernel's 2.4e-12 lies inside that spread: e64 happens to
# be a small draw here, the other pivot order is legitimate rounding.
EXCEPTIONS = {
    ("rnea36", 8, "factor", "problem 2 node 3"): (32.0, {"G": 18.6, "Cinv": 20.3}),
    ("rnea36", 9, "factor", "problem 2 node 4"): (32.0, {"S": 20.3}),
}
# worst e_gpu / max(e64, floor) per quantity over all cases, kernels and k on the MI355X
# (stage_errors.json); S, G and C^-1 without the two exceptions: 13.4, 13.6, 14.8
MEASURED = {"S": 20.3, "Ap": 2.6, "G": 18.6, "Cinv": 20.3, "x": 6.3, "z": 6.2, "y": 9.6}

KS = (1, 2, 10)
# kernel variant -> (set_admm_kernel, set_admm_operands, debug_paths)
VARIANTS = {"sweep_split": ("sweep", "split", ()), "sweep_fused": ("sweep", "fused", ()),
            "sweep2": ("sweep2", None, ()), "chain": ("chain", None, ()),
            "chain_one_group": ("chain", None, ("rc_one_group",))}
DATA_KEYS = ("As", "Ps", "qs", "ls", "us", "rho")

_REFS = {}     # (tag, N, problem) -> (the device data the reference was built from, Reference)
_RECORDS = []  # rows of stage_errors.json
OUT = os.path.join(os.environ.get("PL_TEST_OUT") or os.path.join(sr.ROOT, "test_out"), "stage_errors.json")


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


def _reference(tag, N, b, raw):
    """The reference of problem b, built once per case from the first handle's data; every later
    handle must have read back the same bits."""
    key = (tag, N, b)
    if key in _REFS:
        data, ref = _REFS[key]
        for k in DATA_KEYS:
            assert np.array_equal(data[k], raw[k][b]), (key, k, "the scaled QP differs between handles")
        return ref
    return None


def _get_reference(bo, tag, N, b, raw):
    ref = _reference(tag, N, b, raw)
    if ref is None:
        ref = sr.Reference(sr.scaled_qp(bo, b, raw))
        _REFS[(tag, N, b)] = ({k: raw[k][b].copy() for k in DATA_KEYS}, ref)
    return ref


def _judge(fails, tag, N, kernel, k, quantity, where, e_gpu, e64, nw_max):
    """Records one comparison and appends a message to ``fails`` when it misses the bar."""
    fl = sr.floor(k, nw_max)
    exc = EXCEPTIONS.get((tag, N, kernel, where))
    factor = exc[0] if exc and quantity in exc[1] else K_BAR
    bar = factor * e64 + fl
    _RECORDS.append(dict(case=f"{tag}-{N}", kernel=kernel, k=k, quantity=quantity, where=where, e_gpu=e_gpu,
                         e64=e64, floor=fl, ratio=e_gpu / max(e64, fl), bar=bar))
    if not (e_gpu <= bar):  # also catches NaN
        fails.append(f"{tag} N={N} {kernel} k={k} {where} {quantity}: e_gpu {e_gpu:.3e} > "
                     f"{factor:g} * e64 {e64:.3e} + floor {fl:.1e}")


def _configure(bo, variant):
    kernel, operands, _ = VARIANTS[variant]
    bo.set_admm_kernel(kernel)
    assert bo.admm_kernel() == kernel
    if operands:
        bo.set_admm_operands(operands)
        assert bo.admm_operands() == operands


def _iterates(bo):
    B = bo.batch
    return tuple(bo.debug(nm, B * ln).reshape(B, ln) for nm, ln in (("xa", bo.n), ("za", bo.m), ("ya", bo.m)))


def _run_variant(tag, N, variant, fails, B=sr.BATCH, probs=None, ks=KS):
    """debug_admm(k) from cold for every k on one handle; compares the listed problems with the
    reference and returns {k: (xa, za, ya)}."""
    bo = sr.make_handle(tag, N, B, debug_paths=VARIANTS[variant][2])
    try:
        _configure(bo, variant)
        nw_max = bo.sizes()["nw_max"]
        if variant == "chain":
            assert bo.admm_groups() == math.ceil((N + 1) / 8), (tag, N, bo.admm_groups())
        if variant == "chain_one_group":
            assert bo.admm_groups() == 1
        out, raw = {}, None
        for k in sorted(ks, reverse=True):  # the longest run first: the reference computes it once
            bo.debug_admm(k, reset=True)
            out[k] = _iterates(bo)
            if raw is None:
                raw = sr.read_scaled(bo)
            for b in (range(B) if probs is None else probs):
                ref = _get_reference(bo, tag, N, b, raw)
                want = ref.iterates("ld", k)[k - 1]
                e64 = ref.e64(k)
                for j, nm in enumerate("xzy"):
                    _judge(fails, tag, N, variant, k, nm, f"problem {b}", sr.rel(out[k][j][b], want[j]), e64[nm],
                           nw_max)
        return out
    finally:
        bo.close()


def _assert_same_bits(a, b, what):
    for k in a:
        for j, nm in enumerate(("xa", "za", "ya")):
            assert np.array_equal(a[k][j], b[k][j]), (what, k, nm)


def _factor_check(tag, N, debug_paths=()):
    bo = sr.make_handle(tag, N, sr.BATCH, debug_paths=debug_paths)
    kernel = "factor" + ("+" + "+".join(debug_paths) if debug_paths else "")
    fails = []
    try:
        bo.debug_admm(0)
        B, X = bo.batch, bo.layout.ndx
        sz = bo.sizes()
        raw = sr.read_scaled(bo)
        nodes = raw["nodes"]
        Sall = bo.debug("S", B * sz["S_stride"]).reshape(B, sz["S_stride"])
        fs_off, fs_stride = sr.fs_offsets(nodes, X)
        FS = bo.debug("FS", B * fs_stride).reshape(B, fs_stride)
        for b in range(B):
            ref = _get_reference(bo, tag, N, b, raw)
            for i, nd in enumerate(nodes):
                nw, U = int(nd[0]), int(nd[1])
                e64 = ref.e64_factor(i)
                where = f"problem {b} node {i}"
                Sg = sr.decode_S(Sall[b], int(nd[10]), nw, int(nd[8]), int(nd[9]))
                _judge(fails, tag, N, kernel, 1, "S", where, sr.rel(Sg, ref.ld.S[i]), e64["S"], sz["nw_max"])
                if U > 0:
                    want = sr.node_stages(ref.nb, i)
                    got = sr.fs_blocks(FS[b], fs_off[i], X, U)
                    for nm, g, w in zip(("Ap", "G", "Cinv"), got, want):
                        _judge(fails, tag, N, kernel, 1, nm, where, sr.rel(g, w), e64[nm], sz["nw_max"])
    finally:
        bo.close()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------- (a) factor
@pytest.mark.parametrize("tag,N", sr.CASE_IDS)
def test_factor(tag, N):
    """Every S_i and, for nodes with u columns, A', G and C^-1 of k_fnode, per problem and node."""
    _factor_check(tag, N)


@pytest.mark.parametrize("N", sr.case("aba36")[4])
def test_factor_fchain_list(N):
    """whole_body_aba's E_{i+1} on the list path instead of the MFMA path."""
    _factor_check("aba36", N, debug_paths=("fchain_list",))


# ---------------------------------------------------------------------------- (b) k iterations from cold
@pytest.mark.parametrize("tag,N", sr.CASE_IDS)
def test_sweep_kernels_from_cold(tag, N):
    """k_admm with both operand paths (bit-equal) and k_admm2 after 1, 2 and 10 iterations."""
    fails = []
    split = _run_variant(tag, N, "sweep_split", fails)
    fused = _run_variant(tag, N, "sweep_fused", fails)
    _run_variant(tag, N, "sweep2", fails)
    _assert_same_bits(split, fused, "split vs fused")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("tag,N", sr.CASE_IDS)
def test_chain_kernel_from_cold(tag, N):
    """k_admm_rc with ceil((N + 1) / 8) workgroups per problem and with one (bit-equal); the
    general-coupling case has no chain kernel and must say so."""
    if tag == "fd36":
        from pinoloco._lib import PinolocoError
        bo = sr.make_handle(tag, N, sr.BATCH)
        try:
            with pytest.raises(PinolocoError):
                bo.set_admm_kernel("chain")
        finally:
            bo.close()
        return
    fails = []
    groups = _run_variant(tag, N, "chain", fails)
    one = _run_variant(tag, N, "chain_one_group", fails)
    _assert_same_bits(groups, one, "chain groups vs one group")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------- (c) warm iterates
@pytest.mark.parametrize("tag,N", [("cv24", 3), ("rnea36", 4)])
def test_warm_iterates(tag, N):
    """Seeded random xa, za, ya, then 4 iterations without a reset: k_admm_init's gather with
    non-zero z and y; the reference starts from the same values."""
    fails = []
    for variant in ("sweep_split", "sweep_fused", "sweep2", "chain", "chain_one_group"):
        bo = sr.make_handle(tag, N, sr.BATCH, debug_paths=VARIANTS[variant][2])
        try:
            _configure(bo, variant)
            B, nw_max = bo.batch, bo.sizes()["nw_max"]
            rng = np.random.default_rng(7)
            start = [0.1 * rng.standard_normal((B, ln)) for ln in (bo.n, bo.m, bo.m)]
            for nm, v in zip(("xa", "za", "ya"), start):
                bo.debug_set(nm, v)
            bo.debug_admm(4, reset=False)
            got = _iterates(bo)
            raw = sr.read_scaled(bo)
            for b in range(B):
                ref = _get_reference(bo, tag, N, b, raw)
                st = tuple(s[b] for s in start)
                want = ref.iterates("ld", 4, start=st, key="warm")[3]
                e64 = ref.e64(4, start=st, key="warm")
                for j, nm in enumerate("xzy"):
                    _judge(fails, tag, N, variant + "/warm", 4, nm, f"problem {b}", sr.rel(got[j][b], want[j]),
                           e64[nm], nw_max)
        finally:
            bo.close()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------- (d) problems per workgroup
@pytest.mark.parametrize("tag,N,B,ppw", sr.PPW_CASES)
def test_problems_per_workgroup(tag, N, B, ppw):
    """The one-wave sweep with 4 (B = 1027) and 2 (B = 515) problems per workgroup, the last
    workgroup ragged: the first and the last problems against their references, and problem 0
    bit-equal to the same problem alone."""
    bo = sr.make_handle(tag, N, B, device=-1)
    assert bo.sizes()["admm_ppw"] == ppw
    bo.close()
    fails = []
    probs = [0, 1, B - 3, B - 2, B - 1]
    big = _run_variant(tag, N, "sweep_fused", fails, B=B, probs=probs, ks=(10,))
    one = _run_variant(tag, N, "sweep_fused", fails, B=1, probs=[0], ks=(10,))
    for j, nm in enumerate(("xa", "za", "ya")):
        assert np.array_equal(big[10][j][0], one[10][j][0]), nm
    assert not fails, "\n".join(fails)
