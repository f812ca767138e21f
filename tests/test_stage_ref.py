"""The stage reference of test_stage_kernels_gpu.py, checked without a GPU (tests/stage_ref.py).

1. The reference is the algorithm.  On data the numpy oracle builds alone (OracleOCP +
   OSQPRef._scale, synthetic problem 1 of every GPU case), the long-double iterates after 10
   iterations agree with both fp64 routes (oracle.osqp_ref.BlockReduced and a sparse LU of K)
   and with OSQPRef(max_iter=10, check_termination=0) itself to 1e-9 relative inf-norm, the
   project's QP-step bar; so do the S_i and the stages A', G, C^-1.  Reference against
   reference: measured over the whole case list, block route vs long double x <= 5.4e-12,
   z <= 5.1e-12, y <= 4.9e-10, S_i <= 3.3e-11, A' <= 1.9e-12, G <= 4.4e-12, C^-1 <= 4.5e-12;
   sparse LU x <= 2.8e-13, z <= 2.7e-13, y <= 3.8e-12; OSQPRef x <= 8.4e-15, y <= 9.5e-13.
2. The case table covers what it claims: checked from host-only handles (device = -1).
"""
import numpy as np
import pytest

import stage_ref as sr

BAR = 1e-9


@pytest.mark.parametrize("tag,N", sr.CASE_IDS)
def test_reference_is_the_algorithm(tag, N):
    from oracle.osqp_ref import OSQPRef, REFERENCE_SETTINGS
    qp, o, (grad, Ax, l, u) = sr.oracle_qp(tag, N, prob=1)
    ref = sr.Reference(qp)
    ld = ref.iterates("ld", 10)[-1]
    assert all(np.all(np.isfinite(np.asarray(v, np.float64))) for v in ld)
    assert np.abs(ld[0]).max() > 0 and np.abs(ld[1]).max() > 0 and np.abs(ld[2]).max() > 0
    for route in ("block64", "lu64"):
        got = ref.iterates(route, 10)[-1]
        for j, nm in enumerate("xzy"):
            e = sr.rel(got[j], ld[j])
            assert e <= BAR, (route, nm, e)
    for i in range(N + 1):
        e = ref.e64_factor(i)
        for nm, v in e.items():
            assert v <= BAR, (i, nm, v)
    # the oracle's own loop (quasi-definite KKT), stopped after 10 iterations with no check
    os_ = OSQPRef(o.hess_diag, o.pattern, dict(REFERENCE_SETTINGS, max_iter=10, check_termination=0))
    os_.update_and_solve(grad, Ax, l, u)
    for nm, got, want in (("x", os_.x, ld[0]), ("z", os_.z, ld[1]), ("y", os_.y, ld[2])):
        e = sr.rel(got, want)
        assert e <= BAR, ("OSQPRef", nm, e)


def test_warm_start_and_history():
    """admm_iterate from given iterates continues a cold run: 6 iterations = 2, then 4 from there."""
    qp, _, _ = sr.oracle_qp("cv24", 3)
    ref = sr.Reference(qp)
    six = ref.iterates("ld", 6)
    four = ref.iterates("ld", 4, start=six[1], key="warm")
    for a, b in zip(four[-1], six[-1]):
        assert np.array_equal(a, b)


def test_decode_S_roundtrip():
    """decode_S against the layout rule of state.h written the other way round (tile t of the
    packed lower 4 x 4 tiles -> lane t // K, slot t % K; pair j = 2 r + h)."""
    rng = np.random.default_rng(0)
    for nw, K in ((30, 1), (42, 2), (78, 4), (105, 6)):
        T = (nw + 3) // 4
        M = rng.standard_normal((nw, nw))
        M = M + M.T
        pad = np.zeros((4 * T, 4 * T))
        pad[:nw, :nw] = M
        s_off = 128
        flat = np.zeros(s_off + K * 64 * 16)
        for o in range(K * 64 * 16):
            slot, ln, j, k = o & 1, (o >> 1) & 63, (o >> 7) & 7, o >> 10
            t = K * ln + k
            if t < T * (T + 1) // 2:
                I = int((np.sqrt(8 * t + 1) - 1) / 2)
                J = t - I * (I + 1) // 2
                flat[s_off + o] = pad[4 * I + (j >> 1), 4 * J + 2 * (j & 1) + slot]
        assert np.array_equal(sr.decode_S(flat, s_off, nw, T, K), M)


def test_case_table_covers_what_it_claims():
    ndx, asr, ppw, nunit, kinds = set(), {}, set(), set(), {}
    wide = padded = general = False
    for tag, _, dyn, kw, Ns in sr.CASES:
        for N in Ns:
            bo = sr.make_handle(tag, N, sr.BATCH, device=-1)
            sz, nodes = bo.sizes(), bo.node_table()
            assert sz["N"] == N and len(nodes) == N + 1
            ndx.add(bo.layout.ndx)
            asr.setdefault(sz["admm_asr"], set()).add(dyn)
            ppw.add(sz["admm_ppw"])
            nunit.update(int(nd[9]) for nd in nodes)
            wide |= any(nd[0] > 64 for nd in nodes)
            padded |= any(4 * nd[8] > nd[0] for nd in nodes)
            gc = sr.general_coupling(bo)
            assert gc == (tag == "fd36"), (tag, N)
            general |= gc
            # node types by width: node 0 | tau nodes | plain nodes | terminal (ndx wide)
            widths = [int(nd[0]) for nd in nodes]
            assert widths[-1] == bo.layout.ndx and int(nodes[-1][1]) == 0
            kinds.setdefault(tag, set()).add(len(set(widths)))
            bo.close()
    for tag, N, B, want in sr.PPW_CASES:
        bo = sr.make_handle(tag, N, B, device=-1)
        assert bo.sizes()["admm_ppw"] == want
        ppw.add(want)
        bo.close()
    assert ndx == {24, 30, 36, 48}
    assert set(asr) == {16, 32} and "whole_body_rnea" in asr[32]
    assert ppw == {1, 2, 4}
    assert nunit >= {1, 2, 3, 4, 6}, nunit
    assert wide and padded and general
    # rnea: tau nodes (wider) and plain nodes at N > tau_nodes = 3, only tau nodes at N <= 3
    assert kinds["rnea36"] == {2, 3}, kinds
    assert kinds["cv24"] == {2}
