"""Batched Jacobians of the point functions on the MI355X (k_dyn_jac.hip) against the host handle.

The device and the host run the same columns (csrc/dyn_jac.h), so their difference is floating-point
contraction and libm.  Bars: relative to max(1, max |block|), per function ten times the worst
difference measured on the MI355X over everything this file runs (both robots, B = 1 and B = 67,
the full wrt and the configuration-only wrt), and never above the function's host-against-oracle
bar of tests/test_dyn_jac_host.py (1e-12; 1e-10 for the solve-based functions).  Measured worst
cases are in DEV_MEASURED below and in DESIGN.md.

1. Every supported function on Go2 and B2G, B = 1 and B = 67 (the four points of
   tests/dyn_jac_ref.py plus perturbed copies; 67 is no multiple of anything the grid uses), with
   the full wrt and with the configuration alone (W = nv < 64: a lone partial tile).
2. The lane-map edges by name: Go2 rnea (W = 66: the second tile has two live lanes), B2G rnea
   (W = 87), a frame position (W = nv, 3 rows), ABA on both robots (the LDS Cholesky, nv = 18, 24).
3. pl_dyn_jac_device through torch tensors equals pl_dyn_jac with host pointers bit for bit; a jac
   buffer pre-filled with NaN has no NaN left and a guard region after it is untouched.
4. The device `out` equals pl_dyn_eval on the device handle bit for bit.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libpinoloco.so, so both share one HIP runtime; the device buffers below)

import dyn_jac_ref as dr

pytestmark = pytest.mark.gpu

# worst relative device-host difference per function measured on the MI355X (see the docstring)
DEV_MEASURED = {
    "rnea": 1.0e-15, "aba": 6.6e-12, "nle": 7.5e-16, "frame_pos": 3.4e-16, "frame_vel": 6.7e-16,
    "frame_vel_rel": 5.6e-16, "gaps_wb": 1.0e-15, "base_acc_wb": 2.2e-15, "com_dyn": 1.3e-15,
    "base_vel_cv": 1.5e-14, "base_acc_cv": 2.2e-15, "gaps_cv": 6.5e-16, "com": 5.6e-16, "gaps_ca": 2.3e-15,
}


def _bar(cname):
    cap = 1e-10 if cname in dr.SOLVE else 1e-12
    return min(cap, 10.0 * DEV_MEASURED[cname])


_cache = {}


def _setup(name):
    if name not in _cache:
        dev, _ = dr.cases(name, device=0)
        host, R = dr.cases(name, device=-1)
        P67, _, _ = dr.batch67(name)
        _cache[name] = (dev, host, P67, R)
    return _cache[name]


def _rel(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(got))
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def _compare(name, cname, B, wrt):
    dev, host, P67, _ = _setup(name)
    (_, pd, keys, cfg), = [c for c in dev if c[0] == cname]
    (_, ph, _, _), = [c for c in host if c[0] == cname]
    args = [P67[k][3] if B == 1 else P67[k][:B] for k in keys]
    sel = None if wrt == "full" else [cfg]
    got, want = pd.jacobian(wrt=sel)(*args), ph.jacobian(wrt=sel)(*args)
    assert len(got) == len(want)
    worst = max(_rel(g, w) for g, w in zip(got, want))
    print(f"{name} {cname} B={B} wrt={wrt}: device-host {worst:.2e} (bar {_bar(cname):.1e})")
    return worst


@pytest.mark.parametrize("name", dr.ROBOTS)
def test_device_matches_host(name):
    dev = _setup(name)[0]
    failed = []
    for cname, _, _, _ in dev:
        worst = max(_compare(name, cname, B, wrt) for B in (1, 67) for wrt in ("full", "cfg"))
        print(f"MEASURED {name} {cname} {worst:.3e}")
        if worst > _bar(cname):
            failed.append((cname, worst))
    assert not failed, failed


@pytest.mark.parametrize("name,cname", [("go2", "rnea"), ("b2g", "rnea"), ("go2", "frame_pos"), ("go2", "aba"),
                                        ("b2g", "aba")])
def test_lane_map_edges(name, cname):
    dev, _, _, R = _setup(name)
    (_, pd, keys, cfg), = [c for c in dev if c[0] == cname]
    tan, rows = pd.jacobian_sizes()
    W = sum(tan)
    assert (name, cname, W) in {("go2", "rnea", 66), ("b2g", "rnea", 87), ("go2", "frame_pos", 18), ("go2", "aba", 60),
                                ("b2g", "aba", 81)}
    assert rows == (3 if cname == "frame_pos" else R.nv)
    assert _compare(name, cname, 67, "full") <= _bar(cname)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name,cname", [("b2g", "rnea"), ("go2", "aba"), ("b2g", "frame_vel_rel"), ("go2", "base_vel_cv")])
def test_device_pointers_bitwise_with_guard(name, cname):
    dev, _, P67, _ = _setup(name)
    (_, pd, keys, cfg), = [c for c in dev if c[0] == cname]
    B = 67
    args = [P67[k][:B] for k in keys]
    val, *blocks = pd.jacobian(with_value=True)(*args)  # host pointers, staged
    want = np.concatenate(blocks, axis=2)
    rows, W = want.shape[1:]
    n, guard = B * rows * W, 4096
    ins = [_dev(a) for a in args]
    jac = torch.full((n + guard,), float("nan"), dtype=torch.float64, device="cuda")
    jac[n:] = -1.2345e300
    out = torch.full((B * rows + guard,), float("nan"), dtype=torch.float64, device="cuda")
    out[B * rows:] = -1.2345e300
    torch.cuda.synchronize()
    pd.jacobian_device(B, [t.data_ptr() for t in ins], jac.data_ptr(), out=out.data_ptr())
    got, gout = jac.cpu().numpy(), out.cpu().numpy()
    assert not np.isnan(got[:n]).any()
    assert np.all(got[n:] == -1.2345e300) and np.all(gout[B * rows:] == -1.2345e300)
    assert np.array_equal(got[:n].reshape(B, rows, W), want)
    assert np.array_equal(gout[:B * rows].reshape(B, rows), val)


@pytest.mark.parametrize("name", dr.ROBOTS)
def test_device_value_equals_eval(name):
    dev, _, P67, _ = _setup(name)
    for cname, pd, keys, cfg in dev:
        args = [P67[k] for k in keys]
        val = pd.jacobian(wrt=[cfg], with_value=True)(*args)[0]
        assert np.array_equal(val, pd(*args)), cname
