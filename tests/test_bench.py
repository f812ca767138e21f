"""bench.py contract pieces that run without a GPU: the rank launcher (--gpus N
spawns N ranks itself when no torchrun environment is present), the roofline byte
accounting and the revision check of the PMC traffic file.  On the GPU: what a plain and a
--full run do, and that --dump-outputs holds the outputs of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.slow
def test_gpus2_launches_two_ranks():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--batch", "3",
                        "--robot", "go2", "--nodes", "6"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 6 and out["gathered_rows"] == 6


def test_world_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def _bench(*argv):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


SMALL = ["--robot", "go2", "--nodes", "10", "--steps", "3", "--warmup", "2"]


# batch 3 replays each step as a HIP graph; from batch 64 on the timed region carries the
# per-launch events of the roofline (bench.py prof_timed)
@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 64])
def test_plain_run_dumps_last_timed_step(tmp_path, B):
    """A plain run times --steps steps, prints ms_per_step and none of the --full legs, and
    --dump-outputs holds what the MPC loop's caller reads after step warmup + steps - 1: the same
    loop driven here gives the same [u_0, x_state] and solve outcome.  Two processes differ at
    most by the order of f64 atomic adds (ulps, through <= 100 ADMM iterations); the suite's
    parity bar on states is 1e-7, the bound here 1e-9 of the largest entry."""
    from conftest import make_robot
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import build_batch
    out = _bench(*SMALL, "--batch", str(B), "--dump-outputs", str(tmp_path / "d"))
    assert out["steps"] == 3 and out["warmup"] == 2 and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(B * 1e3 / out["ms_per_step"], rel=1e-12)
    assert "cpu_baseline" not in out and "host_io" not in out
    assert ("roofline" in out) == (B >= 64)
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in ("u0_xstate", "step_stats")}
    assert sorted(os.listdir(tmp_path / "d")) == ["step_stats.npy", "u0_xstate.npy"]
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in got.values())

    R = make_robot("go2")
    lay, P, X, XS, T0 = build_batch(R, "whole_body_rnea", 10, B, 0)
    bo = BatchedOCP(R, "whole_body_rnea", 10, batch=B, device=0, gait_type="trot", gait_period=0.8)
    bo.set_params(P)
    bo.set_x(X)
    bo.init_solver()
    bo.mpc_setup(XS, T0)
    for k in range(5):
        if k == 2:  # the timed region, as bench.py enters it
            bo.sync()
            if B >= 64:
                bo.profile(1)
        bo.mpc_step(k)
    bo.sync()
    want = bo.mpc_download()
    st = bo.mpc_stats()
    bo.close()
    assert got["u0_xstate"].shape == want.shape == (B, lay.nu[0] + lay.nx)
    assert np.abs(got["u0_xstate"] - want).max() <= 1e-9 * np.abs(want).max()
    assert np.array_equal(got["step_stats"][:, 0], st["status"])
    assert np.array_equal(got["step_stats"][:, 1], st["admm_iters"])
    assert np.abs(got["step_stats"][:, 3] - st["f"]).max() <= 1e-9 * np.abs(st["f"]).max()


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(tmp_path):
    """--full: the CPU baseline, the host_io pass and (batch < 64) the roofline from profiled
    steps after the timed region; the dump still holds the last timed step."""
    plain = _bench(*SMALL, "--batch", "3", "--dump-outputs", str(tmp_path / "p"))
    full = _bench(*SMALL, "--batch", "3", "--full", "--dump-outputs", str(tmp_path / "f"))
    assert full["steps"] == 3 and full["ms_per_step"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["host_io"]["steps"] == 3
    assert full["roofline"]["launches"] > 0 and "profiled steps" in full["roofline"]["launch_timing"]
    for n in ("u0_xstate", "step_stats"):
        a, b = np.load(tmp_path / "p" / f"{n}.npy"), np.load(tmp_path / "f" / f"{n}.npy")
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-9 * np.abs(a).max()


def test_admm_bytes_stored_triangle():
    import bench
    # node table columns: [nw, nu, x_off, row_off, nrow, ncol, ent_off, nent, ntile, nunit, s_off, ncpl]
    ntab = np.zeros((3, 12), dtype=np.int32)
    ntab[:, 0] = [10, 12, 4]
    ntab[:, 9] = [1, 2, 1]
    sz = {"nnz": 100, "n": 26, "m": 30}
    tri = np.array([55, 78, 10.0])
    want = 8 * (2 * tri.sum() - tri[0] - tri[-1] + 100 + 7 * 26 + 7 * 30)
    assert bench.admm_bytes_per_problem_iter(sz, ntab) == want
    blk = np.array([1, 2, 1]) * 64 * 16.0
    wantp = 8 * (2 * blk.sum() - blk[0] - blk[-1] + 100 + 7 * 26 + 7 * 30)
    assert bench.admm_bytes_per_problem_iter(sz, ntab, padded=True) == wantp


def test_traffic_file_is_revision_keyed(tmp_path, monkeypatch):
    import bench
    f = tmp_path / "t.json"
    rec = {"src_sha": bench.traffic_source_sha(), "batch": 8, "nodes": 5, "workload": "w",
           "bytes_per_problem_iter": 1.0}
    f.write_text(json.dumps(rec))
    monkeypatch.setattr(bench, "TRAFFIC_FILE", str(f))
    assert bench.measured_traffic(8, 5, "w")["bytes_per_problem_iter"] == 1.0
    assert bench.measured_traffic(16, 5, "w") is None
    rec["src_sha"] = "0" * 16
    f.write_text(json.dumps(rec))
    assert bench.measured_traffic(8, 5, "w") is None
