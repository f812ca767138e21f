"""numpy twin of the rollout log's record step (pl_mpc_record_host, k_mpc_record), written from the
definitions of the feature, not from csrc/record.h.

Row: the fields of FIELDS side by side, all float64.  Metrics, per problem over its steps:
  steps            how many steps were seen
  first_nonfinite  first k whose x_state has a non-finite entry, else -1
  first_out        first k (finite x_state) with |z - z_ref| > dz_tol or c_z < cz_min, else -1;
                   z = q[2], c_z = 1 - 2 (q[3]^2 + q[4]^2), q the configuration inside x_state
                   (at 6 for centroidal_vel, x = [h, q], else at 0); tolerance None = never out
  max_dz, min_cz   max |z - z_ref| and min c_z over the finite states, from 0 and 1
  n_not_solved     steps with status != 1;  n_ls_rejected: steps with ls_accepted == 0
  max_viol         max finite viol_max, from 0
Slots: of the steps s = 0, 1, ... since the start, those with s % every == 0 are recorded while a
slot is free, and counted as dropped afterwards."""
import numpy as np

FIELDS = ("x_init", "u0", "stats", "x_state", "ground_f", "anchor_active")
STATS = ("status", "admm_iters", "ls_accepted", "ls_alpha", "viol_max", "f", "pri_res", "dua_res")


def widths(nx, nu0, n_feet=4):
    return dict(zip(FIELDS, (nx, nu0, 8, nx, 3 * n_feet, n_feet)))


def offsets(nx, nu0, n_feet=4):
    w = widths(nx, nu0, n_feet)
    off, o = {}, 0
    for f in FIELDS:
        off[f] = o
        o += w[f]
    return off, o


def row(step, n_feet=4):
    """One step (a dict as BatchedOCP.mpc_record_host takes it) as the dict of a log row's fields."""
    gf = np.zeros((n_feet, 3)) if step.get("ground_f") is None else np.asarray(step["ground_f"], dtype=np.float64)
    an = np.zeros((n_feet, 3)) if step.get("anchors") is None else np.asarray(step["anchors"], dtype=np.float64)
    return {"x_init": np.asarray(step["x_init"], dtype=np.float64),
            "u0": np.asarray(step["u0"], dtype=np.float64),
            "stats": np.array([float(step["stats"][k]) for k in STATS]),
            "x_state": np.asarray(step["x_state"], dtype=np.float64),
            "ground_f": gf.reshape(-1),
            "anchor_active": (an.reshape(n_feet, 3)[:, 2] != 0).astype(np.float64)}


def slots(n_steps, capacity, every):
    """(indices of the recorded steps, dropped)"""
    due = [s for s in range(n_steps) if s % every == 0]
    return due[:capacity], max(0, len(due) - capacity)


def metrics(ks, x_states, stats, z_ref, dz_tol=None, cz_min=None, qoff=0):
    """ks [T], x_states [T][nx], stats [T][8] (columns STATS) of one problem -> the metrics dict."""
    m = dict(steps=0, first_nonfinite=-1, first_out=-1, n_not_solved=0, n_ls_rejected=0, max_dz=0.0, min_cz=1.0,
             max_viol=0.0)
    for k, xs, st in zip(ks, np.asarray(x_states, dtype=np.float64), np.asarray(stats, dtype=np.float64)):
        m["steps"] += 1
        if not np.all(np.isfinite(xs)):
            if m["first_nonfinite"] == -1:
                m["first_nonfinite"] = int(k)
        else:
            q = xs[qoff:]
            dz = abs(q[2] - z_ref)
            cz = 1.0 - 2.0 * (q[3] * q[3] + q[4] * q[4])
            m["max_dz"] = max(m["max_dz"], dz)
            m["min_cz"] = min(m["min_cz"], cz)
            out = (dz_tol is not None and dz > dz_tol) or (cz_min is not None and cz < cz_min)
            if out and m["first_out"] == -1:
                m["first_out"] = int(k)
        m["n_not_solved"] += int(st[0] != 1)
        m["n_ls_rejected"] += int(st[2] == 0)
        if np.isfinite(st[4]):
            m["max_viol"] = max(m["max_viol"], float(st[4]))
    return m


INT_FIELDS = ("steps", "first_nonfinite", "first_out", "n_not_solved", "n_ls_rejected")
CZ_BAR = 1e-15  # three multiplies / adds on values <= 1, where a fused multiply-add may round once less


def compare(got, want, who=""):
    """Integer metrics, max_dz and max_viol exact; min_cz within CZ_BAR."""
    for k in INT_FIELDS:
        assert int(got[k]) == int(want[k]), (who, k, got[k], want[k])
    assert float(got["max_dz"]) == float(want["max_dz"]), (who, got["max_dz"], want["max_dz"])
    assert float(got["max_viol"]) == float(want["max_viol"]), (who, got["max_viol"], want["max_viol"])
    assert abs(float(got["min_cz"]) - float(want["min_cz"])) <= CZ_BAR, (who, got["min_cz"], want["min_cz"])
