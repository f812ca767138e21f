"""numpy twin of the timeline step of the device MPC loop (pl_mpc_timeline_host, k_mpc_prepare with
a timeline), written from the definitions of the feature and the repository's own gait tables
(pinoloco/gait.py), not from csrc/timeline.h.

One problem, MPC step k, keyframes sorted by k_start (dicts as BatchedOCP.keyframe makes them):
  governing keyframe s   the last one with k_start <= k; the first one for k before it
  commands               keyframe s's when ramp == 0, s is the last keyframe or k < k_start_s;
                         else a = (k - k_s) / (k_{s+1} - k_s), c = c_s + a (c_{s+1} - c_s)
                         (base_vel_des always; ext_force_des / arm_vel_des only where the robot has
                         the frame)
  gait scalars           GaitSequence(gait, period).n_contacts / .swing_period
  schedule               GaitSequence.get_gait_schedule, node by node, at t_0 = fma(k, dt_min, t0) +
                         t_shift and t_{i+1} = fma(dt_min, gamma^i, t_i), gamma as horizon_dts has
                         it: the bracket t0 + k dt_min and every t_i + dt_i are rounded once, as the
                         library states them (include/pinoloco.h, csrc/targets.h)
  warm start (k > 0)     forces of every node <- f_des = 0.8 / 1.2 m g / n_contacts on the z axis of
                         the front / rear feet, zero on a foot in swing and on the end effector"""
from fractions import Fraction

import numpy as np

from pinoloco.gait import GaitSequence

GAIT_NAMES = {0: "trot", 1: "walk", 2: "stand", "trot": "trot", "walk": "walk", "stand": "stand"}
CODES = {"trot": 0, "walk": 1, "stand": 2}
COMMANDS = (("base_vel_des", 6), ("ext_force_des", 3), ("arm_vel_des", 3))
GRAV = 9.81


def fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic, then the nearest double)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def segment(keys, k):
    s = 0
    for j, kf in enumerate(keys):
        if kf["k_start"] <= k:
            s = j
    return s


def commands(keys, s, k):
    """{name: values} of step k, and whether they were ramped."""
    K = keys[s]
    cur = {n: np.asarray(K.get(n, np.zeros(w)), dtype=np.float64) for n, w in COMMANDS}
    if not K.get("ramp") or s + 1 >= len(keys) or k < K["k_start"]:
        return cur, False
    Kn = keys[s + 1]
    a = float(k - K["k_start"]) / float(Kn["k_start"] - K["k_start"])
    nxt = {n: np.asarray(Kn.get(n, np.zeros(w)), dtype=np.float64) for n, w in COMMANDS}
    return {n: cur[n] + a * (nxt[n] - cur[n]) for n, _ in COMMANDS}, True


def command_bar(keys, s, ramped):
    """The bar of a ramped command, per component: 2**-51 (|c_s| + |c_{s+1}|), one product rounding plus
    one sum rounding of c_s + a (c_{s+1} - c_s), which also covers a build that fuses the two; zero
    (exact) for a held or clamped one."""
    if not ramped:
        return {n: np.zeros(w) for n, w in COMMANDS}
    K, Kn = keys[s], keys[s + 1]
    return {n: 2.0 ** -51 * (np.abs(np.asarray(K.get(n, np.zeros(w)), dtype=np.float64))
                             + np.abs(np.asarray(Kn.get(n, np.zeros(w)), dtype=np.float64))) for n, w in COMMANDS}


def prepare(robot, lay, keys, k, t0, p, x=None):
    """The prepare step of MPC step k on copies of p [np] and x [n] (None: no warm start).
    Returns a dict: p, x, seg, gait_type, gait_period, commands [12], ramped, bar [12]."""
    keys = list(keys)
    p = np.array(p, dtype=np.float64)
    s = segment(keys, k)
    K = keys[s]
    cmd, ramped = commands(keys, s, k)
    bar = command_bar(keys, s, ramped)
    has = {"base_vel_des": True, "ext_force_des": robot.ext_force_frame is not None,
           "arm_vel_des": robot.arm_ee_frame is not None}
    for n, w in COMMANDS:
        if has[n]:
            o = lay.poff[n][0]
            p[o:o + w] = cmd[n]
    gait = GAIT_NAMES[K.get("gait_type", K.get("gait", "trot"))]
    gs = GaitSequence(gait, float(K.get("gait_period", 0.8)))
    p[lay.poff["n_contacts"][0]] = gs.n_contacts
    p[lay.poff["swing_period"][0]] = gs.swing_period
    dt_min, dt_max = p[lay.poff["dt_min"][0]], p[lay.poff["dt_max"][0]]
    t = fma(float(k), dt_min, t0) + float(K.get("t_shift", 0.0))
    gamma = (dt_max / dt_min) ** (1 / (lay.N - 1))   # horizon_dts: dt_i = dt_min gamma^i
    contact, swing = np.ones((4, lay.N)), np.zeros((4, lay.N))
    for i in range(lay.N):
        if i > 0:
            t = fma(dt_min, gamma ** (i - 1), t)
        c, sw = gs.get_gait_schedule(t, [], 1)
        contact[:, i], swing[:, i] = c[:, 0], sw[:, 0]
    oc, osw = lay.poff["contact_schedule"][0], lay.poff["swing_schedule"][0]
    p[oc:oc + 4 * lay.N] = contact.T.ravel()   # [node][foot], the column-major 4 x N parameter
    p[osw:osw + 4 * lay.N] = swing.T.ravel()
    if x is not None:
        x = np.array(x, dtype=np.float64)
        if k > 0:
            fg = GRAV * robot.mass
            for i in range(lay.N):
                f = np.zeros(lay.nf)
                for foot in range(4):
                    if contact[foot, i] != 0.0:
                        f[3 * foot + 2] = (0.8 if foot < 2 else 1.2) * fg / gs.n_contacts
                o = lay.x_off[i] + lay.ndx + lay.f_idx
                x[o:o + lay.nf] = f
    return {"p": p, "x": x, "seg": s, "gait_type": CODES[gait], "gait_period": float(K.get("gait_period", 0.8)),
            "commands": np.concatenate([cmd[n] for n, _ in COMMANDS]), "ramped": ramped,
            "bar": np.concatenate([bar[n] for n, _ in COMMANDS])}


def compare(got_p, want, lay, robot, who=""):
    """got_p [np] against a prepare() result: everything exact except a ramped command, within its bar.
    Returns the largest command deviation in units of the bar (0 where the bar is zero and met)."""
    p = want["p"]
    cmd_idx, cmd_bar = [], []
    off = 0
    for n, w in COMMANDS:
        present = n == "base_vel_des" or (robot.ext_force_frame is not None if n == "ext_force_des"
                                          else robot.arm_ee_frame is not None)
        if present:
            cmd_idx += list(range(lay.poff[n][0], lay.poff[n][0] + w))
            cmd_bar += list(want["bar"][off:off + w])
        off += w
    cmd_idx, cmd_bar = np.array(cmd_idx), np.array(cmd_bar)
    rest = np.ones(lay.np, dtype=bool)
    rest[cmd_idx] = False
    bad = np.nonzero(got_p[rest].view(np.uint64) != p[rest].view(np.uint64))[0]
    at = np.nonzero(rest)[0][bad][:8]
    assert bad.size == 0, (who, "parameters differ at", at, [float.hex(v) for v in got_p[at]], [float.hex(v) for v in p[at]])
    dev = np.abs(got_p[cmd_idx] - p[cmd_idx])
    assert np.all(dev <= cmd_bar), (who, "commands", dev, cmd_bar)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(cmd_bar > 0, dev / cmd_bar, 0.0)
    return float(rel.max())
