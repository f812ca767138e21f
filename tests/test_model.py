"""Model tables: Pinocchio URDF semantics restated in pinoloco/model.py.

Pins: total masses from the URDFs, joint
counts after buildReducedModel (utils/robot.py:13-22, 96-118), joint order of the
urdfdom child map, and the SRDF reference poses.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_robot

REF = GOLDEN  # robots/<name>_description/{urdf,srdf}/: the reference's robot descriptions


@pytest.mark.parametrize("name,nq,nv,mass", [("go2", 19, 18, 16.087), ("b2", 19, 18, 72.5803),
                                              ("b2g", 25, 24, 77.26827)])
def test_dims_and_mass(name, nq, nv, mass):
    R = make_robot(name)
    assert (R.nq, R.nv, R.nj) == (nq, nv, nq - 7)
    assert R.mass == pytest.approx(mass, abs=1e-4)
    assert R.model.joints[1].name == "root_joint"
    # feet FR, FL, RR, RL (utils/gait_sequence.py:7) resolve to frames
    names = [R.model.frames[f].name for f in R.foot_frames]
    assert names == ["FR_foot", "FL_foot", "RR_foot", "RL_foot"]


def test_joint_order_is_name_sorted_dfs():
    """urdfdom keeps children in a std::map, so the DFS visits legs FL, FR, RL, RR."""
    R = make_robot("go2")
    legs = [j.name[:2] for j in R.model.joints[2:]]
    assert legs == ["FL"] * 3 + ["FR"] * 3 + ["RL"] * 3 + ["RR"] * 3


def test_b2g_gripper_locked_and_arm_frames():
    R = make_robot("b2g")
    names = [j.name for j in R.model.joints]
    assert len(names) == 1 + 1 + 12 + 6
    assert R.model.frames[R.arm_ee_frame].name == "gripperStator"
    assert R.ext_force_frame == R.arm_ee_frame


def test_reference_pose_is_normalised():
    for name in ("go2", "b2", "b2g"):
        R = make_robot(name)
        assert np.linalg.norm(R.q0[3:7]) == pytest.approx(1.0, abs=1e-12)
        assert np.all(R.q0[7:] >= R.joint_pos_min - 1e-9) and np.all(R.q0[7:] <= R.joint_pos_max + 1e-9)


def test_json_roundtrip():
    from pinoloco import model as mdl
    R = make_robot("b2")
    m2 = mdl.Model.from_dict(R.model.to_dict())
    assert m2.nq == R.model.nq and len(m2.frames) == len(R.model.frames)
    assert m2.total_mass() == pytest.approx(R.model.total_mass(), rel=1e-15)


def test_tables_regenerate_from_urdf():
    """The shipped JSON tables equal a fresh parse of the reference URDF/SRDF (stored as data
    under tests/golden/robots/)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
    import gen_models
    from pinoloco import model as mdl
    for name, lock in (("go2", None), ("b2g", [20])):
        fresh = gen_models.build(REF, name, lock)
        shipped = mdl.Model.load(os.path.join(os.path.dirname(__file__), "..", "pino-locoman_amd", "pinoloco",
                                              "models", f"{name}.json"))
        assert fresh.to_dict() == shipped.to_dict()
