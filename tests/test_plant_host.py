"""The plant settings of the device MPC loop (pl_mpc_set_plant / pl_mpc_get_plant /
pl_mpc_set_disturbance, include/pinoloco.h) on host-only handles: the setter is a setting and
round-trips without a device, every refused argument comes back as PinolocoError with a
message, and the disturbance buffers need a device."""
import numpy as np
import pytest

from conftest import make_robot


def _host(dyn="whole_body_rnea", batch=2, **kw):
    from pinoloco.ocp import BatchedOCP
    return BatchedOCP(make_robot("go2"), dyn, 6, batch=batch, device=-1, **kw)


def test_plant_setting_round_trips():
    bo = _host()
    assert bo.mpc_get_plant() == ("nominal", 1)  # the default: the reference's own loop
    for mode, sub in (("aba", 1), ("aba", 16), ("nominal", 4), ("aba", 3), ("nominal", 1)):
        bo.mpc_set_plant(mode, sub)
        assert bo.mpc_get_plant() == (mode, sub)
    bo.mpc_set_plant()  # the defaults of the call: "aba", one substep
    assert bo.mpc_get_plant() == ("aba", 1)
    bo.close()


@pytest.mark.parametrize("dyn,kw", [("whole_body_rnea", {}), ("whole_body_rnea", {"include_acc": False}),
                                    ("whole_body_acc", {}), ("whole_body_acc", {"include_base": False}),
                                    ("whole_body_aba", {}), ("centroidal_acc", {}),
                                    ("centroidal_acc", {"include_base": False})])
def test_aba_plant_allowed_on_every_q_v_state(dyn, kw):
    bo = _host(dyn, **kw)
    bo.mpc_set_plant("aba", 4)
    assert bo.mpc_get_plant() == ("aba", 4)
    bo.close()


def test_bad_plant_arguments_are_errors():
    from pinoloco import _lib
    bo = _host()
    bo.mpc_set_plant("aba", 2)
    for sub in (0, 17, -1):
        with pytest.raises(_lib.PinolocoError, match="substeps"):
            bo.mpc_set_plant("aba", sub)
        with pytest.raises(_lib.PinolocoError, match="substeps"):
            bo.mpc_set_plant("nominal", sub)
    with pytest.raises(_lib.PinolocoError, match="mode"):
        bo.mpc_set_plant("rk4", 1)
    assert _lib.lib().pl_mpc_set_plant(bo.h, 2, 1) < 0  # an unknown code at the C-ABI itself
    assert b"mode" in _lib.lib().pl_last_error()
    assert _lib.lib().pl_mpc_set_plant(None, 1, 1) < 0
    assert bo.mpc_get_plant() == ("aba", 2)  # a refused call changes nothing
    bo.close()


@pytest.mark.parametrize("include_base", [True, False])
def test_aba_plant_refused_on_centroidal_vel(include_base):
    """x = [h, q] there; the plant is defined on x = [q, v]."""
    from pinoloco import _lib
    bo = _host("centroidal_vel", include_base=include_base)
    with pytest.raises(_lib.PinolocoError, match="centroidal_vel"):
        bo.mpc_set_plant("aba", 1)
    bo.mpc_set_plant("nominal", 2)  # the default plant stays selectable
    assert bo.mpc_get_plant() == ("nominal", 2)
    bo.close()


def test_disturbance_needs_a_device_and_right_shapes():
    from pinoloco import _lib
    bo = _host(batch=2)
    ndx = bo.layout.ndx
    with pytest.raises(_lib.PinolocoError, match="device"):
        bo.mpc_set_disturbance(np.zeros((2, 6)), np.zeros((2, ndx)))
    with pytest.raises(_lib.PinolocoError, match="device"):
        bo.mpc_set_disturbance()
    for w in (np.zeros((2, 5)), np.zeros((3, 6)), np.zeros(6), np.zeros((2, 6, 1))):
        with pytest.raises(_lib.PinolocoError, match="base_wrench"):
            bo.mpc_set_disturbance(base_wrench=w)
    for z in (np.zeros((2, ndx + 1)), np.zeros((1, ndx)), np.zeros((2, bo.layout.nx)), np.zeros(2 * ndx)):
        with pytest.raises(_lib.PinolocoError, match="state_noise"):
            bo.mpc_set_disturbance(state_noise=z)
    bo.close()
