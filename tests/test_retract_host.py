"""Layout of the batched retract (pl_ocp_retract_sizes) and its argument errors, without a
GPU: widths and row counts against Layout for every dynamics variant, offsets that tile the
packed buffer, centroidal_vel's v rows ignoring the terminal row, and PinolocoError for a
retract on a host-only handle, steps outside [1, N] and a terminal row with steps < N."""
import numpy as np
import pytest

from conftest import make_robot

N, B = 6, 3
FIELDS = ("q", "v", "a", "forces", "tau", "eom_base")
# (robot, dynamics, constructor arguments)
VARIANTS = [("go2", "whole_body_rnea", {}),
            ("go2", "whole_body_rnea", {"include_acc": False}),
            ("go2", "whole_body_acc", {}),
            ("go2", "whole_body_acc", {"include_base": False}),
            ("go2", "whole_body_aba", {}),
            ("go2", "centroidal_vel", {}),
            ("go2", "centroidal_vel", {"include_base": False}),
            ("go2", "centroidal_acc", {}),
            ("go2", "centroidal_acc", {"include_base": False}),
            ("b2g", "whole_body_rnea", {})]
IDS = [f"{r}-{d}" + "".join(f"-{k}0" for k in kw) for r, d, kw in VARIANTS]


def _host(rname, dyn, kw, batch=B):
    from pinoloco.ocp import BatchedOCP
    R = make_robot(rname)
    return R, BatchedOCP(R, dyn, N, batch=batch, device=-1, **kw)


@pytest.mark.parametrize("rname,dyn,kw", VARIANTS, ids=IDS)
@pytest.mark.parametrize("steps,terminal", [(2, False), (N, False), (N, True)])
def test_retract_sizes_match_layout(rname, dyn, kw, steps, terminal):
    R, bo = _host(rname, dyn, kw)
    lay = bo.layout
    sz = bo.retract_sizes(steps, terminal)
    cv = dyn == "centroidal_vel"
    fd = dyn == "whole_body_rnea" and not kw.get("include_acc", True)
    want_w = {"q": lay.nq, "v": lay.nv, "a": 0 if fd else lay.nv, "forces": lay.nf, "tau": lay.nj, "eom_base": 6}
    t = int(terminal)
    want_r = {"q": steps + t, "v": steps + (0 if cv else t), "a": steps, "forces": steps, "tau": steps,
              "eom_base": steps}
    if rname == "b2g":
        assert lay.nf == 15  # the external-force frame
    off = 0
    for f in FIELDS:
        assert sz[f]["width"] == want_w[f], f
        assert sz[f]["rows"] == want_r[f], f
        assert sz[f]["offset"] == off, f  # the fields tile the buffer in order, no gaps
        off += B * want_r[f] * want_w[f]
    assert sz["total"] == off
    bo.close()


def test_retract_sizes_default_is_every_node():
    R, bo = _host("go2", "whole_body_rnea", {})
    assert bo.retract_sizes() == bo.retract_sizes(N, False)
    assert bo.retract_sizes()["q"]["rows"] == N
    bo.close()


def test_centroidal_vel_v_rows_ignore_terminal():
    """v comes from the inputs U[0..N-1]: the terminal node adds a row to q only."""
    for kw in ({}, {"include_base": False}):
        R, bo = _host("go2", "centroidal_vel", kw)
        a, b = bo.retract_sizes(N, False), bo.retract_sizes(N, True)
        assert a["v"]["rows"] == b["v"]["rows"] == N
        assert (a["q"]["rows"], b["q"]["rows"]) == (N, N + 1)
        bo.close()


def test_retract_errors():
    from pinoloco._lib import PinolocoError
    R, bo = _host("go2", "whole_body_rnea", {})
    for steps, terminal in [(0, False), (N + 1, False), (2, True), (-1, False)]:
        with pytest.raises(PinolocoError):
            bo.retract_sizes(steps, terminal)
        with pytest.raises(PinolocoError):
            bo.retract(steps, terminal)
    with pytest.raises(PinolocoError, match="no device"):
        bo.retract(2, False)  # host-only handle
    with pytest.raises(PinolocoError, match="no device"):
        bo.retract_device(np.zeros(1).ctypes.data, 2, False)
    bo.close()


def test_null_handle_is_an_error():
    import ctypes as C
    from pinoloco import _lib
    out = (C.c_longlong * 19)()
    assert _lib.lib().pl_ocp_retract_sizes(None, 2, 0, out) != 0
    assert b"null handle" in _lib.lib().pl_last_error()
    assert _lib.lib().pl_ocp_retract(None, 2, 0, None, None, None, None, None, None) != 0
    assert _lib.lib().pl_ocp_retract_device(None, 2, 0, None) != 0
