"""The end-effector volume restatement (oracle/arm_oracle.py) against the reference's own
GetObstMap / TunnelCost outputs (tests/golden/arm.npz and the crafted per-branch cases of
tests/golden/arm_cases.npz, both from tests/golden/make_golden_arm.py).  Bit-exact where the
reference returns, the same exception class where it raises; no GPU."""
import numpy as np
import pytest

import arm_cases as AC
import arm_oracle as AO


def _case(golden, i):
    d = golden("arm")
    return {k[len(f"a{i}_"):]: d[k] for k in d.files if k.startswith(f"a{i}_")}


@pytest.mark.parametrize("i", range(3))
def test_get_obst_map_golden(golden, i):
    c = _case(golden, i)
    sX, sY, sZ = (int(v) for v in c["shape"])
    resX, resY, resZ = c["res"]
    fm, om, gm = AO.get_obst_map(c["Z"], resX, resY, resZ, sX, sY, sZ, c["obst"], *c["xy_m"])
    assert np.array_equal(fm, c["finalMap"]) and np.array_equal(om, c["obstMap"]) and np.array_equal(gm, c["groundMap"])


@pytest.mark.parametrize("i", range(3))
def test_tunnel_cost_golden(golden, i):
    c = _case(golden, i)
    sX, sY, sZ = (int(v) for v in c["shape"])
    resX, resY, resZ = c["res"]
    Rlim, rO, rm = c["radii"]
    got = AO.tunnel_cost(Rlim, rO, rm, c["base"], sX, sY, sZ, resX, resY, resZ, c["heading"], c["finalWP"], c["initWP"])
    ref = c["tunnel"]
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), int((got != ref).sum())


# ---- crafted per-branch cases (tests/golden/arm_cases.npz, listed in tests/arm_cases.py)
def test_cases_file_is_small_and_data_only(golden):
    import os

    d = golden("arm_cases")  # allow_pickle=False
    assert all(d[k].dtype.kind in "fuU" for k in d.files)
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "arm_cases.npz")) < os.path.getsize(os.path.join(here, "arm.npz"))
    assert set(AC.T4) == {"T4cap", "T4back", "T4wall"} and len(AC.T_RAISE) == 4 and len(AC.G_RAISE) == 6


@pytest.mark.parametrize("name", AC.G_OK)
def test_get_obst_map_cases(golden, name):
    c = AC.case(golden("arm_cases"), name)
    fm, om, gm = AO.get_obst_map(*AC.obst_args(c))
    assert np.array_equal(fm, c["finalMap"]) and np.array_equal(om, c["obstMap"]) and np.array_equal(gm, c["groundMap"])


@pytest.mark.parametrize("name", AC.G_RAISE)
def test_get_obst_map_raises_as_the_reference(golden, name):
    c = AC.case(golden("arm_cases"), name)
    with pytest.raises(AC.ERRORS[AC.G_ERR[name]]):
        AO.get_obst_map(*AC.obst_args(c))


@pytest.mark.parametrize("name", AC.T_OK)
def test_tunnel_cost_cases(golden, name):
    c = AC.case(golden("arm_cases"), name)
    got = AO.tunnel_cost(*AC.tunnel_args(c))
    assert got.shape == c["tunnel"].shape
    assert np.array_equal(got, c["tunnel"]), int((got != c["tunnel"]).sum())


@pytest.mark.parametrize("name", AC.T_RAISE)
def test_tunnel_cost_raises_as_the_reference(golden, name):
    c = AC.case(golden("arm_cases"), name)
    with pytest.raises(AC.ERRORS[AC.T_ERR[name]]):
        AO.tunnel_cost(*AC.tunnel_args(c))


@pytest.mark.parametrize("name", AC.T4)
def test_waypoint_exemption_decides_t4(golden, name):
    """Mutation check: with the waypoints moved to the far corner (no exemption at the crafted cell)
    the restatement must differ from the reference's output, at exactly that cell, where it closes."""
    c = AC.case(golden("arm_cases"), name)
    far = np.uint32([s - 1 for s in c["shape"]])
    moved = AO.tunnel_cost(*AC.tunnel_args(c, fw=far, iw=far))
    diff = np.argwhere(moved != c["tunnel"])
    wp = c["finalWP"] if not np.array_equal(c["finalWP"], far) else c["initWP"]
    assert diff.tolist() == [[int(wp[1]), int(wp[0]), int(wp[2])]]
    assert np.isinf(moved[tuple(diff[0])]) and np.isfinite(c["tunnel"][tuple(diff[0])])
