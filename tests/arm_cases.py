"""The crafted end-effector cases of tests/golden/arm_cases.npz (tests/golden/make_golden_arm.py
`cases`): names at import time for parametrisation, and one dict per case.  Every output in the
file is the reference's own; `err` is the class name it raised, "" where it returned.

TunnelCost   T1 one base point . T2a-d resX != resY, four resZ (nZ 34 / 27 / 23 / 17, nK 18 / 15 /
13 / 9: nZ / 2 on a half rounds up and down) . T3 strong roll / pitch, yaw beyond +-pi/2 . T4cap /
T4back / T4wall a waypoint on a cell only the "never the sample / start node" rule keeps open . T5
tunnel outside the volume . T6 clipped by all six faces . T7a/b every base x = +-1e300 (all 10),
T7c the last base point alone at 1e300 . T8a-c NaN / inf base, NaN yaw, T8d a finite base of 1e308
whose node index is inf: the reference raises.
GetObstMap   G1 negative heights wrap . G2 below -sZ: IndexError . G3 iz >= sZ skipped . G4a-d xm /
ym on the grid: x only, y only, both, neither . G5a/b DEM 16x20 / 7x5 on a 12x12 volume . G6
obstacle values 2, NaN, 0.9999999 are ground . G7 exact halves, dyadic resZ . G8a/b 1x1x1, 3x3x2 .
G9a-c NaN / inf in a converted column, NaN outside the volume's extent, G9f a finite -1e308 whose
index is -inf: raises; G9d/e NaN / inf in the column / row the xm / ym test skips: returns . G10a
1e300 skipped, G10b -1e300 IndexError .
C1 / C2 the chain test's DEMs on T1's / T2b's volumes."""
import os

import numpy as np

_D = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arm_cases.npz"), allow_pickle=False)
T_NAMES = [str(s) for s in _D["t_names"]]
G_NAMES = [str(s) for s in _D["g_names"]]
T_ERR = dict(zip(T_NAMES, (str(s) for s in _D["t_err"])))
G_ERR = dict(zip(G_NAMES, (str(s) for s in _D["g_err"])))
T_OK = [n for n in T_NAMES if not T_ERR[n]]
T_RAISE = [n for n in T_NAMES if T_ERR[n]]
G_OK = [n for n in G_NAMES if not G_ERR[n]]
G_RAISE = [n for n in G_NAMES if G_ERR[n]]
T4 = [n for n in T_NAMES if n.startswith("T4")]
ERRORS = {"ValueError": ValueError, "OverflowError": OverflowError, "IndexError": IndexError}


def case(d, name):
    """Fields of one case from the loaded file d, `vol` split into shape / res (/ xy_m)."""
    c = {k[len(name) + 1:]: d[k] for k in d.files if k.startswith(name + "_")}
    vol = c.pop("vol")
    c["shape"] = tuple(int(v) for v in vol[:3])
    c["res"] = tuple(float(v) for v in vol[3:6])
    if len(vol) > 6:
        c["xy_m"] = (float(vol[6]), float(vol[7]))
    else:
        c["radii"] = tuple(float(v) for v in d["t_radii"])
    return c


def tunnel_args(c, fw=None, iw=None):
    """TunnelCost's positional arguments for a T case, optionally with other waypoints."""
    return (*c["radii"], c["base"], *c["shape"], *c["res"], c["heading"], c["finalWP"] if fw is None else fw,
            c["initWP"] if iw is None else iw)


def obst_args(c):
    """GetObstMap's positional arguments for a G case."""
    return (c["Z"], *c["res"], *c["shape"], c["obst"], *c["xy_m"])
