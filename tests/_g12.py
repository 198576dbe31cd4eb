"""G12 (tests/golden/make_goldens.py `main_g12`): Gaspari-Cohn, 2 500 obs x 100 members, made by the reference.

The file leaves out HX, which its other arrays determine exactly; `load_g12` puts it back: every G12 stencil is one
row with weight 1, and LinOb.estimate returns that row's copy, so HX is X's picked rows.
"""
from conftest import load_golden


def load_g12():
    g = load_golden("G12")
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    assert g["sten_idx"].shape[1] == 1 and (g["sten_wts"][:, 0] == 1.0).all()
    assert "HX" not in g
    g["HX"] = g["X"].reshape(N, M)[g["sten_idx"][:, 0]]
    return g
