"""LETKF weight interpolation in NumPy, for the tests: written from the definition.

Grid of shape (ny, nx), column c = iy*nx + ix.  Nodes on an axis of n points with stride s: 0, s, 2s, .. below n-1, and n-1 (one
node if n == 1).  Node (jy, jx) has index jy*nxn + jx and is the grid column (node_y[jy], node_x[jx]).  Node pairs are those of
tests/_letkf.py at the nodes' positions.  Column (iy, ix) lies in the cell [y0, y1] x [x0, x1] of consecutive nodes (on a node line:
the cell with y0 < iy); ty = (iy - y0)/(y1 - y0), tx likewise (0 on an axis with one node); beta = (1-ty)(1-tx), (1-ty)tx, ty(1-tx),
ty tx on (y0,x0), (y0,x1), (y1,x0), (y1,x1); [T_c | w_c] = sum beta_n [T_n | w_n] in that order over the corners with beta != 0 (a
select: a corner with beta == 0 is not read).  If every corner in use has n_local == 0 the column's rows are copied."""
import numpy as np

import _etkf
import _letkf


def axis_nodes(n, s):
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    return np.append(np.arange(0, n - 1, s, dtype=np.int64), n - 1)


def axis_cell(i, nodes):
    """(j0, t): the lower node's index along the axis and the fraction of the way to the upper one."""
    if nodes.size == 1 or i == 0:
        return 0, 0.0
    j0 = int(np.searchsorted(nodes, i, side="left")) - 1        # nodes[j0] < i <= nodes[j0 + 1]
    return j0, float(i - nodes[j0]) / float(nodes[j0 + 1] - nodes[j0])


def mesh(ny, nx, stride):
    """dict: node_y, node_x, node_col (nnodes,) the grid column of every node, corner (ncol, 4) node indices (-1 where the corner
    does not exist), beta (ncol, 4)."""
    node_y, node_x = axis_nodes(ny, stride[0]), axis_nodes(nx, stride[1])
    nxn = node_x.size
    corner = np.full((ny * nx, 4), -1, dtype=np.int64)
    beta = np.zeros((ny * nx, 4))
    for iy in range(ny):
        jy, ty = axis_cell(iy, node_y)
        for ix in range(nx):
            jx, tx = axis_cell(ix, node_x)
            c = iy * nx + ix
            beta[c] = [(1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx]
            for n, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                if jy + dy < node_y.size and jx + dx < nxn:
                    corner[c, n] = (jy + dy) * nxn + jx + dx
    assert np.all(corner[beta != 0.0] >= 0)
    node_col = (node_y[:, None] * nx + node_x[None, :]).reshape(-1)
    return dict(node_y=node_y, node_x=node_x, node_col=node_col, corner=corner, beta=beta, ny=ny, nx=nx)


def column_pairs(m, Tn, wn, n_local=None):
    """T_c (ncol, M, M), w_c (ncol, M) and reached (ncol,) from the node pairs: plain float64 sums in the fixed corner order."""
    ncol, M = m["beta"].shape[0], Tn.shape[1]
    Tc, wc = np.empty((ncol, M, M)), np.empty((ncol, M))
    reached = np.zeros(ncol, dtype=bool)
    for c in range(ncol):
        T = w = None
        for n in range(4):
            b = m["beta"][c, n]
            if b != 0.0:                # a select: a corner with beta == 0 is never read
                k = m["corner"][c, n]
                T = b * Tn[k] if T is None else T + b * Tn[k]
                w = b * wn[k] if w is None else w + b * wn[k]
                if n_local is None or n_local[k] != 0:
                    reached[c] = True
        Tc[c], wc[c] = T, w
    return Tc, wc, reached


def apply_pairs(X, ncol, n_lead, Tc, wc, reached, rtpp=None):
    """Posterior member rows: reached columns through _etkf.etkf_members, the others copied."""
    X = np.asarray(X, dtype=np.float64)
    M = X.shape[1]
    post = np.empty_like(X)
    for c in range(ncol):
        rows = c + ncol * np.arange(n_lead)
        if not reached[c]:
            post[rows] = X[rows]
        else:
            T = Tc[c] if not rtpp else (1.0 - rtpp) * Tc[c] + rtpp * np.eye(M)
            post[rows] = _etkf.etkf_members(X[rows], T, wc[c])
    return post


def interp_cycle(X, HX, value, error, assim, ob_lat, ob_lon, ob_hw, grid_lat, grid_lon, n_lead, shape, stride):
    """The cycle with weight interpolation.  The obs block and the diagnostics are _letkf.letkf_cycle's; a unit stride is that
    function altogether."""
    plain = _letkf.letkf_cycle(X, HX, value, error, assim, ob_lat, ob_lon, ob_hw, grid_lat, grid_lon, n_lead)
    ny, nx = shape
    m = mesh(ny, nx, stride)
    if tuple(stride) == (1, 1):
        return dict(plain, mesh=m, node_stats=plain["stats"], Tn=plain["T"], wn=plain["w"], reached=plain["stats"]["n_local"] > 0)
    glat = np.asarray(grid_lat, dtype=np.float64).reshape(-1)
    glon = np.asarray(grid_lon, dtype=np.float64).reshape(-1)
    Tn, wn, st, rho = _letkf.weights(glat[m["node_col"]], glon[m["node_col"]], plain["prior_ym"], plain["prior_Yp"], value, error, assim,
                                     ob_lat, ob_lon, ob_hw)
    Tc, wc, reached = column_pairs(m, Tn, wn, st["n_local"])
    post = apply_pairs(X, ny * nx, n_lead, Tc, wc, reached)
    out = dict(plain)
    out.update(post=post, T=Tc, w=wc, mesh=m, node_stats=st, Tn=Tn, wn=wn, reached=reached, node_rho=rho, plain_post=plain["post"])
    return out
