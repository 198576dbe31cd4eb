"""Per-column multiplicative inflation of the LETKF, adaptive after Miyoshi (2011, MWR 139).

Every solve point x of `LETKF` / `SlabLETKF` (a column, a node of the weight mesh, a (slab group, column) pair) carries a factor
lambda(x) > 0 that enters its solve as Hunt's rho, A_x = ((M-1)/lambda_b) I + C_x, and is re-estimated from the innovations of the
observations that reach the point:

    p1 = sum_k w_k d_k^2,  p2 = trace(C_x)/(M-1),  p3 = sum_k rho_k            (w_k = rho_k/r_k over the obs with rho_k(x) != 0)
    lambda_o = (p1 - p3)/p2,  v_o = (2/p3) ((lambda_b p2 + p3)/p2)^2,  v_b = sigma_b^2
    lambda_a = clip(lambda_b + v_b/(v_o + v_b) (lambda_o - lambda_b), lower, upper)

The update of a cycle uses lambda_b; lambda_a is kept in `values` for the next one.  `sigma_b=0` is a fixed field.  A point no
observation reaches keeps its rows and its factor (this departs from Miyoshi's code, which inflates such a point by its factor).
The obs block: an observation with the default point interpolation is solved under that interpolation of the field,
lambda_ob[j] = sum_e wts[j, e] lambda_row[idx[j, e]] over its stencil, lambda_row the field expanded to state rows (with a
weight_stride the node field is first expanded to columns bilinearly in grid-index space); observations with a user-defined
forward operator take 1.0."""
import numpy as np


class ColumnInflation(object):
    def __init__(self, initial=1.0, sigma_b=0.04, lower=1e-2, upper=1e2, values=None):
        """initial: the factor every solve point starts from; sigma_b: the prior standard deviation of the factor (0.04 is
        Miyoshi's value; 0: the field is fixed); lower, upper: guards of the algebra, not tuning; values: a field from an earlier
        run, in the shape of the solve layout -- (ny, nx), (nyn, nxn) with a weight_stride, a leading ngroups axis for
        `SlabLETKF` -- checked at the first update."""
        sigma_b, lower, upper, initial = float(sigma_b), float(lower), float(upper), float(initial)
        if not (np.isfinite(sigma_b) and sigma_b >= 0.0):
            raise ValueError("ColumnInflation: sigma_b=%r must be finite and >= 0" % (sigma_b,))
        if not (np.isfinite(lower) and np.isfinite(upper) and 0.0 < lower <= upper):
            raise ValueError("ColumnInflation: the bounds must be finite with 0 < lower <= upper, got (%r, %r)" % (lower, upper))
        if not (np.isfinite(initial) and lower <= initial <= upper):
            raise ValueError("ColumnInflation: initial=%r must lie within [%r, %r]" % (initial, lower, upper))
        self.initial, self.sigma_b, self.lower, self.upper = initial, sigma_b, lower, upper
        self.values = None
        if values is not None:
            self.values = self._checked(np.array(values, dtype=np.float64))

    def _checked(self, v):
        if not (np.all(np.isfinite(v)) and np.all(v >= self.lower) and np.all(v <= self.upper)):
            raise ValueError("ColumnInflation: values must be finite and within [%r, %r]" % (self.lower, self.upper))
        return v

    def field(self, shape):
        """The (validated) field for a solve layout of `shape`: created from `initial` at the first update, ValueError when the
        values at hand have another shape or left the bounds."""
        shape = tuple(int(s) for s in shape)
        if self.values is None:
            self.values = np.full(shape, self.initial, dtype=np.float64)
        if self.values.shape != shape:
            raise ValueError("ColumnInflation: values have shape %r but the filter solves on %r" % (self.values.shape, shape))
        return self._checked(self.values)

    def save(self, path):
        if self.values is None:
            raise ValueError("ColumnInflation: no values yet (they are created at the first update)")
        np.save(path, self.values)

    def load(self, path):
        self.values = self._checked(np.array(np.load(path), dtype=np.float64))
        return self


def _axis_cells(n, nodes):
    """(j0 (n,), t (n,)): for every grid index the lower node of its cell and the fraction of the way to the upper one (7y-2: on a
    node line the cell below; 0 on an axis with one node)."""
    nodes = np.asarray(nodes, dtype=np.int64)
    i = np.arange(n)
    if nodes.size == 1:
        return np.zeros(n, dtype=np.int64), np.zeros(n)
    j0 = np.maximum(np.searchsorted(nodes, i, side="left") - 1, 0)
    t = (i - nodes[j0]) / (nodes[j0 + 1] - nodes[j0]).astype(np.float64)
    return j0, t


def expand_nodes(field, node_y, node_x, ny, nx):
    """The node field (..., nyn, nxn) to the grid's columns (..., ny, nx), bilinearly in grid-index space as the weights are."""
    field = np.asarray(field, dtype=np.float64)
    jy, ty = _axis_cells(ny, node_y)
    jx, tx = _axis_cells(nx, node_x)
    jy1 = np.minimum(jy + 1, field.shape[-2] - 1)
    jx1 = np.minimum(jx + 1, field.shape[-1] - 1)
    ty, tx = ty[:, None], tx[None, :]
    f = lambda a, b: field[..., a[:, None], b[None, :]]
    return (1.0 - ty) * (1.0 - tx) * f(jy, jx) + (1.0 - ty) * tx * f(jy, jx1) + ty * (1.0 - tx) * f(jy1, jx) + ty * tx * f(jy1, jx1)


def ob_factors(field_cols, group_of_slab, idx, wts):
    """lambda_ob (P,) from the column field (ngroups, ncol), the group of every slab (n_lead,) and the obs' stencils (idx (P, E)
    global state rows lead * ncol + col, wts (P, E)): the forward operator applied to the field expanded to state rows."""
    field_cols = np.asarray(field_cols, dtype=np.float64)
    ncol = field_cols.shape[1]
    idx = np.asarray(idx, dtype=np.int64)
    wts = np.asarray(wts, dtype=np.float64)
    idx = np.where(wts != 0.0, idx, 0)          # an entry without weight is never read
    lam = field_cols[np.asarray(group_of_slab, dtype=np.int64)[idx // ncol], idx % ncol]
    return np.sum(np.where(wts != 0.0, wts * lam, 0.0), axis=1)
