"""Spatially varying adaptive inflation (Anderson 2009), for the localised EnSRF.

Keeps the surface of the reference's `AdaptiveInflation`
(efa_xray/assimilation/adaptive_inflation.py): `AdaptiveInflation(priorstate,
priorinf)` with `priorinf = (inftype, infile, initvals)` loads `infile` or, on
any failure, builds a field from `initvals = (mean, std)`;
`build_initial_inflation`, `inflate_state(priorstate)` and
`save_to_disk(filename)`.  The reference never updates the field; here
`EnSRF(state, obs, loc='GC', adaptive_inflation=ai).update()` does, on the
device, and writes the new field back into `ai.inflation`.

The field holds, per state variable, a (validtime, y, x, moment) array with
moment = ['mean', 'std']: the mean and standard deviation of each grid point's
VARIANCE inflation factor.  Documented deviation: `inflate_state` scales the
perturbations by sqrt(mean), not by mean as the reference does (the two agree at
mean = 1), so that the field is the variance factor Anderson's update assumes.
"""
from collections import OrderedDict

import numpy as np

from efa_xray_amd.state.ensemble import EnsembleState

_IDIMS = ("validtime", "y", "x", "moment")
MOMENTS = ("mean", "std")


class InflationField(object):
    """The inflation field: `variables[name]` is (nt, ny, nx, 2); `coords` holds validtime (lead hours from the first
    valid time), lat / lon on (y, x) and moment.  `to_vect()` / `from_vect()` give the (nstate, 2) rows in the state's
    `to_vect()` order."""

    def __init__(self, variables, coords):
        self.variables = OrderedDict((n, np.ascontiguousarray(v, dtype=np.float64)) for n, v in variables.items())
        self.coords = dict(coords)

    def __getitem__(self, key):
        return self.coords[key] if key in self.coords else self.variables[key]

    def vars(self):
        return list(self.variables.keys())

    def to_vect(self):
        return np.ascontiguousarray(np.concatenate([v.reshape(-1, 2) for v in self.variables.values()], axis=0))

    def from_vect(self, vect):
        vect = np.asarray(vect, dtype=np.float64)
        r0 = 0
        for name, v in self.variables.items():
            n = v.size // 2
            self.variables[name] = np.ascontiguousarray(vect[r0:r0 + n].reshape(v.shape))
            r0 += n

    def to_xarray(self):
        import xarray  # optional
        vd = dict((n, (list(_IDIMS), v)) for n, v in self.variables.items())
        cd = {"validtime": self.coords["validtime"], "lat": (["y", "x"], self.coords["lat"]),
              "lon": (["y", "x"], self.coords["lon"]), "moment": list(MOMENTS)}
        return xarray.Dataset(vd, cd)


def _lead_hours(valids):
    """Valid times as lead hours from the first one (the reference's `leads`); numeric times are taken as seconds."""
    v = np.asarray(valids)
    if v.dtype.kind == "M":
        return ((v - v[0]) / np.timedelta64(1, "s")).astype(np.float64) / 3600.0
    v = v.astype(np.float64)
    return (v - v[0]) / 3600.0


def _grid_latlon(state):
    ny, nx = state.ny(), state.nx()
    lat, lon = state.column_latlon()
    return lat.reshape(ny, nx), lon.reshape(ny, nx)


def _read_field(filename):
    """An InflationField from a file written by `save_to_disk` (xarray when importable, else scipy's netCDF-3 reader)."""
    try:
        import xarray
    except ImportError:
        xarray = None
    variables, coords = OrderedDict(), {}
    if xarray is not None:
        with xarray.open_dataset(filename) as ds:
            for name in ds.data_vars:
                if tuple(ds[name].dims) == _IDIMS:
                    variables[name] = np.asarray(ds[name].values, dtype=np.float64)
            for c in ("validtime", "lat", "lon"):
                coords[c] = np.asarray(ds[c].values, dtype=np.float64)
    else:
        from scipy.io import netcdf_file
        with netcdf_file(filename, "r", mmap=False) as f:
            for name, var in f.variables.items():
                if tuple(var.dimensions) == _IDIMS:
                    variables[name] = np.array(var[:], dtype=np.float64)
            for c in ("validtime", "lat", "lon"):
                coords[c] = np.array(f.variables[c][:], dtype=np.float64)
    if not variables:
        raise ValueError("%s holds no (validtime, y, x, moment) inflation variable" % filename)
    coords["moment"] = np.array(MOMENTS)
    return InflationField(variables, coords)


class AdaptiveInflation(object):
    """A per-grid-point prior inflation field that EnSRF(..., loc='GC', adaptive_inflation=...) applies and then re-estimates
    from the innovations, ob by ob (the variance-factor update of Anderson 2009, Tellus 61A).

    priorinf = (inftype, infile, initvals): inftype is kept as given; the field is read from infile, and when that is not
    possible every grid point starts at initvals = (mean, std).  lower / upper bound the mean and sd_lower the std
    (defaults as in DART: 1, 1e6, 0).  The field's values must be finite with the mean in [lower, upper] and std >= 0."""

    def __init__(self, priorstate, priorinf, lower=1.0, upper=1e6, sd_lower=0.0):
        if not isinstance(priorstate, EnsembleState):
            raise TypeError("priorstate must be an EnsembleState")
        inftype, infile, initvals = priorinf
        self.inftype = inftype  # stored, not interpreted (as in the reference)
        lower, upper, sd_lower = float(lower), float(upper), float(sd_lower)
        if not (np.isfinite(lower) and lower > 0.0 and np.isfinite(upper) and upper >= lower and
                np.isfinite(sd_lower) and sd_lower >= 0.0):
            raise ValueError("bounds must satisfy 0 < lower <= upper (finite) and sd_lower >= 0; got %r, %r, %r"
                             % (lower, upper, sd_lower))
        self.lower, self.upper, self.sd_lower = lower, upper, sd_lower
        try:
            self.inflation = _read_field(infile)
        except Exception:
            self.inflation = self.build_initial_inflation(priorstate, initvals)
        self.check_values()

    def build_initial_inflation(self, priorstate, initvals):
        """A field on `priorstate`'s grid and valid times (as lead hours) with the same (mean, std) = initvals everywhere."""
        moments = np.asarray(initvals, dtype=np.float64).reshape(2)
        fields = OrderedDict((name, np.broadcast_to(moments, arr.shape[:3] + (2,)).copy())
                             for name, arr in priorstate.variables.items())
        lat, lon = _grid_latlon(priorstate)
        coords = dict(validtime=_lead_hours(priorstate.coords.get("validtime", np.arange(priorstate.ntimes()))),
                      lat=lat, lon=lon, moment=np.array(MOMENTS))
        return InflationField(fields, coords)

    def check_values(self):
        """ValueError unless every mean is finite and in [lower, upper] and every std is finite and >= 0 (a mean <= 0 would
        turn the inflated prior into NaN)."""
        v = self.inflation.to_vect()
        mean, std = v[:, 0], v[:, 1]
        if not (np.all(np.isfinite(v)) and np.all(mean >= self.lower) and np.all(mean <= self.upper) and np.all(std >= 0.0)):
            raise ValueError("inflation field: every mean must be finite and in [lower, upper] = [%g, %g] and every std "
                             "finite and >= 0" % (self.lower, self.upper))

    def check_state(self, state):
        """ValueError unless the field covers `state` (the same variables, (validtime, y, x) shape and grid) and its values
        are valid (check_values)."""
        f = self.inflation
        if f.vars() != state.vars():
            raise ValueError("inflation field variables %r differ from the state's %r" % (f.vars(), state.vars()))
        for name in state.vars():
            want = state.variables[name].shape[:3] + (2,)
            if f.variables[name].shape != want:
                raise ValueError("inflation field %r has shape %r, the state needs %r" % (name, f.variables[name].shape, want))
        lat, lon = _grid_latlon(state)
        if not (np.array_equal(np.asarray(f.coords["lat"]).reshape(lat.shape), lat) and
                np.array_equal(np.asarray(f.coords["lon"]).reshape(lon.shape), lon)):
            raise ValueError("inflation field grid (lat/lon) differs from the state's")
        self.check_values()

    def inflate_state(self, priorstate):
        """A NEW state: every member x <- mean + sqrt(lambda) (x - mean), lambda the field's mean at its grid point
        (points with lambda == 1 keep their values bit for bit)."""
        self.check_state(priorstate)
        out = OrderedDict()
        for name, x in priorstate.variables.items():
            lam = self.inflation.variables[name][..., 0:1]
            mean = x.mean(axis=-1, keepdims=True)
            out[name] = np.where(lam == 1.0, x, mean + np.sqrt(lam) * (x - mean))
        return type(priorstate)(out, dict((k, np.array(v, copy=True)) for k, v in priorstate.coords.items()))

    def save_to_disk(self, filename="prior_inflation.nc"):
        """Write the current field to a netCDF file: with xarray when it imports (as the reference), else as classic
        netCDF-3 through scipy, as `EnsembleState.save_to_disk` does."""
        try:
            import xarray  # noqa: F401
        except ImportError:
            return self._save_netcdf3(filename)
        self.inflation.to_xarray().to_netcdf(filename)

    def _save_netcdf3(self, filename):
        from scipy.io import netcdf_file
        f0 = self.inflation
        nt, ny, nx, _ = next(iter(f0.variables.values())).shape
        with netcdf_file(filename, "w", version=2) as f:
            f.history = "efa_xray_amd AdaptiveInflation.save_to_disk"
            f.moments = " ".join(MOMENTS)
            for d, n in zip(_IDIMS, (nt, ny, nx, 2)):
                f.createDimension(d, n)
            f.createVariable("validtime", "d", ("validtime",))[:] = np.asarray(f0.coords["validtime"], dtype=np.float64)
            f.variables["validtime"].units = "hours"
            for c in ("lat", "lon"):
                f.createVariable(c, "d", ("y", "x"))[:] = np.asarray(f0.coords[c], dtype=np.float64)
            for name, val in f0.variables.items():
                f.createVariable(name, "d", _IDIMS)[:] = val
