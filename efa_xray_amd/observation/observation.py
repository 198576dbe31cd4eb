"""Observation record + localisation helpers.

Same constructor, attributes and methods as the reference's `Observation`
(efa_xray/observation/observation.py:17-146).  `localize`, `gaspari_cohn` and
`haversine` are kept as NumPy functions because user code calls them (e.g. to
plot a localisation footprint); `EnSRF.update` does NOT call them -- the
taper is evaluated inside the HIP kernels from (lat, lon, localize_radius).
"""
import numpy as np

from efa_xray_amd.state.ensemble import EnsembleState

EARTH_RADIUS_KM = 6371.0


class Observation(object):
    def __init__(self, value=None, obtype=None, time=None, error=None, lat=None,
                 lon=None, vert=None,
                 prior_mean=None, post_mean=None, prior_var=None, post_var=None,
                 assimilate_this=False, description=None, localize_radius=None,
                 vert_localize_radius=None):
        # observation.py:18-36 (note: assimilate_this defaults to False there too).  vert_localize_radius is this
        # project's own: the vertical half-width that goes with `vert`, in the unit of `vert`
        if vert_localize_radius is not None:
            check_vert_halfwidth(vert_localize_radius)
        self.value = value
        self.obtype = obtype
        self.time = time
        self.error = error
        self.lat = lat
        self.lon = lon
        self.vert = vert
        self.prior_mean = prior_mean
        self.post_mean = post_mean
        self.prior_var = prior_var
        self.post_var = post_var
        self.assimilate_this = assimilate_this
        self.assimilated = False
        self.description = description
        self.localize_radius = localize_radius
        self.vert_localize_radius = vert_localize_radius

    # This project's own as well: the temporal half-width that goes with `time`, in hours when the state's
    # validtime is datetime64, else in validtime's own unit.  An attribute, not a constructor parameter (the constructor's
    # parameter list is the reference's plus vert_localize_radius); checked when it is set.  None: no temporal taper.
    _time_localize_radius = None

    @property
    def time_localize_radius(self):
        return self._time_localize_radius

    @time_localize_radius.setter
    def time_localize_radius(self, c):
        if c is not None:
            check_vert_halfwidth(c, "time_localize_radius")
        self._time_localize_radius = c

    def estimate(self, state):
        """Ensemble estimate of this ob: interpolate the matching field
        (observation.py:40-50)."""
        return state.interpolate(self.obtype, self.time, self.lat, self.lon)

    def stencil(self, state):
        """The same estimate as a linear stencil (state rows, weights) so the
        forward operator can run on the GPU (efa_forward_stencil_dev)."""
        return state.interp_stencil(self.obtype, self.time, self.lat, self.lon)

    def distance_to_state(self, state):
        return state.distance_to_point(self.lat, self.lon)

    def localize(self, state, type='GC', full_state=False):
        """Gaspari-Cohn weights of this ob against a state grid or a list of
        observations (observation.py:59-87).  Unlike the reference, a missing
        localize_radius returns ones instead of raising in abs(None)."""
        halfwidth = self.localize_radius
        if isinstance(state, EnsembleState):
            distances = state.distance_to_point(self.lat, self.lon)
        else:
            ourloc = (self.lat, self.lon)
            distances = np.array([haversine(ourloc, (ob.lat, ob.lon)) for ob in state])
        if halfwidth is None:
            return np.ones(distances.shape)
        if type == 'GC':
            return gaspari_cohn(distances, halfwidth)
        raise ValueError("unknown localization type %r" % (type,))


def check_vert_halfwidth(c, where="vert_localize_radius"):
    """A vertical (or temporal) half-width as a float; ValueError unless it is a finite number > 0."""
    try:
        v = float(c)
    except (TypeError, ValueError):
        raise ValueError("%s=%r: expected a number" % (where, c))
    if not np.isfinite(v) or v <= 0.0:
        raise ValueError("%s=%r: expected a finite number > 0" % (where, c))
    return v


def gaspari_cohn(distances, halfwidth):
    """observation.py:117-130."""
    r = np.divide(distances, abs(halfwidth))
    weights = np.zeros(np.shape(r))
    inner = r <= 1.0
    outer = (r > 1.0) & (r < 2.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        weights[inner] = ((((-0.25 * r + 0.5) * r + 0.625) * r - 5.0 / 3.0) * r ** 2 + 1.0)[inner]
        weights[outer] = (((((r / 12.0 - 0.5) * r + 0.625) * r + 5.0 / 3.0) * r - 5.0) * r + 4.0
                          - 2.0 / (3.0 * r))[outer]
    return weights


def haversine(loc1, loc2):
    """observation.py:135-146."""
    lat1 = np.radians(loc1[0])
    lat2 = np.radians(loc2[0])
    dlat = lat2 - lat1
    dlon = np.radians(loc2[1] - loc1[1])
    a = np.sin(dlat / 2) ** 2 + np.cos(lat1) * np.cos(lat2) * np.sin(dlon / 2) ** 2
    return EARTH_RADIUS_KM * (2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a)))
