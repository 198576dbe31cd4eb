"""The LETKF's cap on the local observations of a solve in NumPy, for the tests: written from the definition.

At a solve point, of the obs of class c with a non-zero taper (an ob with a flag of 0 has a taper of 0: tests/_letkf.py's taper),
the caps[c] with the largest taper keep it, equal tapers ordered by lower ob index first, and the others get 0; caps[c] = 0 is no
limit.  The cycle is tests/_letkf.py's (and its kin's: _letkf_interp, _letkf_infl, _letkf_control) on the selected tapers: `capped`
puts `select` behind `_letkf.taper`, which all of them call.

The device's taper differs from the oracle's in its last bits (near 1e-12 absolute for half-widths >= 200 km), so a
near-tie at the cap would make model and device pick different obs.  `select` therefore asserts that, wherever a cap bites, the
last winner and the first loser differ by at least MIN_GAP absolute unless they are equal to the bit: a condition on the inputs,
not a tolerance on the result."""
import contextlib

import numpy as np

import _letkf

MIN_GAP = 1e-9


def select(rho, ob_class, caps, min_gap=MIN_GAP, last_first=False, info=None):
    """rho (npts, P) with the losers' tapers zeroed.  ob_class (P,) ints or None (all class 0); last_first: equal tapers ordered by
    HIGHER index first (the opposite rule, for the tests that must be able to fail); info: a dict that receives reach (npts,
    nclass), bites (npts,) and gap (the smallest winner-loser gap that is not a bit-equal tie, inf when there is none)."""
    rho = np.asarray(rho, dtype=np.float64)
    npts, P = rho.shape
    caps = [int(c) for c in caps]
    cls = np.zeros(P, dtype=np.int64) if ob_class is None else np.asarray(ob_class, dtype=np.int64)
    assert cls.shape == (P,) and (P == 0 or (cls.min() >= 0 and cls.max() < len(caps))) and min(caps) >= 0
    out = rho.copy()
    reach = np.zeros((npts, len(caps)), dtype=np.int64)
    bites = np.zeros(npts, dtype=bool)
    gap = np.inf
    for i in range(npts):
        for c, cap in enumerate(caps):
            cand = np.flatnonzero((rho[i] != 0.0) & (cls == c))
            reach[i, c] = cand.size
            if cap == 0 or cand.size <= cap:
                continue
            if last_first:
                cand = cand[::-1]
            order = cand[np.argsort(-rho[i, cand], kind="stable")]
            a, b = rho[i, order[cap - 1]], rho[i, order[cap]]
            if a != b:
                gap = min(gap, a - b)
                assert a - b >= min_gap, "point %d, class %d: the last winner %r and the first loser %r are a near-tie" % (i, c, a, b)
            out[i, order[cap:]] = 0.0
            bites[i] = True
    if info is not None:
        info.update(reach=reach, bites=bites, gap=gap)
    return out


def n_local(reach, caps):
    """sum_c min(cap_c, reach_c) per point, a cap of 0 being no limit."""
    caps = np.asarray(caps, dtype=np.int64)
    return np.where(caps[None, :] > 0, np.minimum(reach, caps[None, :]), reach).sum(axis=1)


@contextlib.contextmanager
def capped(ob_class, caps, **kw):
    """Within the block tests/_letkf.py's taper is the selected one: every model of the family then runs under the cap.  Yields the
    list of the `info` dicts of the calls, in call order (for letkf_cycle: the grid's, then the obs')."""
    plain = _letkf.taper
    log = []

    def taper(*args):
        info = {}
        out = select(plain(*args), ob_class, caps, info=info, **kw)
        log.append(info)
        return out

    _letkf.taper = taper
    try:
        yield log
    finally:
        _letkf.taper = plain


def letkf_cycle(c, ob_class, caps, assim=None, **kw):
    """tests/_letkf.py's cycle of the seeded case c under the cap; the result gains reach / bites / gap of the grid (and of the
    obs as ob_reach / ob_bites / ob_gap)."""
    a = c["assim"] if assim is None else assim
    with capped(ob_class, caps, **kw) as log:
        ref = _letkf.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], a, c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                                 c["grid_lon"], c["n_lead"])
    ref.update(reach=log[0]["reach"], bites=log[0]["bites"], gap=log[0]["gap"], ob_reach=log[1]["reach"], ob_bites=log[1]["bites"],
               ob_gap=log[1]["gap"])
    return ref


# the cases of DESIGN.md 7y-8: (M, P, ny, nx, n_lead), caps, half-widths (None: the default), classes k % 3 or one class
CASES = [
    ((3, 5, 3, 5, 2), (2,), None),
    ((16, 64, 5, 7, 3), (8,), None),
    ((17, 33, 5, 7, 3), (1,), None),
    ((31, 64, 4, 5, 2), (16,), None),
    ((40, 400, 6, 7, 3), (50,), None),
    ((80, 700, 6, 7, 2), (100,), None),
    ((136, 300, 3, 6, 1), (64,), None),
    ((20, 120, 9, 11, 2), (12,), (300.0, 800.0)),
    ((16, 64, 5, 7, 3), (4, 0, 12), None),
    ((40, 400, 6, 7, 3), (10, 0, 40), None),
]


def make_case(shape, caps, hw):
    c = _letkf.make_case(*shape, seed=0, **({} if hw is None else dict(hw=hw)))
    ob_class = None if len(caps) == 1 else np.arange(c["P"], dtype=np.int32) % 3
    return c, ob_class
