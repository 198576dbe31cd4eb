"""ensemble_gram / ensemble_eofs / ensemble_clusters end to end on the MI355X: planted modes and planted groups
of members, against the longdouble model tests/_gram.py and against ensemble_sensitivity on the same state."""
import warnings

import numpy as np
import pytest

import _gram as gm

pytestmark = pytest.mark.gpu

U = gm.U
NVAR, NT, NY, NX, M = 2, 2, 6, 8, 20
NOISE = 1e-6


def _grid():
    return np.meshgrid(np.linspace(30, 40, NY), np.linspace(250, 260, NX), indexing="ij")


def _orthonormal(rng, rows, cols, against=None):
    """`cols` orthonormal columns of length `rows`, orthogonal to the columns of `against`"""
    A = rng.standard_normal((rows, cols))
    if against is not None:
        A = np.concatenate([against, A], axis=1)
    Q = np.linalg.qr(A)[0]
    return Q[:, -cols:]


def _planted(dtype=np.float64, seed=3):
    """Three orthogonal spatial patterns times standardised PCs, amplitudes 4 : 2 : 1, plus 1e-6 noise and a member-independent
    mean field.  Returns (state, pcs (3, M), patterns (3, N), the members (N, M))."""
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(seed)
    N = NVAR * NT * NY * NX
    E = _orthonormal(rng, N, 3)                                        # unit-length spatial patterns
    V = _orthonormal(rng, M, 3, against=np.ones((M, 1)))              # unit length, mean 0, mutually orthogonal
    pcs = np.sqrt(M - 1.0) * V.T                                      # unit sample variance
    for k in range(3):
        if pcs[k][int(np.argmax(np.abs(pcs[k])))] < 0.0:
            pcs[k] = -pcs[k]
    amp = np.array([4.0, 2.0, 1.0]) * np.sqrt(N)
    X = 5.0 * rng.standard_normal((N, 1)) + (E * amp) @ pcs + NOISE * rng.standard_normal((N, M))
    lat, lon = _grid()
    state = EnsembleState.from_array(X.reshape(NVAR, NT, NY, NX, M), lat, lon, varnames=["t2m", "psfc"], dtype=dtype)
    return state, pcs, (E * amp).T, X


def test_eofs_of_a_planted_state():
    from efa_xray_amd import ensemble_eofs, ensemble_gram, ensemble_sensitivity, observation_targets
    state, pcs, pats, _ = _planted()
    N = state.nstate()
    out = ensemble_eofs(state, 3)       # (the noise's own modes lie below the null threshold 64 M u trace)
    X = np.ascontiguousarray(state.to_vect())
    m = gm.model(X, NVAR * NT, np.ones(NVAR * NT))
    G = out["gram"]
    assert out["n"] == N and out["n_bad"] == 0 and out["weight_sum"] == float(N) and np.all(out["scales"] == 1.0)
    assert np.array_equal(gm.bits(G), gm.bits(np.ascontiguousarray(G.T))) and gm.ratio(G, m) <= 1.0
    assert np.array_equal(gm.bits(ensemble_gram(state)["gram"]), gm.bits(G))
    lam, ex, pc = out["variance"], out["explained"], out["pcs"]
    assert lam.shape == (3,) and pc.shape == (3, M) and np.all(np.diff(lam) <= 0.0) and np.all(lam >= 0.0)
    assert ex[:3].sum() > 0.999 and np.all(np.abs(lam[:3] / (np.array([16.0, 4.0, 1.0]) * N) - 1.0) < 1e-5)
    # the planted PCs, up to the documented sign; the noise rotates a mode by about NOISE / (gap of the amplitudes)
    assert np.max(np.abs(pc[:3] - pcs)) <= 100 * NOISE
    assert np.max(np.abs(pc @ pc.T / (M - 1.0) - np.eye(3))) <= 1e-12
    assert np.max(np.abs(pc.mean(axis=1))) <= 1e-12
    for k in range(3):
        assert pc[k][int(np.argmax(np.abs(pc[k])))] > 0.0
        v = pc[k] / np.sqrt(M - 1.0)
        assert np.max(np.abs(G @ v - lam[k] * v)) <= 64 * M * U * np.trace(G), k
    # the patterns are ensemble_sensitivity's cov of the PCs, bit for bit, and the planted ones
    sens = ensemble_sensitivity(state, pc)
    assert out["patterns"].shape == (3, NVAR, NT, NY, NX)
    assert np.array_equal(gm.bits(out["patterns"]), gm.bits(sens["cov"]))
    assert np.max(np.abs(out["patterns"][:3].reshape(3, N) - pats)) <= 1e-3 * np.max(np.abs(pats))
    # sqrt(c_i) patterns_ik = sqrt(lambda_k) e_ik with e_k of unit length (c = 1 here)
    for k in range(3):
        e = out["patterns"][k].reshape(-1) / np.sqrt(lam[k])
        assert abs(e @ e - 1.0) <= 1e-11, k
    none = ensemble_eofs(state, 2, patterns=False)
    assert "patterns" not in none and np.array_equal(gm.bits(none["pcs"]), gm.bits(pc[:2]))
    # the leading PC is a forecast metric as it is
    tg = observation_targets(state, pc[:1], 2, {"t2m": 1.0, "psfc": 1.0})
    assert len(tg["targets"]) == 2 and tg["metric_var"].shape == (3, 1) and abs(tg["metric_var"][0, 0] - 1.0) <= 1e-12


def test_eofs_in_a_weighted_norm_obey_the_identity():
    from efa_xray_amd import ensemble_eofs
    state, _, _, _ = _planted()
    lat, _ = _grid()
    w = np.cos(np.radians(lat))
    norm = {"t2m": [1.0, 0.5], "psfc": 2.0}
    out = ensemble_eofs(state, 3, norm=norm, weights=w)
    assert np.array_equal(out["scales"], [[1.0, 0.5], [2.0, 2.0]]) and abs(out["weight_sum"] - 4 * w.sum()) <= 1e-12 * 4 * w.sum()
    X = np.ascontiguousarray(state.to_vect())
    m = gm.model(X, NVAR * NT, out["scales"].reshape(-1), w.reshape(-1))
    assert gm.ratio(out["gram"], m) <= 1.0
    c = np.repeat(out["scales"].reshape(-1) ** 2, NY * NX) * np.tile(w.reshape(-1), NVAR * NT)
    for k in range(3):
        e = np.sqrt(c) * out["patterns"][k].reshape(-1) / np.sqrt(out["variance"][k])
        assert abs(e @ e - 1.0) <= 1e-11, k


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_std_norm_makes_units_irrelevant(dtype):
    from efa_xray_amd import EnsembleState, ensemble_eofs, ensemble_gram
    state, _, _, X = _planted(dtype)
    lat, lon = _grid()
    f = 1024.0 if dtype == np.float32 else 1000.0             # (a power of two keeps the float32 members exact)
    arr = X.reshape(NVAR, NT, NY, NX, M)
    big = arr.copy()
    big[1] *= f
    st_big = EnsembleState.from_array(big, lat, lon, varnames=["t2m", "psfc"], dtype=dtype)
    a = ensemble_eofs(state, 3, norm="std", patterns=False)
    b = ensemble_eofs(st_big, 3, norm="std", patterns=False)
    assert np.allclose(b["scales"][1] * f, a["scales"][1], rtol=1e-12) and np.allclose(b["scales"][0], a["scales"][0], rtol=1e-14)
    assert np.allclose(a["gram"], b["gram"], rtol=0.0, atol=1e-11 * np.trace(a["gram"]))
    assert np.max(np.abs(a["pcs"] - b["pcs"])) <= 1e-9
    # every variable then carries the same share: trace(G) = sum_i c_i var_i = the number of elements
    assert abs(np.trace(a["gram"]) - state.nstate()) <= 1e-12 * state.nstate()
    # a constant variable: scale 0 and a warning
    flat = arr.copy()
    flat[1] = 7.0
    st_flat = EnsembleState.from_array(flat, lat, lon, varnames=["t2m", "psfc"], dtype=dtype)
    with pytest.warns(RuntimeWarning, match="scale 0"):
        c = ensemble_gram(st_flat, norm="std")
    assert np.all(c["scales"][1] == 0.0) and np.all(c["scales"][0] > 0.0) and c["n"] == NT * NY * NX
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ensemble_gram(state, norm="std")


def _grouped(dtype, seed=5):
    """Members in three groups of 7, 8 and 5 at centres 10 sigma apart; members 0, 7 and 15 sit exactly at their centres."""
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(seed)
    N = NVAR * NT * NY * NX
    sizes = (7, 8, 5)
    group = np.repeat(np.arange(3), sizes)
    centres = np.round(10.0 * rng.standard_normal((N, 3)) * 64) / 64       # exact in float32
    dev = np.round(rng.standard_normal((N, M)) * 64) / 64
    dev[:, [0, 7, 15]] = 0.0
    X = centres[:, group] + dev
    perm = rng.permutation(M)                                             # the groups are not contiguous
    lat, lon = _grid()
    state = EnsembleState.from_array(X[:, perm].reshape(NVAR, NT, NY, NX, M), lat, lon, varnames=["t2m", "psfc"], dtype=dtype)
    return state, group[perm], [int(np.nonzero(perm == c)[0][0]) for c in (0, 7, 15)]


def test_clusters_of_planted_groups():
    from efa_xray_amd import clusters_from_gram, distances_from_gram, ensemble_clusters
    results = {}
    for dtype in (np.float64, np.float32):
        state, group, centres = _grouped(dtype)
        out = ensemble_clusters(state, 3)
        # the labels, numbered in the order of the lowest members
        order = sorted(range(3), key=lambda c: int(np.nonzero(group == c)[0][0]))
        want = np.empty(M, dtype=np.int64)
        for lab, c in enumerate(order):
            want[group == c] = lab
        assert np.array_equal(out["labels"], want)
        assert list(out["sizes"]) == [int(np.sum(group == c)) for c in order]
        assert list(out["medoids"]) == [centres[c] for c in order]
        # against the distances of the longdouble model
        X = np.ascontiguousarray(state.to_vect())
        m = gm.model(X, NVAR * NT, np.ones(NVAR * NT))
        assert gm.ratio(out["gram"], m) <= 1.0
        ref = clusters_from_gram(m["G"].astype(np.float64), 3)
        for key in ("labels", "sizes", "medoids"):
            assert np.array_equal(out[key], ref[key]), key
        d2 = distances_from_gram(m["G"].astype(np.float64))
        direct = ((X[:, :, None].astype(np.float64) - X[:, None, :].astype(np.float64)) ** 2).sum(axis=0)
        assert np.allclose(d2, direct, rtol=1e-10) and np.allclose(distances_from_gram(out["gram"]), direct, rtol=1e-10)
        assert np.allclose(out["within"], [direct[md, out["labels"] == k].sum() for k, md in enumerate(out["medoids"])], rtol=1e-10)
        results[dtype] = out
    assert np.array_equal(results[np.float64]["labels"], results[np.float32]["labels"])
    assert np.array_equal(results[np.float64]["medoids"], results[np.float32]["medoids"])
