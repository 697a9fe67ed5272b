"""The inputs of the BSDF tests (tests/test_bsdf_model.py on the CPU, tests/test_gpu_bsdf.py on the device): one material
table with every kind of row the renderer knows, and seeded sets of (row, wi, wo, u) aimed at the places where the BSDF
code branches or cancels.  Every set is a few thousand lanes; all directions and samples are float32, and they are what
they are -- nothing downstream normalises them."""
import functools

import numpy as np

import bsdf_model as BM

ALPHAS = (1e-3, 1e-2, 0.1, 0.5, 1.0)
ETAS = (1.49 / 1.000277, 1.0 / 1.5, 2.419, 1.0)      # int_ior / ext_ior: acrylic in air, from inside glass, diamond, no interface
CONDUCTORS = {  # eta, k, specular reflectance
    "veach-mis": ((0.200438, 0.924033, 1.10221), (3.91295, 2.45285, 2.14219), (0.3, 0.3, 0.3)),
    "Al": ((1.657460, 0.880369, 0.521229), (9.223869, 6.269523, 4.837001), (1.0, 1.0, 1.0)),
}
ONE_M = np.float32(1.0) - np.float32(2.0 ** -24)       # the largest float32 below 1
U_EDGES = np.array([0.0, 2.0 ** -24, 0.5, ONE_M], np.float32)


def _row(kind, refl=(1, 1, 1), alpha=0.0, eta=(0, 0, 0), k=(0, 0, 0), one_sided=False):
    r = np.zeros(BM.STRIDE, np.float32)
    r[0], r[1:4], r[4], r[5:8], r[8:11], r[11] = kind, refl, alpha, eta, k, 1.0 if one_sided else 0.0
    return r


@functools.lru_cache(maxsize=None)
def table():
    """-> rows (n_mat,16) float32, {group name: row numbers}"""
    rows, groups = [], {}

    def add(group, r):
        groups.setdefault(group, []).append(len(rows))
        rows.append(r)

    add("diffuse", _row(BM.DIFFUSE, (0.5, 0.6, 0.7)))
    add("diffuse", _row(BM.DIFFUSE, (0.8, 0.25, 0.1), one_sided=True))
    for name, (eta, k, spec) in CONDUCTORS.items():
        for sign in (1.0, -1.0):          # Beckmann, GGX
            for a in ALPHAS:
                add("rough_conductor", _row(BM.ROUGH_CONDUCTOR, spec, sign * a, eta, k))
        add("conductor", _row(BM.CONDUCTOR, spec, 0.0, eta, k))
    add("rough_conductor", _row(BM.ROUGH_CONDUCTOR, (1, 1, 1), 0.1, *CONDUCTORS["Al"][:2], one_sided=True))
    add("conductor", _row(BM.CONDUCTOR, (1, 1, 1), 0.0, *CONDUCTORS["Al"][:2], one_sided=True))
    for e in ETAS:
        for sign in (1.0, -1.0):
            for a in ALPHAS:
                add("rough_dielectric", _row(BM.ROUGH_DIELECTRIC, (1, 1, 1), sign * a, (e, 0, 0), one_sided=True))
        add("dielectric", _row(BM.DIELECTRIC, (1, 1, 1), 0.0, (e, 0, 0), one_sided=True))
    groups = {g: np.array(v, np.int32) for g, v in groups.items()}
    groups["all"] = np.arange(len(rows), dtype=np.int32)
    groups["glass"] = np.concatenate([groups["rough_dielectric"], groups["dielectric"]])
    groups["rough"] = np.concatenate([groups["rough_conductor"], groups["rough_dielectric"]])
    return np.stack(rows), groups


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _with_z(rng, z):
    """unit vectors of the given z, any azimuth"""
    phi = rng.uniform(0, 2 * np.pi, z.shape[0])
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], -1)


def _stratified(rng, n):
    """n points of the unit cube, every component stratified into n cells (a Latin hypercube), below 1 in float32"""
    u = np.stack([(rng.permutation(n) + rng.random(n)) / n for _ in range(3)], -1)
    return np.minimum(u.astype(np.float32), ONE_M)


def _pick(rng, group, n):
    return rng.choice(table()[1][group], n).astype(np.int32)


def _alpha_eta(idx):
    rows = table()[0].astype(np.float64)
    a = np.abs(rows[idx, 4])
    e = np.where(rows[idx, 5] > 0, rows[idx, 5], 1.0)
    return np.where(a > 0, a, 0.1), e


def _f32(idx, wi, wo, u):
    return idx, np.ascontiguousarray(wi, np.float32), np.ascontiguousarray(wo, np.float32), np.ascontiguousarray(u, np.float32)


def _refract(wi, eta):
    """the direction wi (unit, float64) continues in through a flat interface of index ratio eta = int / ext, Snell's law;
    the mirror direction where there is none"""
    ci = wi[:, 2]
    e = np.where(ci > 0, eta, 1.0 / eta)
    c2 = 1.0 - (1.0 - ci * ci) / (e * e)
    ct = np.sqrt(np.maximum(c2, 0.0))
    t = np.stack([-wi[:, 0] / e, -wi[:, 1] / e, -np.sign(ci) * ct], -1)
    return np.where((c2 > 0)[:, None], t, wi * np.array([-1.0, -1.0, 1.0]))


def set_uniform(n=8192, seed=11):
    rng = np.random.default_rng(seed)
    return _f32(_pick(rng, "all", n), _sphere(rng, n), _sphere(rng, n), _stratified(rng, n))


def set_grazing(n=4096, seed=12):
    """|wi.z| from 1e-6 to 1e-1, either side; wo uniform or, for half the lanes, near the mirror direction"""
    rng = np.random.default_rng(seed)
    z = 10.0 ** rng.uniform(-6, -1, n) * rng.choice([-1.0, 1.0], n)
    wi = _with_z(rng, z)
    idx = _pick(rng, "all", n)
    a, _ = _alpha_eta(idx)
    near = _unit(wi * np.array([-1.0, -1.0, 1.0]) + a[:, None] * rng.normal(size=(n, 3)) * 0.5)
    wo = np.where((rng.random(n) < 0.5)[:, None], _sphere(rng, n), near)
    return _f32(idx, wi, wo, _stratified(rng, n))


def set_axes(n=4096, seed=13):
    """wi exactly on the horizon (z = 0), exactly +z, exactly -z, and so close to +-z that sincos_phi's switch (sin^2 of the
    stretched wi against 4 * 2^-24) is within a percent either way: a quarter each"""
    rng = np.random.default_rng(seed)
    idx = _pick(rng, "all", n)
    a, _ = _alpha_eta(idx)
    wi = _with_z(rng, np.zeros(n)).astype(np.float32).astype(np.float64)
    wi[:, 2] = 0.0
    k = rng.integers(0, 4, n)
    wi[k == 1] = (0.0, 0.0, 1.0)
    wi[k == 2] = (0.0, 0.0, -1.0)
    # the stretched direction (a x, a y, z) / |.| has sin^2 = 4 * 2^-24 where tan(theta) = sqrt(4 * 2^-24) / a, about
    t = np.sqrt(4.0 * 2.0 ** -24) / a * 10.0 ** rng.uniform(-0.005, 0.005, n)
    near = _with_z(rng, rng.choice([-1.0, 1.0], n) / np.sqrt(1.0 + t * t))
    wi[k == 3] = near[k == 3]
    return _f32(idx, wi, _sphere(rng, n), _stratified(rng, n))


def set_mirror(n=8192, seed=14):
    """wo: the mirror direction of wi, perturbed by about alpha (where a rough lobe has its mass)"""
    rng = np.random.default_rng(seed)
    idx = _pick(rng, "rough", n)
    a, _ = _alpha_eta(idx)
    wi = _sphere(rng, n)
    wo = _unit(wi * np.array([-1.0, -1.0, 1.0]) + a[:, None] * rng.normal(size=(n, 3)) * rng.choice([0.3, 1.0, 2.0], n)[:, None])
    return _f32(idx, wi, wo, _stratified(rng, n))


def set_horizon_wo(n=4096, seed=15):
    """wo exactly on the horizon, and within a few float32 steps of it on either side"""
    rng = np.random.default_rng(seed)
    z = rng.choice(np.array([0.0, 2.0 ** -24, -2.0 ** -24, 1e-6, -1e-6]), n)
    # (a few at float32's smallest number: cos_i * cos_o underflows there, and which lobe wo belongs to is anybody's guess)
    z = np.where(rng.random(n) < 0.01, rng.choice(np.array([1e-45, -1e-45]), n), z)
    wo = _with_z(rng, np.zeros(n))
    wo[:, 2] = z
    return _f32(_pick(rng, "all", n), _sphere(rng, n), wo, _stratified(rng, n))


def set_equal(n=2048, seed=16):
    """wo = wi (retro-reflection: the half vector is wi itself), and wo = -wi (straight through)"""
    rng = np.random.default_rng(seed)
    wi = _sphere(rng, n)
    wo = np.where((rng.random(n) < 0.75)[:, None], wi, -wi)
    return _f32(_pick(rng, "all", n), wi, wo, _stratified(rng, n))


def set_refracted(n=8192, seed=17):
    """rough glass, wo across the interface: at the refracted direction exactly (as float32 allows) and around it by about alpha"""
    rng = np.random.default_rng(seed)
    idx = _pick(rng, "rough_dielectric", n)
    a, e = _alpha_eta(idx)
    wi = _sphere(rng, n)
    wo = _unit(_refract(wi, e) + a[:, None] * rng.normal(size=(n, 3)) * rng.choice([0.0, 0.3, 1.0], n)[:, None])
    return _f32(idx, wi, wo, _stratified(rng, n))


def set_critical(n=4096, seed=18):
    """glass seen from its dense side at the critical angle +- 1e-7 .. 1e-1 radians; wo at the mirror direction or the
    refracted one, perturbed by about alpha"""
    rng = np.random.default_rng(seed)
    idx = _pick(rng, "glass", n)
    a, e = _alpha_eta(idx)
    idx, a, e = idx[e != 1.0], a[e != 1.0], e[e != 1.0]
    n = idx.shape[0]
    dense_below = e > 1.0                       # the dense medium is inside: wi comes from below
    s = np.where(dense_below, 1.0 / e, e)       # sin of the critical angle
    theta = np.arcsin(s) + 10.0 ** rng.uniform(-7, -1, n) * rng.choice([-1.0, 1.0], n)
    wi = _with_z(rng, np.cos(theta) * np.where(dense_below, -1.0, 1.0))
    base = np.where((rng.random(n) < 0.5)[:, None], wi * np.array([-1.0, -1.0, 1.0]), _refract(wi, e))
    rough = table()[0][idx, 0] == BM.ROUGH_DIELECTRIC
    wo = _unit(base + np.where(rough, a, 0.0)[:, None] * rng.normal(size=(n, 3)) * 0.5)
    return _f32(idx, wi, wo, _stratified(rng, n))


def set_u_edges(seed=19):
    """every component of u at 0, 2^-24, 0.5 and the largest float32 below 1, for every row: all 64 combinations at six
    directions of wi from steep to moderate, above and below; at the grazing one (cos 0.02, where a normal on the horizon
    sends the reflection through the surface) the 32 with the lobe sample at 0 or 0.5 -- the grazing set is the place for
    that direction, and here it would take the set's ambiguous share past the cap by itself"""
    rng = np.random.default_rng(seed)
    rows = table()[0]
    combos = np.stack(np.meshgrid(U_EDGES, U_EDGES, U_EDGES, indexing="ij"), -1).reshape(-1, 3)
    few = combos[(combos[:, 0] == 0.0) | (combos[:, 0] == 0.5)]
    per_row = [(z, few if z == 0.02 else combos) for z in (0.999, 0.8, 0.6, 0.3, 0.02, -0.6, -0.9)]
    z = np.concatenate([np.full(c.shape[0], z) for z, c in per_row])
    u = np.concatenate([c for _, c in per_row])
    idx = np.repeat(np.arange(rows.shape[0], dtype=np.int32), z.size)
    n = idx.shape[0]
    return _f32(idx, _with_z(rng, np.tile(z, rows.shape[0])), _sphere(rng, n), np.tile(u, (rows.shape[0], 1)))


SETS = {
    "uniform": set_uniform, "grazing": set_grazing, "axes": set_axes, "mirror": set_mirror, "horizon_wo": set_horizon_wo,
    "equal": set_equal, "refracted": set_refracted, "critical": set_critical, "u_edges": set_u_edges,
}
# The two sets aimed at a branch on purpose, and the cap on the ambiguous share of each: its measured share on the oracle
# (profiles/bsdf/band.txt), rounded up to the next whole per cent.  Every other set is held to bsdf_model.AMBIGUOUS_CAP.
NARROW = {"grazing": 0.08, "critical": 0.06}


@functools.lru_cache(maxsize=None)
def get(name):
    s = SETS[name]()
    assert s[0].shape[0] <= 1 << 16
    for a in s:
        a.setflags(write=False)
    return s
