"""Emitter sampling pinned to its specification: the CPU oracle's emitter sample without its visibility test
(pgo_emitter_probe: sample_emitter_ray of oracle/pg_oracle_render.c, which the render pass wraps its shadow ray around) against
tests/emitter_model.py, a float64 model with a derived float32 error band.  The device is compared with the oracle bit for
bit elsewhere (tests/test_gpu_emitter.py), so what holds here holds for it.

The broad sets take p and the geometric normal from the hits of test_surface_model.hits(name) (every fourth normal flipped)
and a uniform e.  A lane whose p lies ON the emitter it samples (the hit was on that very shape) has no decided answer even
in exact arithmetic -- cos = 0 on a quad's own plane, a gap of 0 from a sphere -- so such lanes must pass like any other but
are counted apart: the cap of 2 % is on all the others.  Measured (profiles/emitter/band.txt): worst |difference| / bracket per
quantity 0.003-0.75 (C is four times that), and no lane under the cap ambiguous on any broad set.  The composition with the
visibility test -- em_weight where the shadow ray is free -- is what the oracle's render pass now does with the same two
functions, so the unchanged render goldens and parity tests hold it to what the unsplit sample_emitter returned.
tools/emitter_mutants.py shows the tests fail for fourteen deliberate errors (profiles/emitter/mutations.txt)."""
import functools

import numpy as np
import pytest

import emitter_model as EM
import raycast_model as RM
import surface_model as SM
import test_raycast_model as TM
import test_surface_model as TS
from oracle import pg_oracle as po

SCENES = TS.SCENES
N_BROAD = TS.N_BROAD
F32 = np.float32


def scene(name):
    return TS.scene(name)


@functools.lru_cache(maxsize=None)
def tables(name):
    return EM.Tables(scene(name))


@functools.lru_cache(maxsize=None)
def broad(name):
    """the broad set of a scene: made once, shared, never changed"""
    h = TS.hits(name)
    s = TS.probe_oracle(name, h)
    n = s["ng"].copy()
    n[::4] = -n[::4]
    e = np.random.default_rng(41 + SCENES.index(name)).random((N_BROAD, 2)).astype(F32)
    return dict(p=s["p"].copy(), n=n, e=e, prim=h["prim"].astype(np.int64))


def probe_oracle(sc, L):
    return po.emitter_probe(sc, L["p"], L["n"], L["e"])


def check(T, L, out, what, cap=True, C=None):
    """every lane equal to the model under one assignment of its doubtful decisions; -> (ambiguous share under the cap, ratios, verdict)"""
    bad, ratio, amb, v = EM.judge(T, L["p"], L["n"], L["e"], out, C)
    own = np.zeros(amb.shape[0], bool) if v is None or "prim" not in L else (v.prim == L["prim"])
    share = float(amb[~own].mean()) if (~own).any() else 0.0
    print("%s: %d lanes, %.3f %% of them ambiguous; %d on the emitter they sample (%.1f %% of those ambiguous), %.3f %% of the others ambiguous (the capped share); worst |difference| / bracket: %s" % (
        what, amb.shape[0], 100.0 * amb.mean(), own.sum(), 100.0 * amb[own].mean() if own.any() else 0.0, 100.0 * share,
        ", ".join("%s %.2f" % (k, r.max()) for k, r in sorted(ratio.items()))))
    for k, idx in bad.items():
        i = idx[0]
        assert idx.size == 0, "%s: %s fails on lanes %s, e.g. p=%s n=%s e=%s -> %s" % (
            what, k, idx[:8], L["p"][i], L["n"][i], L["e"][i], {c: out[c][i] for c in out})
    if cap:
        assert share <= EM.AMBIGUOUS_CAP
    return share, ratio, v


@pytest.mark.parametrize("name", SCENES)
def test_oracle_against_the_model(name):
    L, T = broad(name), tables(name)
    out = probe_oracle(scene(name), L)
    share, ratio, v = check(T, L, out, name + " broad")
    kinds = np.bincount(v.kind, minlength=3)
    want = {"veach-ajar": (1, 0, 0), "torus": (0, 0, 1), "mixed": (1, 1, 1), "cornell-box": (1, 0, 0), "veach-mis": (0, 1, 0)}[name]
    assert ((kinds >= 256) >= np.array(want, bool)).all(), kinds
    if name == "torus":          # (whose only light is directional: every lane has a sample)
        assert kinds[2] >= 64 and (out["ds_delta"] == 1).all() and (out["need_shadow"] == 1).all()
    else:
        assert (out["ds_pdf"] == 0).sum() >= 64


@pytest.mark.parametrize("name", SCENES)
def test_mis_consistency(name):
    """the density a sample was drawn with is the density emitter_hit_pdf reports for a hit at the sampled point"""
    L, T = broad(name), tables(name)
    out = probe_oracle(scene(name), L)
    fails, judged, between = EM.consistency(T, L["p"], L["e"], out)
    print("%s: %d lanes judged, %d between the inside cut and the cap limit (not judged)" % (name, judged.sum(), between.sum()))
    assert fails.size == 0, (fails[:8], {c: out[c][fails[0]] for c in out})
    assert name == "torus" or judged.sum() >= 2048


@pytest.mark.parametrize("name", SCENES)
def test_shadow_rays(name):
    """no sample is occluded by its own emitter, and a blocker that surely lies strictly between occludes it; the ray-casting
    model (tests/raycast_model.py) says which rays are ambiguous"""
    L, T = broad(name), tables(name)
    sc = scene(name)
    out = probe_oracle(sc, L)
    y = out["need_shadow"] != 0
    assert y.sum() >= 1024
    idx = EM.choice(T, L["e"][:, 0])[0]
    sampled = T.emitters[idx]
    t, prim, _, _, _ = po.intersect(sc, out["sh_o"][y], out["sh_d"][y], out["sh_tmax"][y])
    m = RM.cast(TM.tables(name), out["sh_o"][y], out["sh_d"][y])
    own = (prim == sampled[y]) & (prim >= 0)
    # (a ray that leaves a point of the emitter itself grazes it: the model calls those ambiguous)
    assert not (own & ~m.ambiguous).any(), np.nonzero(y)[0][own & ~m.ambiguous][:8]
    tmax = out["sh_tmax"][y].astype(np.float64)
    blocked = np.isfinite(m.t_sure) & (m.t_hi < tmax) & ~m.ambiguous
    print("%s: %d shadow rays, %d hit their own emitter (all ambiguous to the model), %d surely blocked, %d occluded" % (
        name, y.sum(), own.sum(), blocked.sum(), (prim >= 0).sum()))
    assert (prim[blocked] >= 0).all(), np.nonzero(y)[0][blocked & (prim < 0)][:8]
    free = ~np.isfinite(m.t_poss) | ((m.t_lo > tmax) & ~m.ambiguous)
    assert (prim[free] < 0).all(), np.nonzero(y)[0][free & (prim >= 0)][:8]
    assert name == "torus" or blocked.sum() >= 32


# ---- known answers on hand-built scenes ----

MATS = lambda S: [S.diffuse_material((0.5, 0.5, 0.5)), S.diffuse_material((0.0, 0.0, 0.0))]


def _quad_light(S, at, size=0.5, radiance=(3.0, 2.0, 1.0)):
    """a square light of side 2 size in the plane z = at[2], facing +z"""
    q = S.rectangle(np.array([[size, 0, 0, at[0]], [0, size, 0, at[1]], [0, 0, 1.0, at[2]], [0, 0, 0, 1]]), (0.0, 0.0, 0.0), radiance)
    for r in q:
        r[22] = 1
    return q


def _floor(S):
    q = S.rectangle(np.array([[20.0, 0, 0, 0], [0, 20.0, 0, 0], [0, 0, 1.0, -5.0], [0, 0, 0, 1]]), (0.5, 0.5, 0.5))
    for r in q:
        r[22] = 0
    return q


@functools.lru_cache(maxsize=None)
def list_scene(count):
    """emitter lists of 1, 2, 3 and 7 entries of mixed kinds (quads, then spheres, then directional lights, with shapes that
    do not emit between them, so that the list order is not the shape order)"""
    from practical_path_guiding_lab_amd import scene as S
    n_q, n_s, n_d = {1: (1, 0, 0), 2: (1, 1, 0), 3: (1, 1, 1), 7: (3, 2, 2)}[count]
    quads, spheres = _floor(S), [S.sphere((-6.0, 1.0, 2.0), 0.75, 0)]
    for k in range(n_q):
        quads = quads + _quad_light(S, (4.0 * k, 3.0, 6.0 + k), 0.5 + 0.25 * k, (3.0 + k, 2.0, 1.0)) + (_floor(S) if k == 0 else [])
    for k in range(n_s):
        spheres += [S.sphere((1.0 + 5.0 * k, 2.0, 3.0), 2.0 - 1.5 * k, 1, (5.0, 6.0 + k, 7.0)), S.sphere((-9.0, 1.0 + k, 2.0), 0.5, 0)]
    lights = [S.directional_light((0.2 * k, -0.3, -1.0), (1.5, 2.5 + k, 3.5)) for k in range(n_d)]
    return TS._finish(quads, spheres, MATS(S), None, None, None) if not lights else _with_lights(S, quads, spheres, lights)


def _with_lights(S, quads, spheres, lights):
    cam = S.make_camera(np.array([[1.0, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 20], [0, 0, 0, 1]]), 40.0, 8, 8)
    return S._finish(list(quads), cam, 4, 8, ["q"] * len(quads), spheres, MATS(S), None, None, lights, None)


def lanes(p, n, e):
    p, n, e = (np.asarray(a, np.float64).reshape(-1, k) for a, k in ((p, 3), (n, 3), (e, 2)))
    m = max(p.shape[0], n.shape[0], e.shape[0])
    full = lambda a: np.tile(a, (m // a.shape[0], 1)).astype(F32)
    return dict(p=full(p), n=full(n), e=full(e))


def choice_samples(count):
    """e1 at 0, 1, 1 - 2^-24 and k / count with its two float neighbours; e2 at 0, 1, 2^-24 and 1/2"""
    e1 = [0.0, 1.0, 1 - 2.0 ** -24]
    for k in range(1, count):
        x = F32(k / count)
        e1 += [float(x), float(np.nextafter(x, F32(0))), float(np.nextafter(x, F32(1)))]
    return np.array([(a, b) for a in e1 for b in (0.0, 1.0, 2.0 ** -24, 0.5)], F32)


@pytest.mark.parametrize("count", [1, 2, 3, 7])
def test_choice_of_emitter(count):
    sc = list_scene(count)
    T = EM.Tables(sc)
    assert T.count == count
    e = choice_samples(count)
    L = lanes((0.3, 0.2, 0.0), (0.0, 0.0, 1.0), e)
    out = probe_oracle(sc, L)
    _, _, v = check(T, L, out, "list of %d" % count, cap=False)
    # the list order: quads, spheres, directional lights -- read off the lanes' own outputs
    n_q, n_s = int((T.emitters >= 0).sum() - (T.emitters >= T.first_sphere).sum()), int((T.emitters >= T.first_sphere).sum())
    x = e[:, 0].astype(np.float64) * count
    sure = np.abs(x - np.rint(x)) > 1e-6
    idx = np.minimum(np.floor(x), count - 1).astype(int)
    assert (out["ds_delta"][sure] == (idx[sure] >= n_q + n_s)).all()
    radiance = {tuple(T.quads[q, 19:22]): k for k, q in enumerate(T.emitters[:n_q])}
    for i in np.nonzero(sure & (idx < n_q) & (out["ds_pdf"] > 0))[0]:   # (a quad's weight names it: its radiance is its own)
        got = out["em_weight"][i].astype(np.float64) * out["ds_pdf"][i]
        assert min(radiance, key=lambda r: np.abs(np.array(r) - got).sum()) == tuple(T.quads[T.emitters[idx[i]], 19:22]), (i, got)
    # e1 = 1 takes the last entry, with the reused sample 1; e1 = 0 the first, with 0
    last, first = e[:, 0] == 1.0, e[:, 0] == 0.0
    assert (v.prim[last] == T.emitters[-1]).all() and (v.prim[first] == T.emitters[0]).all()


@functools.lru_cache(maxsize=None)
def quad_scene():
    """one unit-area light, centre (10, 0, 0), facing +z"""
    from practical_path_guiding_lab_amd import scene as S
    return TS._finish(_floor(S) + _quad_light(S, (10.0, 0.0, 0.0)), None, MATS(S), None, None, None)


def quad_cases():
    """the light's centre (e = (1/2, 1/2)) from points at distance 2 whose direction makes cos = -1e-7, +1e-7 and exactly 0 with
    the normal, from below, from overhead, and from the light point itself"""
    c = np.array([10.0, 0, 0])
    p = [c + (2, 0, 2e-7), c + (2, 0, -2e-7), c + (2, 0, 0), c + (0, 0, -2), c + (0, 0, 2), c]
    return lanes(p, (0.0, 0.0, 1.0), (0.5, 0.5))


def test_quad_light_at_grazing_incidence():
    sc, L = quad_scene(), quad_cases()
    out = probe_oracle(sc, L)
    check(EM.Tables(sc), L, out, "quad", cap=False)
    pdf = out["ds_pdf"].astype(np.float64)
    assert pdf[1] == 0 and pdf[2] == 0 and pdf[3] == 0 and pdf[5] == 0           # from behind, edge-on, from below, dist = 0
    assert (out["need_shadow"] == [1, 0, 0, 0, 1, 0]).all()
    assert pdf[4] == 4.0 and (out["em_weight"][4] == np.array([3, 2, 1], F32) / F32(4)).all()   # overhead: d^2 / (cos A) = 4
    assert abs(pdf[0] - 4.0 / 1e-7) <= 1e-5 * pdf[0]
    assert (out["ds_d"][4] == (0, 0, -1)).all() and (out["sh_d"][4] == (0, 0, -1)).all()
    mag = F32(1 + 10) * F32(1e-4)
    assert out["sh_o"][4][2] == F32(2) - mag                                     # towards the light: n = +z, the light below
    assert abs(out["sh_tmax"][4] - (2 - float(mag)) * (1 - 1e-3)) < 1e-6
    assert np.isnan(out["ds_d"][5]).all()


@functools.lru_cache(maxsize=None)
def sphere_scene(r=2.0):
    from practical_path_guiding_lab_amd import scene as S
    return TS._finish(_floor(S), [S.sphere((0.0, 0.0, 0.0), r, 1, (5.0, 6.0, 7.0))], MATS(S), None, None, None)


def sphere_distances(r=2.0):
    adj = F32(r) * (F32(1) - F32(EM.K_SPHERE))
    below_switch, above_switch = r / np.sqrt(EM.SWITCH) * 1.01, r / np.sqrt(EM.SWITCH) * 0.99
    return [r * (1 + 2.0 ** -20), r, float(adj), float(np.nextafter(adj, F32(0))), float(np.nextafter(adj, F32(9))), r / 2,
            above_switch, below_switch, 1e3 * r, 4.0 * r]


def sphere_cases(r=2.0):
    """the sphere light (at the origin: |c - p| is then p's own z, to the float) from straight above at the distances of
    sphere_distances, with e1 at 0 (the cap's centre, where sin_alpha cancels), 1 (the tangent ring, where the facing cosine
    crosses zero), 2^-24, 1 - 2^-24 and 1/2"""
    c = np.zeros(3)
    e = [(a, b) for a in (0.0, 1.0, 2.0 ** -24, 1 - 2.0 ** -24, 0.5) for b in (0.0, 1.0, 2.0 ** -24, 0.3)]
    p = [c + (0, 0, d) for d in sphere_distances(r) for _ in e]
    return lanes(p, (0.0, 0.0, -1.0), e * len(sphere_distances(r)))


@pytest.mark.parametrize("r", [2.0, 0.03])
def test_sphere_light_from_every_distance(r):
    sc, L = sphere_scene(r), sphere_cases(r)
    out = probe_oracle(sc, L)
    check(EM.Tables(sc), L, out, "sphere r = %g" % r, cap=False)
    per = L["p"].shape[0] // len(sphere_distances(r))
    block = lambda k: slice(k * per, (k + 1) * per)
    assert (out["ds_pdf"][block(5)] == 0).all() and (out["ds_d"][block(5)] == 0).all()      # inside: nothing at all
    assert (out["ds_pdf"][block(3)] == 0).all() and (out["ds_pdf"][block(2)] == 0).all()    # on the cut and a float below it
    assert (out["ds_d"][block(3)] == 0).all() and (out["ds_d"][block(2)] == 0).all()
    # a float above the cut the sampler runs (ds_d is set) -- and, p being INSIDE the sphere by r kSphereEps, sin_max > 1, cos_max = 0
    # and every point it makes faces away: no sample, as from r itself (test_between_the_inside_cut_and_the_cap_limit has the rest)
    assert ((out["ds_d"][block(4)] != 0).any(axis=1) | np.isnan(out["ds_d"][block(4)]).any(axis=1)).all()
    assert (out["ds_pdf"][block(4)] == 0).all() and (out["ds_pdf"][block(1)] == 0).all()
    assert (out["need_shadow"][block(4)] == 0).all() and (out["need_shadow"][block(1)] == 0).all()
    want = 1 / (2 * np.pi * (1 - np.sqrt(1 - 1 / 16.0)))
    pdf = out["ds_pdf"][block(9)].astype(np.float64)
    assert (pdf[pdf > 0] == pdf[pdf > 0][0]).all() and abs(pdf[pdf > 0][0] - want) <= 1e-5 * want   # from 4 r: sin = 1/4
    far = out["ds_pdf"][block(8)].astype(np.float64)                                      # from 1e3 r float32's formula is 7.5 % off at most
    assert (np.abs(far[far > 0] * (2 * np.pi * (1 - np.sqrt(1 - 1e-6))) - 1) <= 0.075).all() and (far > 0).sum() >= per // 2
    centre = (L["e"][:, 0] == 0) & (out["ds_pdf"] > 0)
    axis = np.array([0, 0, -1.0])
    assert (np.abs(out["ds_d"][centre] - axis).max(axis=1) <= 5e-4).all()                   # e1 = 0: the axis, to sin_alpha's half mantissa


def gap_cases(r):
    """reference points straight above the sphere light at one float above the inside cut, at r, and one float above r -- the
    last is where sin alpha = r / |c - p| reaches emitter_hit_pdf's cap limit 0.99999994 for r = 0.03 and not for r = 2"""
    adj = F32(r) * (F32(1) - F32(EM.K_SPHERE))
    z = [float(np.nextafter(adj, F32(9))), float(F32(r)), float(np.nextafter(F32(r), F32(9)))]
    e = [(0.5, 0.3), (0.0, 0.0), (0.25, 0.75), (1.0, 0.5)]
    return z, lanes([(0.0, 0.0, d) for d in z for _ in e], (0.0, 0.0, -1.0), e * len(z))


# what the two sides give one float above r (float32, as recorded from the oracle): the sampler's cone density, and the hit
# pdf for a hit of the sphere's top seen from there -- for r = 0.03 its area form d^2 / (|cos| 4 pi r^2) with d = one float of r
GAP_ANSWERS = {2.0: (0.15923269093036652, 0.15923269093036652), 0.03: (0.15920990705490112, 3.0676645496596213e-16)}


@pytest.mark.parametrize("r", [2.0, 0.03])
def test_between_the_inside_cut_and_the_cap_limit(r):
    """Known answers where the sampler's cone and emitter_hit_pdf's area form could meet.  From the inside cut up to r itself both
    give NOTHING: the sampler makes no sample (sin_max >= 1: every point faces away), and the hit pdf is 0 for every hit of the
    sphere, because seen from on or inside it every point of it faces away.  One float above r the sampler has the cone's
    density; the hit pdf has the cone's too for r = 2 (sin alpha = 0.99999988: below the cap limit) and the area form's
    3.07e-16 for r = 0.03 (sin alpha rounds to the cap limit): there the two reference formulas disagree, by fifteen orders of
    magnitude, and both numbers are pinned as they are -- not to each other."""
    sc = sphere_scene(r)
    z, L = gap_cases(r)
    out = probe_oracle(sc, L)
    check(EM.Tables(sc), L, out, "gap r = %g" % r, cap=False)
    pdf = out["ds_pdf"].reshape(3, 4).astype(np.float64)
    assert (pdf[0] == 0).all() and (pdf[1] == 0).all() and (out["need_shadow"].reshape(3, 4)[:2] == 0).all()
    sampler, hit_top = GAP_ANSWERS[r]
    assert (np.abs(pdf[2, :3] - sampler) <= 1e-6 * sampler).all(), pdf[2]          # (the fourth lane is the tangent ring)
    assert pdf[2, 3] == 0 or abs(pdf[2, 3] - sampler) <= 1e-6 * sampler
    # hits of the top (from above), the side and the bottom (from inside) of the sphere, seen from the three reference points
    nq = sc.quads.shape[0]
    rays = ((0, 0, 3 * r), (0, 0, -1), 2 * r), ((3 * r, 0, 0), (-1, 0, 0), 2 * r), ((0, 0, 0), (0, 0, -1), r)
    ref = np.array([(0.0, 0.0, d) for d in z], F32)
    got = np.array([po.surface_probe(sc, np.full(3, nq, np.int32), np.tile(F32(o), (3, 1)), np.tile(F32(d), (3, 1)), np.full(3, t, F32), ref)["emitter_pdf"]
                    for o, d, t in rays], np.float64)                              # (hit, reference point)
    print("r = %g: sampler %s, hit pdf (top, side, bottom) x (cut+, r, r+) %s" % (r, pdf.tolist(), got.tolist()))
    assert (got[:, :2] == 0).all() and (got[1:, 2] == 0).all()
    assert abs(got[0, 2] - hit_top) <= 1e-6 * hit_top
    if r == 0.03:   # the area form's own value: |p - ref| = one float of r, cos = -1
        d = float(np.nextafter(F32(r), F32(9))) - float(F32(r))
        assert abs(hit_top - d * d / (4 * np.pi * float(F32(r)) ** 2)) <= 1e-5 * hit_top


@functools.lru_cache(maxsize=None)
def directional_scene():
    from practical_path_guiding_lab_amd import scene as S
    return _with_lights(S, _floor(S), [S.sphere((0.0, 0.0, 0.0), 1.0, 0)], [S.directional_light((0.0, -0.6, -0.8), (1.5, 2.5, 3.5))])


def directional_cases():
    """p at the bounding sphere's centre, inside it, outside it (twice), and n perpendicular to the light, along it, against it"""
    sc = directional_scene()
    c, R = sc.bounding_sphere()[:3].astype(np.float64), float(sc.bounding_sphere()[3])
    p = [c, c + (1, 2, 3), c + (2 * R, 0, 0), c + (0, -3 * R, R)]
    n = [(0, 0, 1), (1, 0, 0), (0, 0.8, -0.6), (0, -0.6, -0.8), (0, 0.6, 0.8)]
    return lanes([q for q in p for _ in n], n * len(p), (0.7, 0.1))


def test_directional_light():
    sc, L = directional_scene(), directional_cases()
    T = EM.Tables(sc)
    out = probe_oracle(sc, L)
    _, _, v = check(T, L, out, "directional", cap=False)
    d = np.asarray(sc.dir_lights, F32)[0]
    assert (out["ds_d"] == -d[0:3]).all() and (out["ds_delta"] == 1).all() and (out["need_shadow"] == 1).all()
    assert (out["ds_pdf"] == 1).all() and (out["em_weight"] == d[3:6]).all()
    R = float(T.bsphere[3])
    L_rec = out["sh_o"].astype(np.float64) + out["sh_d"] * (out["sh_tmax"].astype(np.float64) / EM.ONE_MINUS_SHADOW)[:, None]
    dist = np.linalg.norm(L_rec - L["p"], axis=1)
    want = 2 * np.maximum(R, np.linalg.norm(L["p"] - T.bsphere[:3], axis=1))
    assert (np.abs(dist - want) <= 1e-5 * want).all() and abs(dist[0] - 2 * R) <= 1e-5 * R and dist[-1] > 6 * R
    # n perpendicular to the light: n . ds_d = 0 exactly (0.8 * 0.6 - 0.6 * 0.8 in float32) -- not below 0: the offset is +n
    k = 2
    assert (out["sh_o"][k] - L["p"][k])[1] > 0 and v.why["side"][k]


def non_finite_lanes(name):
    """the broad set's first 96 lanes with NaN, inf and 0 in p and n"""
    L = {k: a[:96].copy() for k, a in broad(name).items() if k != "prim"}
    nan, inf = F32(np.nan), F32(np.inf)
    L["p"][0:8], L["p"][8:16, 1], L["p"][16:24], L["p"][24:32] = nan, inf, -inf, 0
    L["n"][32:40], L["n"][40:48, 2], L["n"][48:56], L["n"][56:64] = nan, inf, -inf, 0
    L["p"][64:72], L["n"][64:72] = nan, nan
    return L


@pytest.mark.parametrize("name", ["mixed", "torus", "cornell-box"])
def test_oracle_returns_for_non_finite_points_and_normals(name):
    """what tests/test_gpu_emitter.py then asks of the device; the choice and the density do not depend on n"""
    L = non_finite_lanes(name)
    out = probe_oracle(scene(name), L)
    good = probe_oracle(scene(name), {k: a[:96] for k, a in broad(name).items()})
    assert set(np.unique(out["ds_delta"])) <= {0, 1} and set(np.unique(out["need_shadow"])) <= {0, 1}
    for k in ("ds_d", "ds_pdf", "em_weight", "ds_delta", "need_shadow"):
        assert np.array_equal(out[k][32:64], good[k][32:64], equal_nan=True), k
    assert not ((out["ds_pdf"] > 0) & (out["ds_delta"] == 0))[0:8].any()    # from a NaN point no area light is sampled


def test_a_scene_without_emitters_gives_zero_lanes():
    from practical_path_guiding_lab_amd import scene as S
    sc = TS._finish(_floor(S), None, MATS(S), None, None, None)
    L = lanes([(0.3, 0.2, 0.0), (1.0, 2.0, 3.0)], (0.0, 0.0, 1.0), [(0.0, 0.0), (1.0, 1.0)])
    out = probe_oracle(sc, L)
    assert EM.Tables(sc).count == 0 and not EM.judge(EM.Tables(sc), L["p"], L["n"], L["e"], out)[0]
    assert (out["sh_d"] == (0, 0, 1)).all() and (out["ds_pdf"] == 0).all() and (out["need_shadow"] == 0).all()


def known_cases():
    """(label, scene, lanes) of every known-answer input above: what tests/test_gpu_emitter.py feeds the device and the oracle"""
    for count in (1, 2, 3, 7):
        yield "list of %d" % count, list_scene(count), lanes((0.3, 0.2, 0.0), (0.0, 0.0, 1.0), choice_samples(count))
    yield "quad", quad_scene(), quad_cases()
    for r in (2.0, 0.03):
        yield "sphere r = %g" % r, sphere_scene(r), sphere_cases(r)
    yield "directional", directional_scene(), directional_cases()
    for r in (2.0, 0.03):
        yield "gap r = %g" % r, sphere_scene(r), gap_cases(r)[1]


# ---- the density a grid of samples has ----

BINS_C, BINS_P, SUB = 24, 24, 32
GRID = 256
PAIRS = ("oblique quad", "two spheres and a quad", "small sphere close up", "list of 3")
# per pair, twice the oracle's own (worst bin difference, |valid fraction - mass|) at the committed grid
# (profiles/emitter/band.txt: 2.18e-04 2.64e-05, 1.88e-03 4.86e-05, 0 0, 5.94e-04 1.31e-03).  What the oracle is off by is
# the grid's own grain: a row of 256 cell centres lands on one side of a bin's edge (256 / 65536 = 3.9e-3 at most), and where
# a small light takes a third of all samples into a few bins, that is what shows.  The single sphere's bins have no grain
# (below) and the oracle's difference there is 0: its tolerance is float64's own rounding of the sums, 1e-12 -- a lane in
# another bin is 1.5e-5.
BIN_TOLERANCE = dict(zip(PAIRS, (4.4e-4, 3.8e-3, 1e-12, 1.2e-3)))
MASS_TOLERANCE = dict(zip(PAIRS, (5.3e-5, 9.8e-5, 1e-12, 2.7e-3)))
# (bins in cos theta, bins in phi, margin of the binned range over the emitters' extent) where a pair has its own.  A single
# sphere above the small-angle switch: cos theta is linear in e1 alone and phi in e2 alone, so with the range taken exactly and
# 16 bins each way every bin holds exactly 16 x 16 of the 256 x 256 cell centres -- the grid has no grain there, and the bins
# see a change of the distribution that 24 x 24 bins over a wider range hid behind one (a row of cells more or less per bin).
PAIR_BINS = {"small sphere close up": (16, 16, 1.0)}


def bins_of(pair):
    return PAIR_BINS.get(pair, (BINS_C, BINS_P, 1.05))


@functools.lru_cache(maxsize=None)
def density_scene(pair):
    from practical_path_guiding_lab_amd import scene as S
    if pair == "oblique quad":
        return quad_scene(), (8.2, 0.3, 0.6)
    if pair == "two spheres and a quad":
        sp = [S.sphere((1.0, 2.0, 3.0), 1.0, 1, (5.0, 6.0, 7.0)), S.sphere((-1.5, 2.5, 3.5), 0.4, 1, (1.0, 1.0, 1.0))]
        return TS._finish(_floor(S) + _quad_light(S, (0.0, 0.0, 5.0), 0.5, (3.0, 2.0, 1.0)) * 1, sp, MATS(S), None, None, None), (0.2, 0.4, 8.5)
    if pair == "small sphere close up":
        return sphere_scene(0.03), (0.03, -0.02, 0.035)
    assert pair == "list of 3"
    return list_scene(3), (0.5, 1.0, 9.0)


def density_frame(T, p, margin=1.05):
    """axis: the mean direction from p to the area emitters; cos_lo: the cosine of `margin` times the angle they reach to"""
    p = np.asarray(p, np.float64)
    dirs, lows = [], []
    for prim in T.emitters[T.emitters >= 0]:
        if prim < T.first_sphere:
            Q = T.quads[prim]
            pts = np.array([Q[0:3] + a * Q[3:6] + b * Q[6:9] for a in (0, 1) for b in (0, 1)])
            dirs.append(SM._unit(Q[0:3] + 0.5 * Q[3:6] + 0.5 * Q[6:9] - p))
            lows.append((SM._unit(pts - p), 0.0))
        else:
            S_ = T.spheres[prim - T.first_sphere]
            d = np.linalg.norm(S_[0:3] - p)
            dirs.append((S_[0:3] - p) / d)
            lows.append((((S_[0:3] - p) / d)[None], np.arcsin(min(1.0, S_[3] / d))))
    axis = SM._unit(np.sum(dirs, axis=0))
    worst = max(float(np.arccos(np.clip(pts @ axis, -1, 1)).max()) + a for pts, a in lows)
    return axis, float(np.cos(min(np.pi, margin * worst)))


def _bins(d, axis, cos_lo, BINS_C, BINS_P):
    s, t = SM.duff(axis[None])
    c = d @ axis
    ph = np.arctan2(d @ t[0], d @ s[0])
    i = np.floor((c - cos_lo) / (1 - cos_lo) * BINS_C).astype(np.int64)
    j = np.minimum(np.floor((ph + np.pi) / (2 * np.pi) * BINS_P).astype(np.int64), BINS_P - 1)
    return np.minimum(i, BINS_C - 1), j, (c >= cos_lo)


@functools.lru_cache(maxsize=None)
def model_mass(pair):
    """the model density integrated over each bin by the midpoint rule: sum over the emitters of 1 / count times the solid-angle
    density wherever the float64 ray from p meets that emitter's front"""
    sc, p = density_scene(pair)
    T = EM.Tables(sc)
    p = np.asarray(p, np.float64)
    BINS_C, BINS_P, margin = bins_of(pair)
    axis, cos_lo = density_frame(T, p, margin)
    cs = cos_lo + (np.arange(BINS_C * SUB) + 0.5) / (BINS_C * SUB) * (1 - cos_lo)
    ps = (np.arange(BINS_P * SUB) + 0.5) / (BINS_P * SUB) * 2 * np.pi - np.pi
    Cc, Pp = np.meshgrid(cs, ps, indexing="ij")
    s, t = SM.duff(axis[None])
    sn = np.sqrt(1 - Cc ** 2)
    w = (sn * np.cos(Pp))[..., None] * s[0] + (sn * np.sin(Pp))[..., None] * t[0] + Cc[..., None] * axis
    dens = np.zeros(Cc.shape)
    for prim in T.emitters[T.emitters >= 0]:
        if prim < T.first_sphere:
            Q = T.quads[prim]
            nl = Q[9:12]
            den = w @ nl
            with np.errstate(divide="ignore", invalid="ignore"):
                tt = ((Q[0:3] - p) @ nl) / den
                x = p + tt[..., None] * w - Q[0:3]
                a, b = (x @ Q[3:6]) * Q[12], (x @ Q[6:9]) * Q[13]
                hit = (tt > 0) & (den < 0) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
                dens += np.where(hit, tt ** 2 / (np.abs(den) * Q[14]), 0.0) / T.count
        else:
            S_ = T.spheres[prim - T.first_sphere]
            oc = S_[0:3] - p
            D2 = oc @ oc
            if D2 <= (S_[3] * (1 - EM.K_SPHERE)) ** 2:
                continue
            b = w @ oc
            hit = (b > 0) & (b * b - D2 + S_[3] ** 2 >= 0)
            dens += np.where(hit, 1 / (2 * np.pi * (1 - np.sqrt(1 - S_[3] ** 2 / D2))), 0.0) / T.count
    dw = ((1 - cos_lo) / cs.size) * (2 * np.pi / ps.size)
    return (dens * dw).reshape(BINS_C, SUB, BINS_P, SUB).sum(axis=(1, 3))


def density_lanes(pair, grid=GRID):
    sc, p = density_scene(pair)
    g = (np.arange(grid) + 0.5) / grid
    e = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    return sc, lanes(p, (0.0, 0.0, 1.0), e)


def density_differences(pair, probe, grid=GRID):
    """-> (worst bin difference, |valid fraction - the model's mass|, lanes that took a directional light) of a sampler:
    probe(scene, lanes) -> the probe's columns"""
    sc, L = density_lanes(pair, grid)
    T = EM.Tables(sc)
    out = probe(sc, L)
    BINS_C, BINS_P, margin = bins_of(pair)
    axis, cos_lo = density_frame(T, L["p"][0], margin)
    area = (out["ds_pdf"] > 0) & (out["ds_delta"] == 0)
    i, j, inside = _bins(out["ds_d"][area].astype(np.float64), axis, cos_lo, BINS_C, BINS_P)
    assert inside.all()                                # every sampled direction lies within the emitters' extent
    h = np.zeros((BINS_C, BINS_P))
    np.add.at(h, (i, j), 1.0 / L["p"].shape[0])
    m = model_mass(pair)
    return float(np.abs(h - m).max()), float(abs(h.sum() - m.sum())), int((out["ds_delta"] != 0).sum())


@pytest.mark.parametrize("pair", PAIRS)
def test_sampling_density(pair):
    worst, mass, directional = density_differences(pair, probe_oracle)
    print("%s: worst bin %.3e (tolerance %.3e), valid fraction against the model's mass %.3e (tolerance %.3e), %d directional lanes" % (
        pair, worst, BIN_TOLERANCE[pair], mass, MASS_TOLERANCE[pair], directional))
    assert worst <= BIN_TOLERANCE[pair] and mass <= MASS_TOLERANCE[pair]
    # a directional entry takes exactly its 1 / count share: the cells of the grid whose e1 count falls in its interval
    T = EM.Tables(density_scene(pair)[0])
    cells = np.floor((np.arange(GRID) + 0.5) / GRID * T.count)
    assert directional == GRID * int((T.emitters[np.minimum(cells, T.count - 1).astype(int)] < 0).sum())
