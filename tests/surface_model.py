"""The surface at a hit in float64 numpy, written from the specifications and not from either implementation: what
pgo_surface_probe (oracle) and pg_surface_probe (device) are held to.

Specifications
  hit point     p = o + t d (quads, box faces, triangles).
  sphere        p lies on the sphere, at radius r from the centre c along x = o + t d - c; n = x / |x|: unit and radial.
  quad, box     n = ng = the stored normal (a box face: + or - the stored axis), bit for bit.
  triangle      ng = the stored face normal, bit for bit; n = the normalised blend (1 - u - v) N0 + u N1 + v N2 of the vertex
                normals, or the face normal where the blend's squared length is 0 (or where the mesh has no vertex normals).
  texture       uv = (1 - u - v) uv0 + u uv1 + v uv2, then to_uv (scale, offset).  bitmap: texel centres at (i + 1/2) / size,
                repeat wrap, the four neighbours decoded through the scene's 8-bit sRGB table and blended in linear light (a
                function that is continuous across texel borders and across the wrap).  checkerboard: color0 where
                frac(u') > 1/2 and frac(v') > 1/2 agree, else color1.  Coordinates whose texel position is NaN or not below
                1e9 in magnitude are taken as position 0 (they would not fit an int).
  frame         (s, t, n) is orthonormal and right-handed, and is Duff et al.'s (2017) branchless basis of n, which is what
                Mitsuba's coordinate_system builds; wi holds the components of -d in it; to_world inverts to_local.
  emitter pdf   0 where the emitter faces away from ref (cos >= 0 for cos = (p - ref) . n / |p - ref|); else, times 1 / count:
                quad     |p - ref|^2 / (|cos| A);
                sphere   1 / (2 pi (1 - cos alpha)) with sin alpha = r / |c - ref| (the cone the sphere subtends), and beyond
                         the cap limit sin alpha >= 1 - 2^-24 (ref on or inside the sphere) the area form
                         |p - ref|^2 / (|cos| 4 pi r^2).

Bands.  Every quantity q carries the bracket  2^-24 ops |q| + sum_j |dq/dx_j| ulp(x_j)  over its float32 inputs x_j (one-sided
float64 differences of one unit in the last place, the greater of the two sides), and passes within C times it.  The input
term stands for the roundings of intermediate results of the inputs' size -- it is what covers the cancellation in o + t d, in
p - c after the re-projection, in a blend of opposed normals, in x - floor(x) at large texture coordinates.  ops, the float32
roundings on the quantity's own path:
  p (flat shapes)   2   product, sum
  p (sphere)       14   x (3), x . x (5), root, quotient, r n0, c + .  -- and |p - c| = r within the same bracket
  n (sphere)       22   the above, then p - c, its square (5), root, quotient
  n (triangle)     14   1 - u - v (2), the blend (5), its square (5), root, quotient
  refl (bitmap)    24   1 - u - v (2), uv blend (5), to_uv (2), texel position (2), the weights (2), two row blends (3 each), the
                        column blend (3), floor and wrap exact;  |q| is taken as the largest of the four texels
  frame            16   (dots and lengths, against 0 or 1: |q| := 1) Duff's components (5), a dot (5), n's own defect from unit
                        length (6: three squares, two sums, the root behind it)
  frame vs Duff     6   per component: reciprocal, two products, a sum, the sign products
  wi                5   a 3-term dot;  its bracket uses sum |d_k s_k|, not |q|
  back             12   to_world (5) over wi (5) and the frame's defect;  |q| := |d|
  pdf (quad)       17   p - ref, its square (5), root, quotient, dot (5), |cos| A, quotient, 1 / count, product
  pdf (cone)       20   c - ref, its square (5), root, quotient, square, 1 - ., root, 1 - ., 2 pi ., quotient, 1 / count, product;
                        and two intermediate results get a term of their own, because one unit in their last place is NOT small
                        against them: m = 1 - sin^2 alpha (absolute error 2^-24 whatever m is: a reference point close to the
                        sphere) and 1 - cos alpha (cos alpha is rounded to 2^-25 near 1: a small or distant sphere; the mixed
                        scene's r = 0.03 light seen from 3 units away loses ten bits here).  These are properties of the
                        formula in float32, shared by Mitsuba; the bracket names them instead of C swallowing them.
  pdf (area form)  19   as the quad's, with 4 pi r^2

Decisions within float32's own reach are AMBIGUOUS; the lane must then equal the model under one assignment of the decision:
  checkerboard     frac(u') or frac(v') within the band of 1/2, or of 0 / 1 (where floor flips)       -> either colour
  blended normal   squared length within its band of 0                                                -> blend or face normal
  emitter pdf      cos within its band of 0                              -> 0, or any density at least that of the band's edge
                   sin alpha within its band of the cap limit                                         -> cone or area form
  bitmap           |texel position| within its band of 1e9                                            -> position 0 or not
C per quantity (BAND_C) is four times the worst ratio measured on the CPU oracle over the suite's own input sets
(profiles/surface/band.txt, written by tools/surface_mutants.py --band).
"""
import numpy as np

EPS = 2.0 ** -24
CAP_LIMIT = float(np.float32(0.99999994))
AMBIGUOUS_CAP = 0.02
# four times the worst |difference| / bracket measured on the oracle (profiles/surface/band.txt); 64 would mean a missing term
BAND_C = {"p": 1.52, "radius": 1.11, "n": 1.29, "refl": 2.25, "frame": 0.89, "duff": 0.97, "wi": 1.25, "back": 0.72, "pdf": 1.96}
OPS = {"p_flat": 2, "p_sphere": 14, "n_sphere": 22, "n_tri": 14, "refl": 24, "frame": 16, "duff": 6, "wi": 5, "back": 12,
       "pdf_quad": 17, "pdf_cone": 20, "pdf_area": 19}


def ulp(x):
    """one unit in the last place of the float32 nearest to x (x: float64 holding float32 values)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def bracket(f, xs, ops, scale=None, steps=None, nan_is_inf=False):
    """q = f(*xs) and 2^-24 ops |q| + sum_j max |f(.. x_j +- ulp ..) - q|; xs: float64 arrays (n,) or (n, k) of float32 values.
    steps[j], where given, stands in the place of ulp(x_j); nan_is_inf: a bracket that is not a number comes back as inf"""
    q = f(*xs)
    b = EPS * ops * (np.abs(q) if scale is None else scale)
    for j, x in enumerate(xs):
        h = ulp(x) if steps is None or steps[j] is None else np.broadcast_to(steps[j], x.shape)
        cols = [()] if x.ndim == 1 else [(slice(None), k) for k in range(x.shape[1])]
        for c in cols:
            worst = 0.0
            for sgn in (1.0, -1.0):
                y = x.copy()
                y[c] = y[c] + sgn * h[c]
                worst = np.maximum(worst, np.abs(f(*xs[:j], y, *xs[j + 1:]) - q))
            b = b + worst
    return q, np.nan_to_num(b, nan=np.inf) if nan_is_inf else b


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


class Tables:
    """the float32 tables of a scene as float64 arrays, and the shape numbering"""

    def __init__(self, sc):
        f = lambda a, w: np.asarray(a, np.float32).reshape(-1, w).astype(np.float64)
        self.quads, self.spheres, self.boxes, self.tris = f(sc.quads, 24), f(sc.spheres, 12), f(sc.boxes, 32), f(sc.tris, 16)
        self.mats = None if sc.materials is None else f(sc.materials, 16)
        self.normals = None if sc.tri_normals is None else f(sc.tri_normals, 9)
        self.uvs = None if sc.tri_uvs is None else f(sc.tri_uvs, 6)
        self.textures = np.asarray(sc.textures, np.uint32).reshape(-1, 16)
        self.texels = np.asarray(sc.texels, np.uint32)
        self.lut = np.asarray(sc.srgb_lut, np.float32).astype(np.float64)
        self.first_sphere = self.quads.shape[0]
        self.first_box = self.first_sphere + self.spheres.shape[0]
        self.first_tri = self.first_box + 6 * self.boxes.shape[0]
        self.n_shapes = self.first_tri + self.tris.shape[0]
        self.n_emitters = int((self.quads[:, 15] != 0).sum() + (self.spheres[:, 5] != 0).sum() + len(sc.dir_lights))

    def kind(self, prim):
        """0 quad, 1 sphere, 2 box face, 3 triangle"""
        return (prim >= self.first_sphere).astype(int) + (prim >= self.first_box) + (prim >= self.first_tri)


def bitmap(T, tex, uu, vv):
    """the bilinear, wrapped, linear-light lookup at to_uv'ed coordinates (uu, vv) of bitmap descriptor rows tex (n, 16) ->
    ((n, 3) colours, (n,) the largest texel value met, (n, 2) texel positions before the 1e9 cut)"""
    W, H, first = tex[:, 1].astype(np.int64), tex[:, 2].astype(np.int64), tex[:, 3].astype(np.int64)
    pos = np.stack([uu * W - 0.5, vv * H - 0.5], axis=1)
    with np.errstate(invalid="ignore"):
        x = np.where(np.abs(pos[:, 0]) < 1e9, pos[:, 0], 0.0)
        y = np.where(np.abs(pos[:, 1]) < 1e9, pos[:, 1], 0.0)
    fx, fy = np.floor(x), np.floor(y)
    wx, wy = x - fx, y - fy
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    out, top = np.zeros((uu.shape[0], 3)), np.zeros(uu.shape[0])
    for dx, dy, w in ((0, 0, (1 - wx) * (1 - wy)), (1, 0, wx * (1 - wy)), (0, 1, (1 - wx) * wy), (1, 1, wx * wy)):
        word = T.texels[first + ((iy + dy) % H) * W + ((ix + dx) % W)]
        rgb = np.stack([T.lut[(word >> s) & 255] for s in (0, 8, 16)], axis=1)
        out += w[:, None] * rgb
        top = np.maximum(top, rgb.max(axis=1))
    return out, top, pos


class Quantity:
    """exact value q, bracket b, and where a decision is doubtful (amb) the value under the other assignment (alt, alt_b)"""

    def __init__(self, q, b):
        self.q, self.b = q, b
        self.amb = np.zeros(q.shape[0], bool)
        self.alt, self.alt_b = q.copy(), b.copy()
        self.at_least = np.full(q.shape[0], np.inf)   # (emitter pdf at grazing incidence: anything from here up ...
        self.graze = np.zeros(q.shape[0], bool)       #  ... or 0)


class Model:
    pass


@np.errstate(invalid="ignore", over="ignore", divide="ignore")
def surface(T, prim, o, d, t, u, v, c_for_decisions=None):
    """the model's answers for hits (prim, o, d, t, u, v): exact columns, and Quantity objects for p, n, refl"""
    C = c_for_decisions or BAND_C
    prim = np.asarray(prim, np.int64)
    o, d, t, u, v = (np.asarray(a, np.float32).astype(np.float64) for a in (o, d, t, u, v))
    n_l = prim.shape[0]
    kind = T.kind(prim)
    m = Model()
    m.kind, m.prim = kind, prim
    m.is_em, m.radiance, m.row = np.zeros(n_l, np.int32), np.zeros((n_l, 3)), np.full(n_l, -1, np.int64)
    m.ng = np.zeros((n_l, 3))
    p_q, p_b = bracket(lambda o_, d_, t_: o_ + t_[:, None] * d_, [o, d, t], OPS["p_flat"])
    n_q, n_b = np.zeros((n_l, 3)), np.zeros((n_l, 3))
    m.radius = np.full(n_l, np.nan)
    m.centre = np.zeros((n_l, 3))
    k = kind == 0
    Q = T.quads[prim[k]]
    m.ng[k], n_q[k], m.is_em[k], m.radiance[k], m.row[k] = Q[:, 9:12], Q[:, 9:12], Q[:, 15] != 0, Q[:, 19:22], Q[:, 22].astype(np.int64)
    m.quad_refl = np.zeros((n_l, 3))
    m.quad_refl[k] = Q[:, 16:19]
    k = kind == 2
    f = prim[k] - T.first_box
    B = T.boxes[f // 6]
    axis = (f % 6) // 2
    nb = np.take_along_axis(B[:, 12:21].reshape(-1, 3, 3), axis[:, None, None].repeat(3, axis=2), axis=1)[:, 0] * np.where(f % 2 == 1, -1.0, 1.0)[:, None]
    m.ng[k], n_q[k], m.row[k] = nb, nb, B[:, 21].astype(np.int64)
    k = kind == 1
    if k.any():
        S = T.spheres[prim[k] - T.first_sphere]
        c, r = S[:, 0:3], S[:, 3]
        radial = lambda o_, d_, t_, c_: _unit(o_ + t_[:, None] * d_ - c_)
        n_q[k], n_b[k] = bracket(radial, [o[k], d[k], t[k], c], OPS["n_sphere"])
        p_q[k], p_b[k] = bracket(lambda o_, d_, t_, c_, r_: c_ + r_[:, None] * radial(o_, d_, t_, c_), [o[k], d[k], t[k], c, r], OPS["p_sphere"])
        m.ng[k] = np.nan                        # (= n: judged through n)
        m.radius[k], m.centre[k] = r, c
        m.is_em[k], m.radiance[k], m.row[k] = S[:, 5] != 0, S[:, 6:9], S[:, 4].astype(np.int64)
    m.p, m.n = Quantity(p_q, p_b), Quantity(n_q, n_b)
    k = kind == 3
    ti = prim[k] - T.first_tri
    R = T.tris[ti]
    m.ng[k], m.row[k] = R[:, 9:12], R[:, 12].astype(np.int64)
    m.n.q[k] = R[:, 9:12]
    if k.any() and T.normals is not None:
        N = T.normals[ti]
        blend = lambda u_, v_, N_: (1 - u_ - v_)[:, None] * N_[:, 0:3] + u_[:, None] * N_[:, 3:6] + v_[:, None] * N_[:, 6:9]
        l2, l2_b = bracket(lambda u_, v_, N_: _dot(blend(u_, v_, N_), blend(u_, v_, N_)), [u[k], v[k], N], 12)
        with np.errstate(invalid="ignore", divide="ignore"):
            q, b = bracket(lambda u_, v_, N_: _unit(blend(u_, v_, N_)), [u[k], v[k], N], OPS["n_tri"])
        zero = l2 == 0
        doubt = l2 <= C["n"] * l2_b
        idx = np.nonzero(k)[0]
        face = R[:, 9:12]
        m.n.q[idx], m.n.b[idx] = np.where(zero[:, None], face, q), np.where(zero[:, None], 0.0, np.nan_to_num(b, nan=np.inf, posinf=np.inf))
        m.n.amb[idx] = doubt
        m.n.alt[idx], m.n.alt_b[idx] = np.where(zero[:, None], np.nan, face), 0.0   # (exactly 0: only the face normal, or whatever a rounded blend gives)
        m.n.any_unit = np.zeros(n_l, bool)
        m.n.any_unit[idx] = zero                 # the exact blend vanishes: a rounded one points anywhere -- any unit vector or the face normal
    # materials: the row's columns, and the reflectance a texture replaces
    m.type, m.one_sided = np.zeros(n_l, np.int64), np.zeros(n_l, np.int64)
    refl = m.quad_refl.copy()
    if T.mats is not None:
        M = T.mats[m.row]
        m.type, m.one_sided, refl = M[:, 0].astype(np.int64), (M[:, 11] != 0).astype(np.int64), M[:, 1:4].copy()
    m.refl = Quantity(refl, np.zeros((n_l, 3)))
    m.textured = np.zeros(n_l, bool)
    if T.mats is not None and T.uvs is not None and k.any():
        tex_i = T.mats[m.row, 12].astype(np.int64) - 1
        tx = np.nonzero(k & (tex_i >= 0))[0]
        if tx.size:
            m.textured[tx] = True
            D = T.textures[tex_i[tx]]
            F = D[:, 4:14].copy().view(np.float32).astype(np.float64)   # color0, color1, scale (u, v), offset (u, v)
            U = T.uvs[prim[tx] - T.first_tri]
            to_uv = lambda u_, v_, U_, F_, a: ((1 - u_ - v_) * U_[:, a] + u_ * U_[:, 2 + a] + v_ * U_[:, 4 + a]) * F_[:, 6 + a] + F_[:, 8 + a]
            uu, uu_b = bracket(lambda *x: to_uv(*x, 0), [u[tx], v[tx], U, F], 9)
            vv, vv_b = bracket(lambda *x: to_uv(*x, 1), [u[tx], v[tx], U, F], 9)
            chk = D[:, 0] == 2
            q, b = np.zeros((tx.size, 3)), np.zeros((tx.size, 3))
            alt, amb = np.zeros((tx.size, 3)), np.zeros(tx.size, bool)
            if chk.any():
                fu, fv = uu - np.floor(uu), vv - np.floor(vv)
                same = (fu > 0.5) == (fv > 0.5)
                q[chk] = np.where(same[:, None], F[:, 0:3], F[:, 3:6])[chk]
                alt[chk] = np.where(same[:, None], F[:, 3:6], F[:, 0:3])[chk]
                near = lambda fr, bb: (np.abs(fr - 0.5) <= bb) | (fr <= bb) | (1 - fr <= bb)
                amb[chk] = (near(fu, C["refl"] * uu_b) | near(fv, C["refl"] * vv_b))[chk]
            bm = ~chk
            if bm.any():
                lookup = lambda u_, v_, U_, F_: bitmap(T, D[bm], to_uv(u_, v_, U_, F_, 0), to_uv(u_, v_, U_, F_, 1))
                top, pos = lookup(u[tx][bm], v[tx][bm], U[bm], F[bm])[1:]
                q[bm], b[bm] = bracket(lambda *x: lookup(*x)[0], [u[tx][bm], v[tx][bm], U[bm], F[bm]], OPS["refl"], top[:, None])
                # the 1e9 cut: with the position moved to the other side of it
                W_H = D[bm][:, 1:3].astype(np.float64)
                pos_b = np.stack([uu_b[bm], vv_b[bm]], axis=1) * W_H + EPS * 2 * np.abs(pos)
                with np.errstate(invalid="ignore"):
                    cut = np.abs(np.abs(pos) - 1e9) <= C["refl"] * pos_b
                amb[bm] = cut.any(axis=1)
                if cut.any():
                    a = alt[bm]
                    with np.errstate(invalid="ignore"):
                        flipped = np.where(cut, np.where(np.abs(pos) < 1e9, np.inf, np.sign(pos) * 0.999e9), pos)
                    a[cut.any(axis=1)] = bitmap(T, D[bm], (flipped[:, 0] + 0.5) / W_H[:, 0], (flipped[:, 1] + 0.5) / W_H[:, 1])[0][cut.any(axis=1)]
                    alt[bm] = a
            m.refl.q[tx], m.refl.b[tx], m.refl.alt[tx], m.refl.amb[tx] = q, b, alt, amb
            m.refl.alt_b[tx] = np.where(chk[:, None], 0.0, np.inf)   # (beyond the cut the weights are noise: any blend of texels)
    return m


def duff(n, sign=None):
    """Duff et al. 2017, "Building an Orthonormal Basis, Revisited" (Mitsuba's coordinate_system): s, t of unit n"""
    sign = np.where(np.signbit(n[:, 2]), -1.0, 1.0) if sign is None else sign
    a = -1.0 / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    s = np.stack([1.0 + sign * n[:, 0] ** 2 * a, sign * b, -sign * n[:, 0]], axis=1)
    return s, np.stack([b, sign + n[:, 1] ** 2 * a, -n[:, 1]], axis=1)


@np.errstate(invalid="ignore", over="ignore", divide="ignore")
def cone_density(ref, c, r, inv):
    """the density 1 / (2 pi (1 - cos alpha)) times inv of the cone a sphere (c, r) subtends from ref, sin alpha = r / |c - ref|
    -> (sin alpha, its bracket, the density, its bracket, cos alpha, d_ca: the absolute error float32 leaves in cos alpha)"""
    sinf = lambda r_, c_, rad_: rad_ / np.sqrt(_dot(c_ - r_, c_ - r_))
    sin, sin_b = bracket(sinf, [ref, c, r], 8)
    mm = 1 - sin ** 2
    ca = np.sqrt(np.maximum(mm, 0.0))
    cone = lambda r_, c_, rad_: inv / (2 * np.pi * (1 - np.sqrt(np.maximum(1 - sinf(r_, c_, rad_) ** 2, 0.0))))
    cq, cb = bracket(cone, [ref, c, r], OPS["pdf_cone"])
    # the two intermediate results whose last place is not small against them (module docstring)
    d_ca = ulp(ca) + (ulp(mm) + 3 * EPS * sin ** 2) / (2 * np.maximum(ca, 1e-300))
    return sin, sin_b, cq, cb + cq / (1 - ca) * d_ca, ca, d_ca


def emitter_pdf(T, m, ref, p, n, C=None):
    """the density for hits m.prim at the implementation's own p and n (float32 values), seen from ref -> Quantity (n,)"""
    C = C or BAND_C
    ref, p, n = (np.asarray(a, np.float32).astype(np.float64) for a in (ref, p, n))
    n_l = ref.shape[0]
    out = Quantity(np.zeros(n_l), np.zeros(n_l))
    em = m.is_em != 0
    if not em.any() or T.n_emitters == 0:
        return out
    inv = 1.0 / T.n_emitters
    cosf = lambda r_, p_, n_: _dot(_unit(p_ - r_), n_)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos, cos_b = bracket(cosf, [ref, p, n], 13)
        faces = cos < 0
        doubt = np.abs(cos) <= C["pdf"] * cos_b
        area = np.ones(n_l)
        k = em & (m.kind == 0)
        area[k] = T.quads[m.prim[k], 14]
        k = em & (m.kind == 1)
        area[k] = 4 * np.pi * m.radius[k] ** 2
        form = lambda r_, p_, n_: _dot(p_ - r_, p_ - r_) / np.abs(cosf(r_, p_, n_)) / area * inv
        q, b = bracket(form, [ref, p, n], OPS["pdf_area"])
        edge = _dot(p - ref, p - ref) / (np.abs(cos) + C["pdf"] * cos_b) / area * inv * (1 - C["pdf"] * OPS["pdf_area"] * EPS)
        use_area = np.ones(n_l, bool)
        if k.any():   # the cone
            c, r = m.centre, np.where(k, m.radius, 1.0)
            sin, sin_b, cq, cb, _, _ = cone_density(ref, c, r, inv)
            in_cone = k & (sin < CAP_LIMIT)
            lim = k & (np.abs(sin - CAP_LIMIT) <= C["pdf"] * sin_b) & faces
            use_area = ~in_cone
            out.amb |= lim
            out.alt[lim], out.alt_b[lim] = np.where(in_cone, q, cq)[lim], np.where(in_cone, b, cb)[lim]
            q, b = np.where(in_cone, cq, q), np.where(in_cone, cb, b)
        b = np.nan_to_num(b, nan=np.inf)
        out.q, out.b = np.where(em & faces, q, 0.0), np.where(em & faces, b, 0.0)
        # grazing: 0, or the facing value -- whose area form has no upper end there: anything from the band's edge up
        g = em & doubt
        out.graze = g
        out.at_least[g & use_area] = edge[g & use_area]
        only = g & ~out.amb
        out.alt[only], out.alt_b[only] = np.where(faces, 0.0, q)[only], np.where(faces, 0.0, b)[only]
        out.amb |= g
    return out


def _within(got, q, b, c):
    with np.errstate(invalid="ignore"):
        d = np.abs(got - q)
        ok = (d <= c * b) | (got == q)
    return ok if ok.ndim == 1 else ok.all(axis=1)


def _ratio(got, q, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(got == q, 0.0, np.abs(got - q) / b)
    r = np.nan_to_num(r, nan=np.inf)
    return r if r.ndim == 1 else r.max(axis=1)


def judge(T, m, out, d, ref, level, C=None):
    """out: the probe's columns (oracle.pg_oracle.SURFACE_FIELDS / SURFACE_FLAGS) for the hits the model m was made of.
    -> (failures: name -> lanes, ratios: band name -> (n,) |difference| / bracket on lanes without a doubtful decision,
        ambiguous: (n,) bool)"""
    C = C or BAND_C
    f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    d, n_l = f64(d), m.prim.shape[0]
    g = {k: f64(out[k]) for k in ("p", "n", "ng", "refl", "radiance", "normal_at", "emitter_pdf", "s", "t", "wi", "back")}
    bad, ratio = {}, {}
    amb = np.zeros(n_l, bool)

    def fail(name, ok):
        bad[name] = np.nonzero(~ok)[0]

    def banded(name, band, quantity, got, sel=None):
        sel = np.ones(n_l, bool) if sel is None else sel
        ok = _within(got, quantity.q, quantity.b, C[band])
        other = quantity.amb & _within(got, quantity.alt, quantity.alt_b, C[band])
        fail(name, ok | other | ~sel)
        r = np.where(sel & ~quantity.amb, _ratio(got, quantity.q, quantity.b), 0.0)
        ratio[band] = np.maximum(ratio.get(band, 0.0), r)
        amb[:] |= quantity.amb & sel
        return ok | other

    # exact columns
    fail("row", out["row"] == (-1 if level == 0 else m.row))
    fail("flags", (out["type"] == m.type) & (out["one_sided"] == m.one_sided) & (out["is_em"] == m.is_em))
    fail("radiance", (g["radiance"] == m.radiance).all(axis=1))
    flat = m.kind != 1
    fail("ng", np.where(flat, (g["ng"] == m.ng).all(axis=1), (g["ng"] == g["n"]).all(axis=1)))
    # the property the next bounce relies on: the normal recomputed from (prim, p) is the geometric normal, bit for bit
    fail("normal_at", (np.asarray(out["normal_at"], np.float32).view(np.uint32) == np.asarray(out["ng"], np.float32).view(np.uint32)).all(axis=1))
    banded("p", "p", m.p, g["p"])
    sph = m.kind == 1
    if sph.any():   # on the sphere
        dist = np.sqrt(_dot(g["p"] - m.centre, g["p"] - m.centre))
        rb = EPS * OPS["p_sphere"] * m.radius + 1.75 * ulp(g["p"]).max(axis=1) + ulp(m.radius)
        fail("on the sphere", ~sph | (np.abs(dist - m.radius) <= C["radius"] * rb))
        ratio["radius"] = np.where(sph, np.abs(dist - m.radius) / rb, 0.0)
    # n: triangles whose exact blend vanishes may hold any unit vector (a rounded blend's direction is noise)
    ok = banded("n", "n", m.n, g["n"])
    if getattr(m.n, "any_unit", None) is not None and m.n.any_unit.any():
        unit = np.abs(_dot(g["n"], g["n"]) - 1) <= C["frame"] * EPS * OPS["frame"]
        bad["n"] = np.nonzero(~(ok | (m.n.any_unit & unit)))[0]
    # reflectance: exact where no texture applies
    ok = banded("refl", "refl", m.refl, g["refl"], m.textured)
    any_texel = m.refl.amb & np.isinf(m.refl.alt_b).any(axis=1) & (g["refl"] >= 0).all(axis=1) & (g["refl"] <= 1).all(axis=1)
    bad["refl"] = np.nonzero(~(ok | any_texel | ~m.textured))[0]
    fail("refl (plain)", m.textured | (g["refl"] == m.refl.q).all(axis=1))
    # the frame on the implementation's own n
    s, t, n = g["s"], g["t"], g["n"]
    defects = np.stack([_dot(s, t), _dot(s, n), _dot(t, n), _dot(s, s) - 1, _dot(t, t) - 1, _dot(n, n) - 1], axis=1)
    hand = np.cross(s, t) - n
    fb = EPS * OPS["frame"]
    fail("frame orthonormal", (np.abs(defects) <= C["frame"] * fb).all(axis=1))
    fail("frame right-handed", (np.abs(hand) <= C["frame"] * 2 * fb).all(axis=1))
    ratio["frame"] = np.maximum(np.abs(defects).max(axis=1) / fb, np.abs(hand).max(axis=1) / (2 * fb))
    sign = np.where(np.signbit(n[:, 2]), -1.0, 1.0)   # (of the float32 n itself: a sensitivity step must not flip it)
    both = lambda n_: np.concatenate(duff(n_, sign), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        dq, db = bracket(both, [n], OPS["duff"], 1.0)
    banded("frame is Duff's", "duff", Quantity(dq, np.nan_to_num(db, nan=np.inf)), np.concatenate([s, t], axis=1))
    local = lambda d_, s_, t_, n_: -np.stack([_dot(d_, s_), _dot(d_, t_), _dot(d_, n_)], axis=1)
    wq, wb = bracket(local, [d, s, t, n], OPS["wi"], np.stack([np.abs(d * a).sum(axis=1) for a in (s, t, n)], axis=1))
    banded("wi", "wi", Quantity(wq, wb), g["wi"])
    wi = g["wi"]
    world = lambda w_, s_, t_, n_: s_ * w_[:, 0:1] + t_ * w_[:, 1:2] + n_ * w_[:, 2:3]
    bq, bb = bracket(world, [wi, s, t, n], 5, np.abs(s * wi[:, 0:1]) + np.abs(t * wi[:, 1:2]) + np.abs(n * wi[:, 2:3]))
    banded("to_world", "wi", Quantity(bq, bb), g["back"])
    len_d = np.sqrt(_dot(d, d))[:, None]
    inv_b = EPS * OPS["back"] * len_d * np.ones(3) + EPS * OPS["frame"] * len_d
    banded("to_world inverts to_local", "back", Quantity(-d, inv_b), g["back"])
    # emitter pdf at the implementation's own p, n
    e = emitter_pdf(T, m, ref, out["p"], out["n"], C)
    got = g["emitter_pdf"]
    ok = _within(got, e.q, e.b, C["pdf"]) | (e.amb & _within(got, e.alt, e.alt_b, C["pdf"])) | (e.graze & ((got >= e.at_least) | (got == 0)))
    fail("emitter pdf", ok)
    ratio["pdf"] = np.where(e.amb, 0.0, _ratio(got, e.q, e.b))
    amb |= e.amb
    m.pdf = e
    return {k: v for k, v in bad.items() if v.size}, ratio, amb
