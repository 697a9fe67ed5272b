"""The any-hit form of the BVH walk's node step (csrc/pg_render_dev.hpp, bvh_node_step<., true>) through pg_scene_intersect in
all three probe forms, against the CPU oracle.  The form is unordered -- the first child the ray reaches next, the later ones
pushed as references alone, nothing dropped when popped -- and promises the boolean only (which occluder, after how many
steps, is not the oracle's), so the boolean is what is compared, on sets the oracle calls occluded and unoccluded in
comparable shares: an always-true or always-false walk cannot pass.  (The closest-hit form is unchanged and stays with
tests/test_gpu_raycast.py, bit for bit.)"""
import functools

import numpy as np
import pytest

import raycast_model as RM
import test_gpu_raycast as GR
import test_raycast_model as TM

pytestmark = pytest.mark.gpu

SCENES = ("veach-ajar", "torus", "mixed")
N = 1 << 15
SIZES = (1, 63, 64, 65, 257, N)
FACTORS = np.array([0.25, 0.999, 1.0, 1.001, 4.0, np.inf], np.float32)   # before, at, just behind, far behind the closest hit; none
WEIGHTS = (0.1, 0.15, 0.15, 0.2, 0.2, 0.2)


def rays_in_leaf_boxes(T, n, seed):
    """origins inside the boxes of leaves (children of the node table whose reference names triangles), any direction"""
    rng = np.random.default_rng(seed)
    planes = T.bvh[:, :24].view(np.float32).reshape(-1, 2, 3, 4)
    refs = T.bvh[:, 24:28]
    nd, ch = np.nonzero((refs != 0xffffffff) & ((refs & 0x80000000) != 0))
    pick = rng.integers(0, nd.shape[0], n)
    lo, hi = planes[nd[pick], 0, :, ch[pick]].astype(np.float64), planes[nd[pick], 1, :, ch[pick]].astype(np.float64)
    d = rng.standard_normal((n, 3))
    return (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def any_hit_pool(name):
    """N rays, shuffled so that every prefix holds all kinds -- aimed at triangles (interiors, edges, vertices), leaving
    surfaces, uniform, from inside leaf boxes, NaN and zero-direction rays -- with limits around the oracle's closest hit,
    and the oracle's answer under those limits: made once, shared, never changed"""
    from oracle import pg_oracle as po
    T = TM.tables(name)
    kinds = [RM.rays_interior, RM.rays_edge, RM.rays_vertex, RM.rays_surface, RM.rays_uniform, rays_in_leaf_boxes]
    o_deg, d_deg = TM.degenerate_rays(name)
    per = (N - o_deg.shape[0]) // len(kinds) + 1
    o, d = zip(*[k(T, per, 501 + i) for i, k in enumerate(kinds)])
    o, d = np.concatenate(o + (o_deg,)), np.concatenate(d + (d_deg,))
    order = np.random.default_rng(6).permutation(o.shape[0])[:N]
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    t0, p0 = po.intersect(TM.scene(name), o, d)[:2]
    f = np.random.default_rng(7).choice(FACTORS, N, p=WEIGHTS)
    with np.errstate(invalid="ignore"):
        tmax = np.where(np.isfinite(t0) & (p0 >= 0), t0 * f, np.float32(np.inf)).astype(np.float32)
    return o, d, tmax, po.intersect(TM.scene(name), o, d, tmax)[1] >= 0


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("name", SCENES)
def test_any_hit_says_what_the_oracle_says(name, form):
    o, d, tmax, want = any_hit_pool(name)
    assert o.shape[0] == N and np.isnan(o).any() and np.isnan(d).any() and (d == 0).all(1).any()
    for n in SIZES[2:]:   # (from one wave on, every prefix holds both answers in comparable shares)
        assert 0.3 <= want[:n].mean() <= 0.7, (n, want[:n].mean())
    for n in SIZES:
        got = GR.cast(name, o[:n], d[:n], tmax[:n], any_hit=True, form=form)[1] >= 0
        np.testing.assert_array_equal(got, want[:n], err_msg="%s form %d n %d" % (name, form, n))
