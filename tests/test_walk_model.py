"""Why an any-hit walk needs no order (csrc/pg_render_dev.hpp, bvh_node_step<., true>), restated in numpy (tests/walk_model.py)
on the scenes' own BVHs: until its first triangle the ray keeps its length, every waiting entry was pushed under that length,
so nothing is ever dropped when popped -- a node is opened if and only if the ray reaches the boxes of all its ancestors.
An unoccluded ray therefore opens the same nodes in any order, and an occluded one finds some occluder either way."""
import numpy as np
import pytest

import raycast_model as RM
import test_raycast_model as TM
import walk_model as WM

N = 1 << 12


def _rays(name):
    """uniform rays and rays aimed at triangles; limits before and behind the BVH's closest hit, and none"""
    T = TM.tables(name)
    o1, d1 = RM.rays_uniform(T, N // 2, 31)
    o2, d2 = RM.rays_interior(T, N // 2, 32)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    _, t0, _, _ = WM.walk(T, o, d, np.full(N, np.inf, np.float32), False, True)
    rng = np.random.default_rng(33)
    f = rng.choice(np.array([0.25, 0.999, 1.0, 1.001, 4.0, np.inf], np.float32), N)
    with np.errstate(invalid="ignore"):
        tmax = np.where(np.isfinite(t0), t0 * f, np.float32(np.inf)).astype(np.float32)
    return T, o, d, tmax


@pytest.mark.parametrize("name", ["torus", "veach-ajar"])
def test_the_unordered_any_hit_walk_opens_what_the_ordered_one_opens(name):
    T, o, d, tmax = _rays(name)
    best_o, _, open_o, leaves_o = WM.walk(T, o, d, tmax, True, True)
    best_u, _, open_u, leaves_u = WM.walk(T, o, d, tmax, True, False)
    occluded = best_o >= 0
    assert 0.3 < occluded.mean() < 0.7, occluded.mean()
    np.testing.assert_array_equal(best_u >= 0, occluded)                       # the answer, every ray
    free = ~occluded
    np.testing.assert_array_equal(open_u[free], open_o[free])                  # the nodes, every unoccluded ray
    np.testing.assert_array_equal(leaves_u[free], leaves_o[free])
    # (walks in which an order exists -- several nodes opened -- not root-only rays: 375 and 700 unoccluded rays here open
    # more than four nodes, 1587 and 4091 rays more than the root)
    assert (open_o[free].sum(1) > 4).sum() > 256 and (open_o.sum(1) > 1).sum() > N // 4
    # the closest-hit walk agrees on who is occluded: the any-hit answer is "the closest-hit walk finds something"
    best_c = WM.walk(T, o, d, tmax, False, True)[0]
    np.testing.assert_array_equal(best_c >= 0, occluded)

