"""Model of include/pgsd_target.h on top of the CPU oracle: the transform of the leaf accumulators (pg_target_apply), the exact
totals a refine then resolves, and the refine itself from the oracle's separately callable steps.  Nothing of the oracle
changes: its accumulators are read (acc_lo / acc_hi), transformed here with the oracle's own conversions (acc_to_float,
quantize) and numpy's correctly rounded float32 sqrt, summed bottom-up as Python integers, and handed back as the irradiance
column OracleTree.load takes.

Test infrastructure; the product never imports it.
"""
from __future__ import annotations

import numpy as np

from oracle import pg_oracle as po

F = np.float32
_M64 = (1 << 64) - 1


def transform(lo, hi, depth):
    """The transform of one leaf accumulator, operation by operation (pgsd_target.h): value lo + hi 2^64 (uint64, int64) of a
    leaf at `depth` -> (lo, hi) of q."""
    s = po.acc_to_float(lo, hi)
    with np.errstate(invalid="ignore"):
        t = np.where(s > 0, np.sqrt(s, dtype=F), F(0)).astype(F)
    t = (t * np.ldexp(F(1), -np.asarray(depth, np.int32)).astype(F)).astype(F)     # 2^-d, exact
    return po.quantize(t)


def _as_int(lo, hi):
    return np.array([int(h) * (1 << 64) + int(l) for l, h in zip(lo, hi)], dtype=object)


def _split(tot):
    lo = np.array([int(v) & _M64 for v in tot], np.uint64)
    hi = np.array([int(v) >> 64 for v in tot], np.int64)
    return lo, hi


def node_totals(cols, lo, hi):
    """(lo, hi) of every node of the canonical arena after pg_target_apply: leaves transformed, interior nodes the exact integer
    sums of their children.  cols: an export(); lo, hi: the per-node accumulator values before the apply (of the oracle's
    quad_column("acc_lo" / "acc_hi"), or of a device's exportAccumulators())."""
    leaf = np.asarray(cols["quadtree_isLeaf"], bool)
    depth = np.asarray(cols["quadtree_depth"], np.int64)
    ch = [np.asarray(cols["quadtree_child_%d_index" % k], np.int64) for k in (1, 2, 3, 4)]
    tot = np.zeros(leaf.shape[0], dtype=object)
    li = np.nonzero(leaf)[0]
    qlo, qhi = transform(np.asarray(lo, np.uint64)[li], np.asarray(hi, np.int64)[li], depth[li])
    tot[li] = _as_int(qlo, qhi)
    for d in range(int(depth.max()) if depth.size else 0, -1, -1):
        sel = np.nonzero(~leaf & (depth == d))[0]
        if sel.size:
            tot[sel] = tot[ch[0][sel]] + tot[ch[1][sel]] + tot[ch[2][sel]] + tot[ch[3][sel]]
    return _split(tot)


def apply_target(tree: po.OracleTree):
    """node_totals of an oracle tree's own accumulators: what exportAccumulators() of the device shows behind pg_target_apply."""
    return node_totals(tree.export(), tree.quad_column("acc_lo"), tree.quad_column("acc_hi"))


def refine_steps(tree: po.OracleTree, cols, tot_lo, tot_hi, iteration):
    """Steps 5 and 6: the totals become the irradiance column (each rounded once), then the oracle's refine steps in the order
    of pgo_refine_and_prepare.  cols carries the finalised vertCount column."""
    cols = dict(cols)
    cols["quadtree_irradiance"] = po.acc_to_float(tot_lo, tot_hi)
    tree.load(cols)
    tree.set_refinement_threshold(iteration)
    tree.kd_refine()
    tree.set_quadtree_refinement_threshold()
    tree.refine_all_quadtree()
    tree.clean_unused_quadtree()


def model_refine(pair: po.OracleSDTreePair, iteration: int):
    """refineAndPrepareSDTreeForNextIteration with pg_target_apply in front of it."""
    cur = pair.current
    cur.finalize_accumulators()
    lo, hi = cur.quad_column("acc_lo"), cur.quad_column("acc_hi")
    cols = cur.export()
    tot_lo, tot_hi = node_totals(cols, lo, hi)
    refine_steps(cur, cols, tot_lo, tot_hi, iteration)
    pair.prev.copy_from(cur)
    cur.reset()


def squared(rec):
    """The records a host passes for the second moment: radiance and radiance_nee_lum squared, one fp32 multiply each."""
    out = dict(rec)
    for k in ("radiance", "radiance_nee_lum"):
        out[k] = (rec[k].astype(F) * rec[k].astype(F)).astype(F)
    return out


def count_to_float(c):
    """kdtree vertCount of a record count (what repeated fp32 "+1" leaves: exact below 2^24, stuck there after)."""
    return np.minimum(np.asarray(c, np.uint64), np.uint64(1 << 24)).astype(F)
