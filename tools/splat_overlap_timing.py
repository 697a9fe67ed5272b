#!/usr/bin/env python3
"""What the deterministic spatial box filter (pg_set_splat_filter, PG_SPATIAL_OVERLAP_BOX) costs pg_splat: 2^20 records of
tests/synth.py's stream into the skewed tree of the filter tests (synth.build_skewed(1 << 15, 5)), for nearest / nearest,
stochastic / box, overlap / nearest and overlap / box in one run.

Per combination: ms per launch (HIP events around `--launches` back-to-back launches after warm-up) and, from the numpy models
of the filters (tests/filter_model.py, tests/filter_overlap_model.py) on the first `--model-records` records, the mean number
of deposits a record makes.  One JSON line on stdout.

    python3 tools/splat_overlap_timing.py [--records 1048576] [--launches 20] [--model-records 65536] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

COMBOS = [("nearest", "nearest"), ("stochastic", "box"), ("overlap", "nearest"), ("overlap", "box")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-records", type=int, default=1 << 16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import filter_model as fm
    import filter_overlap_model as fom
    import synth
    from practical_path_guiding_lab_amd.sdtree import SDTree

    bb0, bb1 = [0.0] * 3, [100.0] * 3
    cols = synth.build_skewed(1 << 15, 5).prev.export()
    host = synth.records(a.records, 41, bb0, bb1)
    rec = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    g = SDTree(0)
    g.load(cols)
    st = g.stats()
    out = {"records": a.records, "launches": a.launches,
           "forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes),
                      "mean_quad_leaf_depth": round(st.mean_quad_leaf_depth, 3), "max_quad_depth": int(st.max_quad_depth)},
           "ms": {}, "deposits_per_record": {}}
    for spatial, directional in COMBOS:
        g.setSplatFilter(spatial, directional, seed=1)
        for _ in range(a.warmup):
            g.addDataPropagate(rec)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            g.addDataPropagate(rec)
        e1.record()
        e1.synchronize()
        out["ms"][spatial + "/" + directional] = round(e0.elapsed_time(e1) / a.launches, 4)
    n = min(a.model_records, a.records)
    if n > 0:
        sub = {k: np.ascontiguousarray(v[..., :n]) for k, v in host.items()}
        for spatial, directional in COMBOS:
            r = fom.splat(cols, sub, directional) if spatial == "overlap" else fm.splat(cols, sub, spatial, directional, seed=1)
            out["deposits_per_record"][spatial + "/" + directional] = round(r["deposits"] / n, 4)
            if spatial == "overlap":
                out["kd_leaves_per_filtered_record"] = round(r["item"].size / max(int(r["filtered"].sum()), 1), 3)
    near = out["ms"]["nearest/nearest"]
    out["ratio_to_nearest"] = {k: round(v / near, 3) for k, v in out["ms"].items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
