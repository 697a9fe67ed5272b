#!/usr/bin/env python3
"""What the learned sampling fraction costs beside the calls it stands next to, one run, one JSON line on stdout.

  query   pg_get_leaf_node_index, pg_pdf and pg_fraction_query on S1 (workload.s1_balanced_tree(), workload.S_QUERIES uniform
          positions).  The query does the former's descent plus one 4-byte gather and the logistic.
  record  pg_splat and pg_fraction_record on S3 (the topology the six splat + refine iterations of S2 leave, its last stream's
          2^24 records), once with uniform positions and once with every record at one position -- all in one leaf, the case
          the kernel's merge is there for.

HIP events around single launches: `--warmup` launches of each call, then `--launches` rounds in which the calls of a group are
timed one after the other (interleaved, so a drift of the device's clocks meets them alike).  Per call: the minimum, the median
and the maximum over the rounds.

    python3 tools/fraction_timing.py [--launches 20] [--warmup 5] [--only query|record] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def interleaved(torch, calls, warmup, launches):
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(launches):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["query", "record"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import SDTree

    out = {"launches": a.launches, "warmup": a.warmup, "library": os.environ.get("PGSD_LIBRARY", "libpgsd.so")}
    if a.only in (None, "query"):
        n = Wk.S_QUERIES
        g = SDTree(0)
        g.load(Wk.s1_balanced_tree())
        g.fractionEnable()
        st = g.stats()
        P = Wk.s_positions_uniform(n, 3, device="cuda")
        D = Wk.s_directions_uniform(n, 4, device="cuda")
        ms = interleaved(torch, {"pg_get_leaf_node_index": lambda: g.getLeafNodeIndex(P), "pg_pdf": lambda: g.pdf(P, D),
                                 "pg_fraction_query": lambda: g.fractionQuery(P)}, a.warmup, a.launches)
        ref = ms["pg_get_leaf_node_index"]
        out["query"] = {"lanes": n, "forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes)}, "ms": ms,
                        "leaf_index_spread_ms": round(ref["max"] - ref["min"], 4)}
        del g
    if a.only in (None, "record"):
        g = SDTree(0)
        g.setup([Wk.S_BBOX[0]] * 3, [Wk.S_BBOX[1]] * 3, 0, 0, 20, 20, True, 0.5)
        rec = None
        for k in range(Wk.S2_ITERATIONS):
            g.setIteration(k, False)
            rec = Wk.s2_record_stream(k, device="cuda")
            g.addDataPropagate(rec)
            g.refineAndPrepare()
        g.setIteration(Wk.S2_ITERATIONS, False)
        g.fractionEnable()
        st = g.stats()
        m = int(rec["radiance"].shape[0])
        u = Wk.s_uniform(m, 9, 3, device="cuda")
        out["record"] = {"records": m, "forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes)}}
        one = torch.tensor([30.0, 40.0, 50.0], device="cuda").reshape(3, 1).expand(3, m).contiguous()
        for name, pos in (("uniform", Wk.s_positions_uniform(m, 8, device="cuda")), ("one_leaf", one)):
            splat = dict(rec, position=pos)
            frec = {"position": pos, "bsdf_pdf": (0.05 + 2.0 * u[0]).contiguous(), "guide_pdf": (0.01 + 4.0 * u[1]).contiguous(),
                    "product": (4.0 * u[2]).contiguous(), "wo_pdf": rec["woPdf"]}
            ms = interleaved(torch, {"pg_splat": lambda: g.addDataPropagate(splat), "pg_fraction_record": lambda: g.fractionRecord(frec)},
                             a.warmup, a.launches)
            out["record"][name] = {"ms": ms, "records_per_s": {k: round(m / (v["median"] * 1e-3), 0) for k, v in ms.items()}}
            acc = g.fractionAccumulators().view(-1, 4)
            out["record"][name]["leaves_hit"] = int((acc[:, 3] > 0).sum())
            g.fractionStep()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
