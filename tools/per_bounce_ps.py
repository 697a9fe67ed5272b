"""Dev tool: what a mesh scene's bounces cost per lane, from a rocprofv3 kernel trace of bench.py --full.
  python tools/per_bounce_ps.py TRACE_DIR BENCH_DETAIL.json [passes]
A pass = the kernels between two k_finish launches.  Of the passes that ran the joint shading kernel (k_wave_shade: the
timed region of `value`, not the pg_render_stages(2) region behind it) the last `passes` (default 3) are averaged.  Launch b
of k_wave_shade in a pass is bounce b; launch b of k_wave_trace is bounce b + 1 (the joint form's first launch walks the camera
rays itself: bounce 0 has no k_wave_trace and its column reads 0); the lanes that went into it are the film's for bounce 0 and
config.paths_alive_after_bounce[b - 1] of the detail file after that.  Also prints which bounces a sort ran in front of
(the k_sort_hist launches between two k_wave_trace launches: two per sort) and the sort kernels' time there."""
import csv
import glob
import json
import sys

d, detail = sys.argv[1], json.load(open(sys.argv[2]))
n_avg = int(sys.argv[3]) if len(sys.argv) > 3 else 3
f = sorted(glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True))[0]
rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f)))
passes, cur = [], []
for s, e, k in rows:
    cur.append((k, (e - s) / 1e3))
    if "k_finish" in k:
        passes.append(cur)
        cur = []
joint = [p for p in passes if any("k_wave_shade<" in k for k, _ in p)][-n_avg:]
cfg = detail["config"]
live = [int(x) for x in cfg["paths_alive_after_bounce"]]
lanes = [int(cfg["paths_per_step"])] + live[:-1]
D = len(live)
shade = [[] for _ in range(D)]
trace = [[] for _ in range(D)]
sort_us = [[] for _ in range(D)]
hists = [[] for _ in range(D)]
for p in joint:
    b_shade, b_trace, su, nh = 0, 0, 0.0, 0  # (the first k_wave_trace of a joint pass is bounce 1's)
    for k, us in p:
        if "k_wave_trace<" in k:
            b_trace += 1
            trace[b_trace].append(us)
            su, nh = 0.0, 0
        elif "k_sort_" in k:
            su += us
            nh += 1 if "k_sort_hist" in k else 0
        elif "k_wave_shade<" in k:
            shade[b_shade].append(us)
            sort_us[b_shade].append(su)
            hists[b_shade].append(nh)
            b_shade += 1
    assert b_shade == D and b_trace == D - 1, (b_shade, b_trace, D)


def mean(x):
    return sum(x) / len(x) if x else 0.0


print(f"# {detail['extra']['library']}  {cfg['workload'][:60]}...  mean of the last {len(joint)} passes of the timed region")
print(f"# ms_per_step under the trace {detail['ms_per_step']}")
print("bounce   lanes in    k_wave_shade us  ps/lane    k_wave_trace us  ps/lane    sort us  k_sort_hist launches")
tot_h = 0
for b in range(D):
    n = max(lanes[b], 1)
    h = mean(hists[b])
    tot_h += h
    print("%4d  %11d   %14.1f  %7.1f   %14.1f  %7.1f   %8.1f  %g" % (
        b, lanes[b], mean(shade[b]), 1e6 * mean(shade[b]) / n, mean(trace[b]), 1e6 * mean(trace[b]) / n, mean(sort_us[b]), h))
print("sum   %11d   %14.1f            %14.1f            %8.1f  %g per pass" % (
    sum(lanes), sum(mean(x) for x in shade), sum(mean(x) for x in trace), sum(mean(x) for x in sort_us), tot_h))
