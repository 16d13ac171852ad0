"""Print the kernel sequence of the LAST full train step from a rocprofv3 --kernel-trace CSV (kernel name, us)."""
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
# a step ends with its last rdg_adam_multi_kernel launch (a step launches it more than once: the rows' Adam next to the MLP
# backward, then the MLP + pose bucket); the launches per step = adam launches / compositing-backward launches (one per step)
idx = [i for i, r in enumerate(rows) if "rdg_adam_multi_kernel" in r["Kernel_Name"]]
n_steps = sum("rdg_render_bwd_kernel" in r["Kernel_Name"] for r in rows)
per = max(1, round(len(idx) / max(1, n_steps)))
ends = idx[per - 1::per]
# a plain bench.py run: the warm-up steps, the untimed settling steps, then the timed steps, all without events: by default
# the LAST step, which is the last timed step (argv[2]: the index of another step, 1 = the second step of the trace)
which = int(sys.argv[2]) if len(sys.argv) > 2 else len(ends) - 1
a, b = ends[which - 1], ends[which]
t0 = int(rows[a]["End_Timestamp"])
prev_end = t0
tot = 0
for r in rows[a + 1:b + 1]:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    print(f"{(s - t0) / 1e3:9.1f} us  +gap {(s - prev_end) / 1e3:6.1f}  dur {(e - s) / 1e3:7.1f}  {r['Kernel_Name'][:110]}")
    prev_end = e
    tot += e - s
print("span us", (int(rows[b]["End_Timestamp"]) - t0) / 1e3, "busy us", tot / 1e3)
