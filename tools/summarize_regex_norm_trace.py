"""The kernels' own times of tools/ops_timing.py's RegexNormalization entries, one line per pattern and path.

`rocprofv3 --kernel-trace --stats` adds up every launch of a kernel, and the nine RegexNormalization entries share three kernels, so the
per-pattern figures come from the trace: the launches in start order, (2 warm-up + R timed) calls per entry in the order ops_timing.py
runs them.  Per entry: the mean duration of its count kernel, of its write kernel and of all kernels of a call (check_strings .. write)
over the timed calls.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ops_timing.py --reps R
    python tools/summarize_regex_norm_trace.py DIR R OUT.csv
"""
import csv, glob, sys
prof_dir, reps, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
paths = glob.glob(prof_dir + "/**/*kernel_trace.csv", recursive=True)
assert len(paths) == 1, paths
rows = list(csv.DictReader(open(paths[0])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
name = [r["Kernel_Name"] for r in rows]
dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
variants = ["\\s class", "\\s general forced", "control class", "control general forced", "Han class", "Han general forced",
            "Mn class", "Mn general forced", "clean_up general"]
calls = []   # (count index, write index)
pending = None
for i, nm in enumerate(name):
    if "SubstRow<false" in nm or "SubstRow<(bool)0" in nm:
        pending = i
    elif "SubstRow<true" in nm or "SubstRow<(bool)1" in nm:
        assert pending is not None, i
        calls.append((pending, i))
        pending = None
per = 2 + reps
print("subst calls found:", len(calls), "expected", per * len(variants))
if len(calls) != per * len(variants):
    for nm in sorted(set(n for n in name if "Subst" in n)):
        print(nm)
    sys.exit(3)
with open(out, "w") as f:
    f.write("variant,timed_calls,count_kernel_us,write_kernel_us,all_kernels_of_call_us,kernels_per_call,count_kernel_name\n")
    for v, label in enumerate(variants):
        mine = calls[v * per + 2:(v + 1) * per]
        cu = sum(dur[c] for c, w in mine) / len(mine)
        wu = sum(dur[w] for c, w in mine) / len(mine)
        first = [c - 1 if "check_strings" in name[c - 1] else c for c, w in mine]
        au = sum(sum(dur[a:w + 1]) for a, (c, w) in zip(first, mine)) / len(mine)
        nk = mine[0][1] - first[0] + 1
        f.write(f"{label},{len(mine)},{cu:.1f},{wu:.1f},{au:.1f},{nk},\"{name[mine[0][0]]}\"\n")
print(open(out).read())
