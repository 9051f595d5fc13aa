"""Start of a kernel -> start of the next one, per launch of the replayed step, from a rocprofv3 kernel trace of bench.py:
   python tools/step_boundaries.py <trace directory>  -> position, kernel, grid, median duration, median start-to-start.
What a launch leaves dirty in the write-back L2 drains at its end or in front of its successor: the duration alone does not
show it, the distance between the two starts does (medians over every replayed step of the trace)."""
import csv, glob, os, statistics, sys
root = sys.argv[1]
f = sorted(glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True))[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp']))
ANCHOR = sys.argv[2] if len(sys.argv) > 2 else 'drug_mix_gather_fwd_kernel'   # a kernel that is launched once per step
fw = [i for i, r in enumerate(rows) if ANCHOR in r['Kernel_Name']]
steps = [(a, b) for a, b in zip(fw, fw[1:]) if b - a > 10]
per = {}
for a, b in steps:
    per[b - a] = per.get(b - a, 0) + 1
period = max(per, key=per.get)
steps = [(a, b) for a, b in steps if b - a == period]
start = lambda i: int(rows[i]['Start_Timestamp'])
for k in range(period):
    r = rows[steps[0][0] + k]
    name = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '')[:46]
    dur = statistics.median((int(rows[a + k]['End_Timestamp']) - start(a + k)) / 1e3 for a, _ in steps)
    nxt = statistics.median((start(a + k + 1) - start(a + k)) / 1e3 for a, _ in steps)
    print('%2d  %-46s %8sx%s  dur %6.2f  to next start %6.2f' % (k + 1, name, r['Grid_Size_X'], r['Grid_Size_Y'], dur, nxt))
print('%d steps; median step span %.2f us' % (len(steps), statistics.median((start(b) - start(a)) / 1e3 for a, b in steps)))
