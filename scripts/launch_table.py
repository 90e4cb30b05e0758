"""rocprofv3 kernel trace (csv) -> one line per (kernel, queue numbered by first appearance, grid) with its launch count, sorted: the table a host-side
refactor must leave byte-identical (profiles/r15, profiles/r17).  python scripts/launch_table.py <kernel_trace.csv> > table.txt"""
import csv, re, sys
from collections import Counter
rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r['Start_Timestamp']), r))
rows.sort(key=lambda x: x[0])
queues, cnt = {}, Counter()
for _, r in rows:
    q = queues.setdefault(r['Queue_Id'], len(queues))
    name = re.sub(r'\(.*', '', r['Kernel_Name']).replace('void pivp::', '').replace('pivp::', '')
    cnt[(name, q, '%sx%sx%s' % (r['Grid_Size_X'], r['Grid_Size_Y'], r['Grid_Size_Z']))] += 1
print('%d launches on %d queues' % (len(rows), len(queues)))
for (name, q, grid), c in sorted(cnt.items()):
    print('%-110s q%d  %-16s %5d' % (name[:110], q, grid, c))
