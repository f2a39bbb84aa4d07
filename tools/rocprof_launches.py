"""Per-launch duration statistics (avg, sd, min, percentiles, max) of the kernels whose name contains a
substring, from a rocprofv3 rocpd database.   usage: python tools/rocprof_launches.py <results.db> <substring>"""
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
sub = sys.argv[2]
names = {r[0]: r[1] for r in db.execute('select id, display_name from rocpd_info_kernel_symbol')}
agg = {}
for kid, s, e in db.execute('select kernel_id, start, end from rocpd_kernel_dispatch order by start'):
    n = names.get(kid, '?')
    if sub in n:
        agg.setdefault(n[:70], []).append((e - s) / 1e3)
for n, d in agg.items():
    ds = sorted(d)
    m = sum(d) / len(d)
    sd = (sum((x - m) ** 2 for x in d) / max(1, len(d) - 1)) ** 0.5
    print(f'{n:70s} n={len(d)} avg={m:.1f} sd={sd:.1f} min={ds[0]:.1f} p10={ds[len(d) // 10]:.1f} '
          f'med={ds[len(d) // 2]:.1f} p90={ds[(9 * len(d)) // 10]:.1f} max={ds[-1]:.1f} us')
