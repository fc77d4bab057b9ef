"""Per-call kernel split of the LCP builds in a rocprofv3 database (profiles/r05_lcp_kernel_stats.csv).

rocprofv3 --kernel-trace --stats -d DIR -o lcp -- python tools/lcp_bench.py --calls 2 --no-host --kasai-max-mib 0 \
    --only c2_uniform_256m,c3_english_256m,all_one_byte_256m,fibonacci_256m
python tools/lcp_kernel_split.py DIR/lcp_results.db > profiles/r05_lcp_kernel_stats.csv

An LCP call is every dispatch from its k_ci_range (the range pass; the suffix-array build never launches it) to its k_lcp_gather;
calls are given to the workloads in lcp_bench.py's order, calls + 1 per workload."""
import collections
import re
import sqlite3
import sys

db=sqlite3.connect(sys.argv[1])
rows=list(db.execute("select name, start, end from kernels order by start"))
names=["c2_uniform_256m","c3_english_256m","all_one_byte_256m","fibonacci_256m"]
calls_per = int(sys.argv[2]) if len(sys.argv) > 2 else 3
def short(nm):
    nm=re.sub(r"\(.*","",nm); nm=re.sub(r"^void ","",nm); nm=nm.replace("sa::","")
    return nm
inside=False; call=-1
acc=collections.OrderedDict()
for nm,s,e in rows:
    k=short(nm)
    if k=="k_ci_range":
        inside=True; call+=1
    if not inside: continue
    if k.startswith("k_post_words"): continue
    w=names[call//calls_per]
    d=acc.setdefault(w,collections.OrderedDict()); st=d.setdefault(k,[0,0]); st[0]+=1; st[1]+=(e-s)
    if k=="k_lcp_gather": inside=False
out=["workload,kernel,launches_per_call,ms_per_call,share_of_kernel_time"]
for w,d in acc.items():
    tot=sum(v[1] for v in d.values())
    for k,(c,ns) in sorted(d.items(), key=lambda kv:-kv[1][1]):
        out.append(f"{w},\"{k}\",{c/calls_per:.1f},{ns/calls_per/1e6:.3f},{ns/tot:.3f}")
    out.append(f"{w},TOTAL kernel time,,{tot/calls_per/1e6:.3f},1.000")
print("\n".join(out))
