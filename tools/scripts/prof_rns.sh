cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${PROFILE_OUT:-$R/profile_out}  # profiler output and logs (kept out of git)
mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_rns -- python3 $R/bench.py --full --no-cpu-baseline --steps 2 --warmup 1 > $O/prof_rns.log 2>&1
python3 - <<PY
import csv,glob
f=sorted(glob.glob("$O/prof_rns/**/*kernel_stats.csv",recursive=True))[-1]
for r in csv.DictReader(open(f)):
    n=r["Name"]
    if any(k in n for k in ("rns_","true, 3>","R0")) or "ntt14w" in n: print(n[:100], r["Calls"], r["AverageNs"], r["MaxNs"])
PY
grep -o '"ckks": {[^}]*}' $O/prof_rns.log | cut -c1-300
