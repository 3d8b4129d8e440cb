O=${1:?usage: prefetch_bench_vs_probe.sh OUT_DIR}; mkdir -p "$O"
for o in "prefetch=0" "prefetch=-1"; do
python bench.py --full --steps 20 --warmup 5 --no-configs --no-cpu-baseline --min-seconds 1 --opt $o --details $O/bd_$o.json > $O/b_$o.json 2>/dev/null
python - "$o" "$O" <<'PY'
import json,sys
o=sys.argv[1]
d=json.load(open('%s/bd_%s.json'%(sys.argv[2],o)))
r=d['regimes']; b=r['beyond_l3']
print(o, 'inside', r['steady_state']['ms_per_launch'], r['steady_state_per_instance_refs']['ms_per_launch'], 'beyond', b['steady_state']['ms_per_launch'], b['steady_state_per_instance_refs']['ms_per_launch'])
PY
done
BATCHES=262144 timeout 600 python tools/prefetch_probe.py warm
