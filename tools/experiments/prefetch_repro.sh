O=${1:?usage: prefetch_repro.sh OUT_DIR}; mkdir -p "$O"
for env in "TINYMPC_KPI_SEPARATE=1" "X=1"; do
for o in "prefetch=0" "prefetch=-1"; do
env $env python bench.py --full --steps 20 --warmup 5 --no-configs --no-cpu-baseline --min-seconds 1 --opt $o --details $O/bd.json > $O/b.json 2>/dev/null
python - "$env $o" "$O/bd.json" <<'PY'
import json,sys
d=json.load(open(sys.argv[2]))
r=d['regimes']; b=r['beyond_l3']
print(sys.argv[1], 'inside', round(r['steady_state']['ms_per_launch'],4), round(r['steady_state_per_instance_refs']['ms_per_launch'],4), 'beyond', round(b['steady_state']['ms_per_launch'],4), round(b['steady_state_per_instance_refs']['ms_per_launch'],4))
PY
done
done
