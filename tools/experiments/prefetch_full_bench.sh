O=${1:?usage: prefetch_full_bench.sh OUT_DIR}; mkdir -p "$O"
for o in "prefetch=0" "prefetch=-1" "prefetch=0" "prefetch=-1"; do
python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --opt $o --details $O/bd.json > $O/b.json 2>/dev/null
python - "$o" "$O/bd.json" <<'PY'
import json,sys
d=json.load(open(sys.argv[2]))
r=d['regimes']; b=r['beyond_l3']
print(sys.argv[1], 'inside', round(r['steady_state']['ms_per_launch'],4), round(r['steady_state_per_instance_refs']['ms_per_launch'],4), 'beyond', round(b['steady_state']['ms_per_launch'],4), round(b['steady_state_per_instance_refs']['ms_per_launch'],4), 'config3', d['configs']['config3']['ms'] if 'configs' in d else None)
PY
done
