# A/B helper: one short headline run per value of an environment switch.  usage: VAR=NAME VALS="a b" bash scripts/ab_headline.sh
# (an empty-string value is written as "-": the variable is then left unset)
cd $GRAFT_REPO_ROOT
for v in $VALS; do
  if [ "$v" = "-" ]; then unset $VAR; else export $VAR=$v; fi
  # (--full: the parity sample against oracle/cbmps.c comes with the CPU baseline)
  python bench.py --full --steps ${STEPS:-3} --warmup 1 --no-route-check --no-energy-check --no-sweeps --no-latency --no-other-modes --no-full-rank --no-real-rank --cpu-seconds 4 2>/dev/null | python -c '
import json, sys
d = json.loads(sys.stdin.read())
print("'$VAR=$v'", round(d["value"], 1), round(d["ms_per_step"], 1), {k: round(x / d["steps"], 1) for k, x in d["kernel_ms"].items()}, d.get("parity_on_sample", {}).get("max_rel_err_amplitude"))'
done
