# VALU instruction counts of the square-root kernel (k_fe_sqrt<FqCfg> over 2^20 elements, tools/bench_wire.py
# --sqrt-only): one rocprofv3 --pmc pass of its own, no tracing beside it, summarised per dispatch into
# <out>/summary.json (wave-instructions; one wave is 64 roots).  Run from the repository root on the MI355X;
# argument: the output directory (default profiles/pmc_wire).
O=${1:-profiles/pmc_wire}; rm -rf $O; mkdir -p $O
C="SQ_INSTS_VALU SQ_INSTS_VALU_INT64 SQ_INSTS_VALU_INT32 SQ_WAVES"
timeout -s KILL 240 rocprofv3 --pmc $C --output-format csv -d $O/sqrt -o run -- python3 tools/bench_wire.py --sqrt-only --reps 3 > $O/sqrt.log 2>&1 || { tail -5 $O/sqrt.log; exit 1; }
python3 - $O <<'PY' || exit 1
import json, os, sys
sys.path.insert(0, "tools")
from pmc_summary import load, summarise
out = sys.argv[1]
rows = {k.split("(")[0]: v for k, v in summarise(load(os.path.join(out, "sqrt"))).items() if "k_fe_sqrt" in k}
assert rows, "no dispatches of k_fe_sqrt"
for v in rows.values():
    v["valu_per_root"] = v["SQ_INSTS_VALU"] / v["SQ_WAVES"]  # a wave-instruction is one instruction of each of its 64 roots
    v["int64_per_root"] = v["SQ_INSTS_VALU_INT64"] / v["SQ_WAVES"]
    v["units"] = "wave-instructions per dispatch; per root = per wave"
json.dump(rows, open(os.path.join(out, "summary.json"), "w"), indent=1)
print(json.dumps(rows))
PY
rm -rf $O/sqrt  # the raw counter files; summary.json and sqrt.log stay
