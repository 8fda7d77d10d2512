#!/bin/bash
# usage: tools/bench_stages.sh <logname> [bench args...]   -- runs GPU tests + bench and prints the stage table
log=$1; shift
export O=${O:-profile_out}; mkdir -p $O      # where the logs go (kept out of git)
timeout 600 python -m pytest tests -m gpu -x -q > $O/gputests.log 2>&1; echo "tests rc=$?"; tail -2 $O/gputests.log
python bench.py --full "$@" > $O/$log 2>&1      # (--full: the kernel path and its roofline are read below)
python - "$log" <<PY
import json,os,sys
O=os.environ["O"]+"/"
l=[x for x in open(O+sys.argv[1]) if x.startswith("{")]
if l:
    d=json.loads(l[-1]); print("value %.1f Gbases/s  ms/step %.3f  dom frac %.3f pipeline frac %.3f"%(d["value"],d["ms_per_step"],d["roofline"]["frac"],d["roofline"]["pipeline_frac"]))
    for k,v in d["roofline"]["stage_ms_per_step"].items(): print("  %-32s %.3f"%(k,v))
    if "cpu_baseline" in d: print("  cpu:",d["cpu_baseline"])
else: print(open(O+sys.argv[1]).read()[-3000:])
PY
