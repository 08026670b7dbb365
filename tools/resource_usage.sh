# Per-kernel register / LDS / scratch usage of the gfx950 build (hipcc -Rpass-analysis=kernel-resource-usage):
# every source of csrc/Makefile, each with the flags the Makefile compiles it with
set -o pipefail
D=$(cd "$(dirname "$0")/.." && pwd)/splendor-gym_amd/csrc
for n in $(make -s -C "$D" names); do
  /opt/rocm/bin/hipcc $(make -s -C "$D" flags-$n) --cuda-device-only -c -Rpass-analysis=kernel-resource-usage \
      -o /dev/null "$D/$n.hip" 2>&1
done | python3 -c '
import re, sys, subprocess
rows, cur = [], None
for line in sys.stdin:
    m = re.search(r"remark:\s+(.*?):\s+(.*?) \[-Rpass", line)
    if not m: continue
    k, v = m.group(1).strip(), m.group(2).strip()
    if k == "Function Name":
        cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}; rows.append(cur)
    elif cur is not None:
        cur[k] = v
cols = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
        "LDS Size [bytes/block]"]
print("kernel | " + " | ".join(c.split(" [")[0] for c in cols))
for r in rows:
    if "(" in r["name"] and "k_" in r["name"]:
        print(r["name"].split("(")[0] + " | " + " | ".join(r.get(c, "-") for c in cols))
'
