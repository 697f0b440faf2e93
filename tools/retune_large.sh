#!/bin/bash
# Re-times only the conv shapes of at least 1024 tokens (the ones the split-bf16 kernels of conv_x3.hip are offered for), except
# the one-clip R = 32 step's (B1, L <= 2048: the headline plan stays as tuned), and keeps every other entry of the committed table.
# Run on an MI355X box: bash tools/retune_large.sh.  Output: tune_out/tune_gfx950.txt (copy it over moditalker_amd/csrc/tune_gfx950.txt).
cd "$(dirname "$0")/.."
O=tune_out
mkdir -p $O
export MTV_TUNE_CACHE=$PWD/$O/tune_raw.txt
python - <<'PY'
import os
import re
keep = []
for line in open("moditalker_amd/csrc/tune_gfx950.txt"):
    m = re.match(r"B(\d+) L(\d+)/", line)
    if line.startswith("#") or (m and int(m.group(1)) * int(m.group(2)) >= 1024 and not (int(m.group(1)) == 1 and int(m.group(2)) <= 2048)):
        continue
    keep.append(line)
open(os.environ["MTV_TUNE_CACHE"], "w").writelines(keep)
print(len(keep), "entries kept")
PY
# (--full: the batched-clips and R = 64 legs are what meets the large shapes)
timeout 900 python bench.py --full --steps 20 --warmup 2 --ramp-steps 5 --no-cpu-baseline --batched-clips 8 > $O/retune_bench_b8.json
timeout 600 python bench.py --full --res 64 --steps 10 --warmup 2 --ramp-steps 5 --no-cpu-baseline --batched-clips 0 > $O/retune_bench_r64.json
timeout 300 python tools/ae_profile.py > $O/retune_ae_decode.txt
timeout 300 python tools/ae_profile.py --extract > $O/retune_ae_extract.txt
(echo "# conv shape -> measured best tile (MT NT NW KS XM); regenerate with tools/make_tune_table.sh on an MI355X"; sort -u $MTV_TUNE_CACHE) > $O/tune_gfx950.txt
wc -l $O/tune_gfx950.txt; grep -c " 48 1 0" $O/tune_gfx950.txt
