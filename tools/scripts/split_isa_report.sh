#!/bin/bash
# Regenerates profiles/split_isa_report.txt from the SHIPPED sources: hipcc -S of learn-fhe_amd/csrc/fhew_api.hip with the
# compiler's resource-usage remarks, tools/split_isa_check.py on the split blind-rotation kernels.  No GPU needed.
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
tmp=$(mktemp -d)
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -S --cuda-device-only \
    -Rpass-analysis=kernel-resource-usage -o $tmp/fhew_api.s $R/learn-fhe_amd/csrc/fhew_api.hip 2> $tmp/remarks.txt
python3 $R/tools/split_isa_check.py $tmp/fhew_api.s $tmp/remarks.txt | tee $R/profiles/split_isa_report.txt
rm -rf $tmp
