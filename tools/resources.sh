#!/bin/bash
# (here, no GPU) registers / scratch / LDS / occupancy of every kernel, one line each: make resource-usage, condensed.
# Usage: tools/resources.sh [extra -D flags]
make -s -C "$(dirname "$0")/../gelato_amd/csrc" resource-usage XFLAGS="$*" | python3 -c "
import sys, re, subprocess
cur = None
for l in sys.stdin:
    m = re.search(r'Function Name: (\S+)', l)
    if m:
        cur = m.group(1); rec = {}
        continue
    m = re.search(r'remark: +(\w[\w /\[\]-]*): (\S+)', l)
    if m and cur:
        rec[m.group(1).strip()] = m.group(2)
        if m.group(1).startswith('LDS Size'):
            name = subprocess.run(['c++filt', cur], capture_output=True, text=True).stdout.strip()
            name = re.sub(r'\(.*', '', name)
            print('%-70s VGPR %-4s AGPR %-3s SGPR %-4s scratch %-4s occ %-2s LDS %s' % (name[:70], rec.get('VGPRs'), rec.get('AGPRs'), rec.get('TotalSGPRs'), rec.get('ScratchSize [bytes/lane]'), rec.get('Occupancy [waves/SIMD]'), rec.get('LDS Size [bytes/block]')))
"
