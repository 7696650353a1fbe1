#!/usr/bin/env python
"""Compare the per-kernel resources of two builds without a GPU.

    make -C pgw4era5_amd/csrc asm          # in each tree: writes resource_usage.txt (-Rpass-analysis=kernel-resource-usage)
    python tools/kernel_resources.py OLD/resource_usage.txt NEW/resource_usage.txt [--json OUT]

Every kernel of OLD must exist in NEW with the same SGPRs, VGPRs, AGPRs, scratch, LDS and occupancy; kernels only NEW
has are listed.  Names are demangled (llvm-cxxfilt / c++filt) and the plev-table type is written the same way for both
builds: a kernel that takes the 64-entry table is `PlevTable` whether the build spells it as a struct or as
`PlevTableT<64>`, and the trailing default template argument is dropped.  Exit status 1 when an OLD kernel differs or
is missing."""
import argparse
import json
import re
import shutil
import subprocess
import sys

FIELDS = {'TotalSGPRs': 'sgpr', 'VGPRs': 'vgpr', 'AGPRs': 'agpr', 'ScratchSize [bytes/lane]': 'scratch',
          'Occupancy [waves/SIMD]': 'occupancy', 'LDS Size [bytes/block]': 'lds'}


def parse(path):
    """mangled name -> dict of the figures above"""
    out, cur = {}, None
    pat = re.compile(r'remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis')
    for line in open(path, errors='replace'):
        m = pat.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == 'Function Name':
            cur = out.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    return out


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or '/opt/rocm/llvm/bin/llvm-cxxfilt'
    res = subprocess.run([tool], input='\n'.join(names), capture_output=True, text=True, check=True)
    return res.stdout.splitlines()


def canonical(name):
    name = name.replace('pgw::PlevTableT<64>', 'pgw::PlevTable')
    name = re.sub(r',\s*pgw::PlevTable\s*>\(', '>(', name)         # the trailing template argument at its default
    # k_regrid<T, FU, W, TOUT = T>: a build that names the store type spells the same-type kernels with it
    return re.sub(r'(pgw::k_regrid<(\w+), (\d+), (\d+)), \2>\(', r'\1>(', name)


def table(path):
    raw = parse(path)
    names = list(raw)
    return {canonical(d): raw[m] for m, d in zip(names, demangle(names))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--json', help='write the comparison here')
    a = ap.parse_args()
    old, new = table(a.old), table(a.new)
    missing = sorted(k for k in old if k not in new)
    changed = {k: dict(old=old[k], new=new[k]) for k in old if k in new and old[k] != new[k]}
    added = {k: new[k] for k in sorted(new) if k not in old}
    print('%d kernels in old, %d in new: %d identical, %d changed, %d missing, %d added'
          % (len(old), len(new), len(old) - len(changed) - len(missing), len(changed), len(missing), len(added)))
    for k, v in changed.items():
        print('CHANGED', k, v)
    for k in missing:
        print('MISSING', k)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(dict(old_kernels=len(old), new_kernels=len(new), identical=len(old) - len(changed) - len(missing),
                           changed=changed, missing=missing, added=added), f, indent=1, sort_keys=True)
    return 1 if (changed or missing) else 0


if __name__ == '__main__':
    sys.exit(main())
