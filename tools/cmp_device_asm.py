#!/usr/bin/env python3
"""tools/cmp_device_asm.py PARENT_BUILD_DIR RESULT_BUILD_DIR [--strip-comments] [--rename REGEX=REPLACEMENT ...]: compare the device
assembly (-save-temps, build/*-hip-amdgcn-*.s) of two builds kernel by kernel; profiles/retired_switches_asm_identity.txt was made with it.
--rename rewrites symbols of the PARENT before the comparison (a kernel that lost a template argument keeps its body under a new mangled
name); the old -> new names it produced are printed."""
import re, sys, glob, os
STRIP = '--strip-comments' in sys.argv[3:]
RENAMES = [tuple(sys.argv[i + 1].split('=', 1)) for i, a in enumerate(sys.argv) if a == '--rename']
renamed = {}
def load(path, parent=False):
    t = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', open(path).read())
    for pat, rep in (RENAMES if parent else []):
        for m in re.finditer(r'[\w$.]*(?:' + pat + r')[\w$.]*', t):
            renamed.setdefault(m.group(0), re.sub(pat, rep, m.group(0)))
        t = re.sub(pat, rep, t)
    if STRIP:
        # assembler comments (hipcc writes the names of the IR blocks there: they count the blocks of arms that were never
        # emitted) and the ordinal of the function inside the file in its local labels (.LBB12_3, .Lfunc_end12, .Ltmp..)
        t = re.sub(r'[ \t]*;[^\n]*', '', t)
        t = re.sub(r'\.(LBB|Lfunc_begin|Lfunc_end|LJTI|LCPI)\d+', r'.\1N', t)
    return t
def split(t):
    # text sections per symbol: from "\t.protected\tNAME" / ".globl NAME" up to .Lfunc_end + the .amdhsa_kernel block that follows
    funcs = {}
    closed = set()
    cur = None
    pre = []
    for line in t.split('\n'):
        m = re.match(r'\s*\.section\s+\.text\.([^,\s]+),', line) or re.match(r'\s*\.globl\s+(_ZL\S+)', line)
        if m and m.group(1) in closed: m = None       # (the text section is reopened behind a kernel's descriptor)
        if m:
            cur = m.group(1); funcs.setdefault(cur, [])
        if cur is None: pre.append(line)
        else: funcs[cur].append(line)
        if line.strip() == '.end_amdhsa_kernel': closed.add(cur); cur = None      # what follows a kernel's descriptor belongs to no kernel
    return pre, funcs
def meta(t):
    # amdhsa.kernels metadata entries keyed by .name
    i = t.find('amdhsa.kernels:')
    j = t.find('amdhsa.target:')
    body = t[i:j]
    ents = re.split(r'\n  - \.', '\n' + body.split('\n', 1)[1])
    d = {}
    for e in ents[1:]:
        m = re.search(r'\.name:\s+(\S+)', e)
        if m:
            d[m.group(1)] = e
    return d
ok = True
for pa in sorted(glob.glob(os.path.join(sys.argv[1], '*-hip-amdgcn-amd-amdhsa-gfx950.s'))):
    name = os.path.basename(pa)
    ra = os.path.join(sys.argv[2], name)
    if not os.path.exists(ra): print(name, 'MISSING in result'); ok = False; continue
    a, b = load(pa, True), load(ra)
    short = name.split('-hip-')[0]
    if a == b:
        print(f'{short}: identical ({len(a.splitlines())} lines)'); continue
    pa_, fa = split(a); pb_, fb = split(b)
    ma, mb = meta(a), meta(b)
    removed = sorted(set(fa) - set(fb)); added = sorted(set(fb) - set(fa))
    diff = [k for k in fa if k in fb and fa[k] != fb[k]]
    mdiff = [k for k in ma if k in mb and ma[k] != mb[k]]
    print(f'{short}: {len(fa)} symbols in parent, {len(fb)} in result; removed {len(removed)}, added {len(added)}, '
          f'bodies differing {len(diff)}, metadata differing {len(mdiff)}, text outside kernels {"identical" if pa_ == pb_ else "differs (symbol tables and metadata of the removed kernels)" if removed else "DIFFERS"}')
    for k in removed: print('   removed:', k)
    for k in added: print('   ADDED:', k); ok = False
    for k in diff: print('   BODY DIFFERS:', k); ok = False
    for k in mdiff: print('   METADATA DIFFERS:', k); ok = False
    if pa_ != pb_ and not removed: ok = False
for old in sorted(k for k in renamed if k.startswith('_Z') and '.' not in k): print('renamed:', old, '->', renamed[old])
sys.exit(0 if ok else 1)
