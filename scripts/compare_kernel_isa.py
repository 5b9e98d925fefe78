"""Do two source trees compile to the same gfx950 kernels?  Compiles every gem_amd/csrc/*.hip of both with build.py's flags plus
`--cuda-device-only -S` and compares kernel by kernel: a sha256 of the instruction stream and the VGPR / SGPR / scratch / LDS figures.  A kernel may
change unit between the trees; local labels are renumbered per function and the per-unit `__hip_cuid` bookkeeping is left out, nothing else.
It compares digests and resource numbers only -- no assembly text is kept.  One line per kernel in --out; hipcub's identical instantiations as one digest.

    python scripts/compare_kernel_isa.py <parent checkout> [<branch checkout, default: this tree>] [--out profiles/n2v_split_isa.json]

A kernel missing by name in one tree whose digest and figures equal those of a kernel missing by name in the other is listed as `renamed` and does
not count as different.  Exit status 1 when a kernel of the parent is missing from the branch or differs.  Needs hipcc, no GPU.  profiles/n2v_split_isa.json was made this way."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gem_amd import build  # noqa: E402

RES = {'.vgpr_count': 'vgpr', '.sgpr_count': 'sgpr', '.private_segment_fixed_size': 'scratch', '.group_segment_fixed_size': 'lds',
       '.vgpr_spill_count': 'vgpr_spills', '.sgpr_spill_count': 'sgpr_spills'}


def unit_kernels(src, workdir):
    """{kernel symbol: {'sha256', 'lines', 'unit', resources...}} of one .hip unit."""
    asm = os.path.join(workdir, os.path.basename(src) + '.s')
    subprocess.check_call([build.HIPCC] + build.CFLAGS + ['--cuda-device-only', '-S', src, '-o', asm])
    text = open(asm).read().split('\n')
    kernels = {m.group(1) for line in text for m in [re.match(r'\s*\.amdhsa_kernel\s+(\S+)', line)] if m}
    out, name, body = {}, None, None
    for line in text:
        m = re.match(r'([A-Za-z_$][\w$.]*):', line)
        if m and m.group(1) in kernels and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r'\.Lfunc_end\d+:', line):
            out[name] = {'sha256': hashlib.sha256('\n'.join(body).encode()).hexdigest(), 'lines': len(body), 'unit': os.path.basename(src)}
            name = None
            continue
        line = line.split(';')[0].strip()                    # comments carry no instruction
        if not line or line.startswith(('.p2align', '.cfi_', '.loc', '.file')):
            continue
        line = line.replace(name, '<this kernel>')           # (its .amdhsa_kernel block and section name: a renamed kernel keeps its digest)
        body.append(re.sub(r'\.L(BB|tmp|func_begin|JTI)\d+_?', r'.L\1_', line))     # function-local labels are numbered by position in the unit
    cur = None
    for line in text:                                        # amdhsa.kernels metadata: one `.name:` per kernel, its figures around it
        m = re.match(r'\s*-?\s*(\.[a-z_]+):\s*(\S+)', line)
        if not m:
            continue
        if line.lstrip().startswith('- '):
            cur = {}
        if cur is None:
            continue
        if m.group(1) in RES:
            cur[RES[m.group(1)]] = int(m.group(2))
        if m.group(1) == '.name' and m.group(2) in out:
            out[m.group(2)]['res'] = cur
    for k, v in out.items():
        v.update(v.pop('res'))
    return out


def tree_kernels(root):
    csrc = os.path.join(root, 'gem_amd', 'csrc')
    srcs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.hip'))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        maps = list(pool.map(lambda s: unit_kernels(s, tmp), srcs))
    allk = {}
    for m in maps:
        for k, v in m.items():
            assert k not in allk, 'kernel %s in two units' % k
            allk[k] = v
    return allk


FIELDS = ('sha256', 'lines', 'vgpr', 'sgpr', 'scratch', 'lds', 'vgpr_spills', 'sgpr_spills')


def is_library(name):
    return name.startswith('_ZN7rocprim')                   # hipcub's sort: one instantiation per target architecture it knows, none of the project's text


def match_renamed(parent, branch, row):
    """{parent name: branch name} of kernels that changed name only: missing by name on either side, with equal digest and resource figures.
    Kernels that share those figures (the same body under several names) are paired in sorted order."""
    gone, new = {}, {}
    for side, other, out in ((parent, branch, gone), (branch, parent, new)):
        for k in sorted(set(side) - set(other)):
            out.setdefault(json.dumps(row(side[k])), []).append(k)
    return {p: b for key in gone for p, b in zip(gone[key], new.get(key, []))}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    if out:
        args.remove(out)
    parent, branch = tree_kernels(args[0]), tree_kernels(args[1] if len(args) > 1 else ROOT)
    row = lambda k: None if k is None else [k[f] for f in FIELDS]
    rows, bad, lib = {}, [], {'parent': hashlib.sha256(), 'branch': hashlib.sha256(), 'count': 0}
    renamed = match_renamed(parent, branch, row)
    for k in sorted(set(parent) | set(branch)):
        if k in renamed or k in renamed.values():
            continue
        p, b = parent.get(k), branch.get(k)
        same = p is not None and row(p) == row(b)
        if p is not None and not same:
            bad.append(k)
        if is_library(k) and same:                           # (compared one by one like the others; recorded as one digest over all of them)
            lib['count'] += 1
            for side, v in (('parent', p), ('branch', b)):
                lib[side].update((k + json.dumps(row(v))).encode())
        elif same:
            rows[k] = row(p) + [p['unit'], b['unit']]
        else:
            rows[k] = {'parent': row(p) and row(p) + [p['unit']], 'branch': row(b) and row(b) + [b['unit']]}
    moved = sorted(k for k in parent if k in branch and parent[k]['unit'] != branch[k]['unit'] and not is_library(k))
    summary = {'kernels_parent': len(parent), 'kernels_branch': len(branch), 'identical': len(parent) - len(bad) - len(renamed), 'changed_unit': moved,
               'renamed': [{'parent': p, 'branch': b, 'figures': row(parent[p])} for p, b in sorted(renamed.items())],
               'missing_or_different': bad, 'only_in_branch': sorted(set(branch) - set(parent) - set(renamed.values())),
               'library_kernels_identical': {'count': lib['count'], 'sha256_over_all_parent': lib['parent'].hexdigest(), 'sha256_over_all_branch': lib['branch'].hexdigest()}}
    if out:
        with open(out, 'w') as f:
            f.write('{"flags": %s,\n "summary": %s,\n "columns": %s,\n "kernels": {\n' % (json.dumps(build.CFLAGS + ['--cuda-device-only', '-S']), json.dumps(summary, indent=1),
                                                                                       json.dumps(list(FIELDS) + ['unit in parent', 'unit in branch'])))
            f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in rows.items()) + '\n }\n}\n')
    print(json.dumps(summary, indent=1))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
