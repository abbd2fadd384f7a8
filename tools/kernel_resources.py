"""Per-kernel resource table from the compiler's resource-usage remarks.

Compile one source for the device with the build's flags plus

    --cuda-device-only -Rpass-analysis=kernel-resource-usage

(no GPU needed), keep stderr in a file, then

    python tools/kernel_resources.py remarks.log [name-substring ...]

prints one markdown row per kernel whose name contains one of the
substrings: VGPRs, AGPRs, SGPRs, scratch bytes per lane, waves per SIMD
and LDS bytes per block.  docs/KERNELS.md holds the committed tables.
"""
import os
import re
import subprocess
import sys

FIELDS = [('VGPRs', r'\bVGPRs: (\d+)'), ('AGPRs', r'\bAGPRs: (\d+)'),
          ('SGPRs', r'TotalSGPRs: (\d+)'),
          ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
          ('waves/SIMD', r'Occupancy \[waves/SIMD\]: (\d+)'),
          ('LDS', r'LDS Size \[bytes/block\]: (\d+)')]


def demangle(name):
    out = name
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for tool in ('c++filt', 'llvm-cxxfilt',
                 os.path.join(rocm, 'llvm', 'bin', 'llvm-cxxfilt')):
        try:
            out = subprocess.run([tool, name], capture_output=True,
                                 text=True, check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            continue
        if out != name:
            break
    if out == name:
        # names the demanglers give up on (a template argument that
        # refers to another): kernel name and its literal arguments
        m = re.match(r'_ZN12_GLOBAL__N_1(\d+)', name)
        if m:
            rest = name[m.end():]
            ident, rest = rest[:int(m.group(1))], rest[int(m.group(1)):]
            lits = re.match(r'I((?:L[a-z]\d+E)+)E', rest)
            args = re.findall(r'L[a-z](\d+)E', lits.group(1)) if lits else []
            return ident + ('<' + ', '.join(args) + '>' if args else '')
    out = re.sub(r'\(anonymous namespace\)::', '', out)
    out = re.sub(r'^void ', '', out)
    depth = 0
    for i, ch in enumerate(out):   # cut the argument list, keep <...>
        depth += ch == '<'
        depth -= ch == '>'
        if ch == '(' and depth == 0:
            return out[:i]
    return out


def main():
    text = open(sys.argv[1]).read()
    wanted = sys.argv[2:]
    print('| kernel | ' + ' | '.join(f for f, _ in FIELDS) + ' |')
    print('|---|' + '---|' * len(FIELDS))
    for block in re.split(r'remark: Function Name: ', text)[1:]:
        mangled = block.split()[0]
        name = demangle(mangled)
        if wanted and not any(w in name for w in wanted):
            continue
        vals = [re.search(pat, block) for _, pat in FIELDS]
        print(f'| `{name}` | '
              + ' | '.join(m.group(1) if m else '?' for m in vals) + ' |')


if __name__ == '__main__':
    main()
