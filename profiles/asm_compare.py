"""Compare the device functions of two `hipcc --cuda-device-only -S` outputs, label numbers and comments normalised: every
kernel of the first must be in the second with the same instructions (exit status 1 otherwise).

    F="-O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -munsafe-fp-atomics --cuda-device-only -S"  # the Makefile's
    git worktree add ../parent HEAD~1                                  # the parent commit's sources and headers
    hipcc $F ../parent/cge.jl_amd/csrc/kernels_fitp.hip -o old.s && hipcc $F cge.jl_amd/csrc/kernels_fitp.hip -o new.s
    python profiles/asm_compare.py old.s new.s
"""
import re, sys


def funcs(path):
    out, cur, buf = {}, None, []
    for l in open(path).read().split('\n'):
        if cur is None:
            m = re.match(r'^(_Z[\w.$]*):', l)
            if m:
                cur, buf = m.group(1), []
            continue
        if l.startswith('.Lfunc_end'):
            out[cur] = '\n'.join(buf)
            cur = None
            continue
        l = re.sub(r'\.(LBB|Ltmp|LJTI|Lcst)\d+(_\d+)?', r'.\1#', l.split(';')[0]).rstrip()
        if l:
            buf.append(l)
    return out


a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
diff = [k for k in a if k in b and a[k] != b[k]]
print(f"{sys.argv[1]}: {len(a)} kernels before, {sum(a[k] == b.get(k) for k in a)} identical, differ: {diff}, "
      f"missing after: {[k for k in a if k not in b]}, new: {[k for k in b if k not in a]}")
sys.exit(1 if diff else 0)
