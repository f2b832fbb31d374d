"""Compares two builds' device code kernel by kernel: the check that a change moved or rewrote
only host code.  Make each side's assembly with the Makefile's flags,
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S \
      zstd-decompressor_amd/csrc/zd_kernels.hip -o SIDE.s
then: python scripts/device_asm_diff.py PARENT.s CHANGE.s
Prints the kernels of each side, how many bodies and descriptors are identical as they stand, how
many only once the function number in block labels (.LBB<n>_<m>, and BB<n>_<m> in the loop comments)
is left out -- the compiler renumbers them when host code makes it emit template instantiations in
another order -- and names every kernel that differs.  Exit status 1 if one does."""
import re
import sys


def kernels(path):
    L = open(path).read().split("\n")
    body, desc = {}, {}
    for i, l in enumerate(L):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            n = m.group(1)
            a = next(k for k, x in enumerate(L) if x.startswith(n + ":"))
            body[n] = L[a:next(k for k in range(a, len(L)) if L[k].startswith(".Lfunc_end"))]
            desc[n] = L[i:next(k for k in range(i, len(L)) if ".end_amdhsa_kernel" in L[k]) + 1]
    return body, desc, L


def norm(lines):
    return [re.sub(r"BB\d+_(\d+)", r"BB_\1", l) for l in lines]


def rest(L):   # the whole file but the unit's id (a hash of its text), file names and function numbers
    L = [re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", l) for l in L if not l.lstrip().startswith(".file")]
    return sorted(re.sub(r"(func_begin|func_end)\d+", r"\1", l) for l in norm(L))


A, DA, LA = kernels(sys.argv[1])
B, DB, LB = kernels(sys.argv[2])
print(f"kernels: {len(A)} / {len(B)}; same set: {set(A) == set(B)}; same order: {list(A) == list(B)}")
same = [n for n in A if n in B and A[n] == B[n]]
label = [n for n in A if n in B and A[n] != B[n] and norm(A[n]) == norm(B[n])]
bad = [n for n in A if n not in B or norm(A[n]) != norm(B[n])] + [n for n in B if n not in A]
print(f"bodies identical as they stand: {len(same)}; after leaving out block-label function numbers: {len(label)}; "
      f"differing: {len(bad)}")
for n in label:
    print("  labels only:", n)
for n in bad:
    print("  DIFFERS:", n)
print("kernel descriptors equal:", all(DA[n] == DB.get(n) for n in DA))
print("every other line of the two files equal (as a multiset):", rest(LA) == rest(LB))
sys.exit(1 if bad or set(A) != set(B) else 0)
