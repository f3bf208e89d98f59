"""Compares the gfx950 code of named kernels (or, with --all, of every kernel) between two device assembly listings (parent and head of a change that
must leave the hot path alone): per kernel the instruction stream (local labels renumbered by order of appearance, so
that a function's place in the file does not show) and the resource figures of its .amdhsa_kernel block.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -S --offload-device-only <unit>.hip -o <listing>.s
    python scripts/compare_kernel_code.py parent.s head.s k_linearize_numeric k_diag_reduce ...
    python scripts/compare_kernel_code.py --all parent.s head.s
    python scripts/compare_kernel_code.py --all parent.s head.s 'k_new<Policy>=k_old'

--all compares every kernel found in either listing, the read-out twins `k<a, b, true>` included, under its full
demangled name: for a change that must leave the whole unit's device code alone.  A further argument HEAD=PARENT pairs
a kernel the change renamed: head's kernel whose name holds HEAD is compared with the parent's whose name holds PARENT.

Prints a markdown table; exit status 1 if a kernel differs or is missing on either side."""
import hashlib
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    txt = open(path).read()
    body, meta = {}, {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        body[m.group(1)] = m.group(2)
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", txt, re.S | re.M):
        meta[m.group(1)] = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
    return body, meta, txt


def normalise(code):
    lines = []
    for ln in code.split("\n"):
        ln = ln.split(";")[0].rstrip()  # comments carry nothing the hardware runs
        if ln.strip():
            lines.append(ln)
    code = "\n".join(lines)
    seen = {}
    def ren(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")
    return re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", ren, code)


def figures(txt, sym):
    """SGPRs / VGPRs / scratch / occupancy / LDS of the '; Kernel info' comment block that follows the function."""
    i = txt.index(f"\n{sym}:")
    blk = txt[i:txt.index("; COMPUTE_PGM_RSRC2:SCRATCH_EN", i)]
    g = lambda k: re.search(rf"; {k}: (\d+)", blk).group(1)
    return (g("TotalNumVgprs"), g("TotalNumSgprs"), g("ScratchSize"), g("LDSByteSize"), g("Occupancy"),
            re.search(r"; codeLenInByte = (\d+)", blk).group(1))


def short(name):
    """`k<a, b>` of a demangled kernel; a head instantiation `k<a, b, false>` of a template that gained a defaulted
    third parameter is the parent's `k<a, b>` (its `k<a, b, true>` twins are new and not compared)."""
    nm = name.replace("sim3opt::", "").split("(")[0].replace("void ", "")
    return re.sub(r"^(k_linearize_\w+<\w+, \w+), false>$", r"\1>", nm)


def main():
    args = [x for x in sys.argv[1:] if x != "--all"]
    everything = len(args) < len(sys.argv) - 1
    a, b, want = args[0], args[1], args[2:]
    (ba, ma, ta), (bb, mb, tb) = kernels(a), kernels(b)
    # (only what has a .amdhsa_kernel block is a kernel: device functions that were not inlined are left out)
    ba = {s: c for s, c in ba.items() if s in ma}
    bb = {s: c for s, c in bb.items() if s in mb}
    names = demangle(sorted(set(ba) | set(bb)))
    label = (lambda nm: nm.replace("sim3opt::", "").replace("void ", "")) if everything else short
    sa = {label(names[s]): s for s in ba}
    sb = {label(names[s]): s for s in bb}
    for head, parent in (w.split("=") for w in want if "=" in w):
        (h,), (p,) = [n for n in sb if head in n], [n for n in sa if parent in n]
        sa[f"{p} -> {h}"], sb[f"{p} -> {h}"] = sa.pop(p), sb.pop(h)
    bad = 0
    print("| kernel | parent VGPR / SGPR / scratch / LDS / occupancy / code bytes | head | instruction stream |")
    print("|---|---|---|---|")
    for nm in sorted(set(sa) | set(sb)):
        if not everything and (not any(nm == w or nm.startswith(w + "<") for w in want)
                               or re.search(r"<\w+, \w+, true>$", nm)):
            continue
        if nm not in sa or nm not in sb:
            print(f"| `{nm}` | {'missing' if nm not in sa else ''} | {'missing' if nm not in sb else ''} | - |")
            bad += 1
            continue
        fa, fb = figures(ta, sa[nm]), figures(tb, sb[nm])
        na = normalise(ba[sa[nm]]).replace(sa[nm], "SELF")
        nb_ = normalise(bb[sb[nm]]).replace(sb[nm], "SELF")
        same = na == nb_
        bad += (not same) or fa != fb
        h = hashlib.sha256(na.encode()).hexdigest()[:12]
        hb = hashlib.sha256(nb_.encode()).hexdigest()[:12]
        print(f"| `{nm}` | {' / '.join(fa)} | {' / '.join(fb)} | "
              f"{'identical (' + str(na.count(chr(10)) + 1) + ' lines, sha256 ' + h + ')' if same else 'DIFFERENT ' + h + ' ' + hb} |")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
