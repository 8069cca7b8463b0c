"""VGPRs, scratch and waves/SIMD of the library's kernels, from the compiler's resource remarks.

  hipcc <build()'s flags> -Rpass-analysis=kernel-resource-usage pint_amd/csrc/pint_hip.hip -o /tmp/x.so 2> new.txt
  python scripts/diag/kernel_regs.py new.txt [old.txt] [name filter, default k_eval|k_glitch|k_wavex|k_fdjump|k_phase_terms]

With two files: every kernel of either whose name matches, side by side, and whether the figures
are equal (the register gate of a change that must leave the evaluation's builds alone).  k_wavex
is a template since the chromatic components: its plain build, k_wavex<false>, is compared with a
parent's untemplated k_wavex; the chromatic build, k_wavex<true>, is listed as new.  k_fdjump
(FDJump / FDJumpDM) and k_phase_terms (PiecewiseSpindown / Wave / IFunc) are listed as new against a parent
without them; "all" as the filter compares
every kernel of the library.
"""
import re
import subprocess
import sys


def read(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k.split()[0]] = int(v)
    return out


def demangle(names):
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, (re.sub(r"\(.*", "", l) for l in txt.splitlines())))
    except Exception:
        return {n: n for n in names}


if __name__ == "__main__":
    files = [a for a in sys.argv[1:] if a.endswith(".txt")]
    rx = re.compile(([a for a in sys.argv[1:] if not a.endswith(".txt")] or ["k_eval|k_glitch|k_wavex|k_fdjump|k_phase_terms"])[0].replace("all", "."))
    new = read(files[0])
    old = read(files[1]) if len(files) > 1 else None
    names = [n for n in dict.fromkeys(list(new) + list(old or {})) if rx.search(n)]
    pretty = demangle(names)
    if old is not None:  # (the plain build of a kernel that became a template stands for the parent's)
        plain = {re.sub(r"^void |<false>$", "", pretty[n]): n for n in names if n in new and pretty[n].endswith("<false>")}
        for n in list(names):
            if n in old and n not in new and pretty[n] in plain:
                old[plain[pretty[n]]] = old[n]
                names.remove(n)
    fmt = lambda d: "-" if d is None else f"{d['VGPRs']:4d} VGPRs {d['ScratchSize']:4d} B {d['Occupancy']:2d} waves"
    same = True
    for n in names:
        a, b = new.get(n), (old or {}).get(n)
        line = f"{pretty[n][:60]:60s} {fmt(a)}"
        if old is not None:
            line += f" | parent {fmt(b)} {'=' if a == b else ('new' if b is None else 'DIFFERENT')}"
            same = same and (a == b or b is None)
        print(line)
    if old is not None:
        print("all equal to the parent" if same else "NOT equal to the parent")
        sys.exit(0 if same else 1)
