#!/usr/bin/env python3
"""Per-symbol comparison of two device assembly listings of one translation unit, for changes that must leave the device
code alone.  Make the listings with the Makefile's flags plus -S --cuda-device-only, at the parent and at the head:
  hipcc $(HIPFLAGS) -S --cuda-device-only -o parent.s sequencer.hip      (in a checkout of the parent)
  hipcc $(HIPFLAGS) -S --cuda-device-only -o head.s sequencer.hip
  tools/compare_device_code.py parent.s head.s
Ignored: .file / .loc / .ident lines (they follow the host text), the order of the symbols and with it the function
number in local labels (.LBB<n>_<m>, .Lfunc_end<n>), and the one-byte __hip_cuid_<hash of the source> object that hipcc
adds to every translation unit; with the function number, the padding between a local label and its comment (the
comment column is fixed, the label's length is not); where the .AMDGPU.gpr_maximums trailer of the last function and the
trailer of the metadata note sit, which is behind whichever symbol comes last: they are compared as "(gpr maximums)" and
with the head of "(metadata)".  A symbol is the text from the directives in front of its .type line to the next symbol's, so a kernel's descriptor
(.amdhsa_kernel) is compared with its code; the metadata note behind the last symbol is compared as "(metadata)", its
per-kernel entries in sorted order.  Exit status 0: identical."""
import re
import sys

TYPE = re.compile(r"\s*\.type\s+([^,\s]+),@(function|object)")
SKIP = re.compile(r"\s*\.(file|loc|ident)\s")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
FUNC_NO = re.compile(r"(BB|\.Lfunc_end|\.Lfunc_begin)\d+")
LABEL_PAD = re.compile(r"^(\.LBB_\d+:)\s+;")


def symbols(path):
    """{symbol: [normalised lines]} and the number of kernels."""
    out, name, kernels = {}, "(preamble)", 0
    for line in open(path):
        if SKIP.match(line):
            continue
        m = TYPE.match(line)
        if m:  # the directives in front of the .type line (.section, .globl, .p2align ...) belong to the new symbol
            prev, name = out.get(name, []), m.group(1)
            while prev and prev[-1].lstrip().startswith((".section", ".globl", ".p2align", ".protected", ".weak", ".hidden")):
                out.setdefault(name, []).insert(0, prev.pop())
        elif line.lstrip().startswith(".amdgpu_metadata"):
            name = "(metadata)"
        elif ".AMDGPU.gpr_maximums" in line:
            name = "(gpr maximums)"
        kernels += line.lstrip().startswith(".amdhsa_kernel ")
        out.setdefault(name, []).append(LABEL_PAD.sub(r"\1 ;", FUNC_NO.sub(r"\1", CUID.sub("__hip_cuid_", line.rstrip()))))
    cuid = [s for s in out if s.startswith("__hip_cuid_")]
    for s in cuid:
        # the lines behind the object (section changes, the metadata's lead-in) stay in the comparison
        out["(after cuid)"] = [l for l in out.pop(s) if "__hip_cuid_" not in l and not l.lstrip().startswith((".byte", ".size", ".p2align"))]
    note, _, trailer = "\n".join(out.get("(metadata)", [])).partition("\namdhsa.target:")
    entries = note.split("\n  - ")  # one entry per kernel, in symbol order
    out["(metadata)"] = entries[:1] + [trailer] + sorted(entries[1:])
    return out, kernels


def main():
    (a, ka), (b, kb) = symbols(sys.argv[1]), symbols(sys.argv[2])
    named = lambda d: [s for s in d if not s.startswith("(")]
    differ = sorted(s for s in a.keys() & b.keys() if a[s] != b[s])
    print("symbols: parent %d, head %d" % (len(named(a)), len(named(b))))
    print("only in parent:", sorted(a.keys() - b.keys()))
    print("only in head:", sorted(b.keys() - a.keys()))
    print("text differs:", differ)
    kernel = lambda entry: re.search(r"\.name:\s+(\S+)", entry).group(1) if ".name:" in entry else entry[:40]
    ma, mb = a["(metadata)"], b["(metadata)"]
    print("metadata entries only in parent:", sorted(kernel(e) for e in set(ma) - set(mb)))
    print("metadata entries only in head:", sorted(kernel(e) for e in set(mb) - set(ma)))
    print("lines compared: %d" % sum(len(v) for v in a.values()))
    print("kernels (.amdhsa_kernel): parent %d, head %d" % (ka, kb))
    same = not differ and a.keys() == b.keys() and ka == kb
    print("VERDICT:", "identical" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
