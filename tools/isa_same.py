#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc -S --cuda-device-only) kernel by kernel.

usage:  python tools/isa_same.py OLD.s NEW.s

Prints the kernels that were added, removed or whose text differs and exits 1 on any difference, 0 when the files hold the
same kernels with the same text (hence the same registers, LDS and occupancy: the resource block of a kernel follows its
code).  A refactor of a hand-scheduled unit is done when this says "same".  The only text that is normalised is the
__hip_cuid_<hash> symbol, a hash of the translation unit's source.  Everything outside a function (file header, metadata) is
compared as one more entry, "(module)"."""
import re
import sys

MODULE = "(module)"


def kernels(text):
    """{function symbol: its text up to the next function}, plus the text outside any function under "(module)"."""
    out, cur = {MODULE: []}, MODULE
    for line in re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text).splitlines():
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif "__hip_cuid_" in line or ".amdgpu_metadata" in line:
            cur = MODULE                # the trailer behind the last function
        out[cur].append(line.rstrip())
    return out


def compare(old_text, new_text):
    """Lines of the report; empty when the two files are the same."""
    old, new = kernels(old_text), kernels(new_text)
    rep = ["removed  %s" % k for k in old if k not in new] + ["added    %s" % k for k in new if k not in old]
    for k in old:
        if k in new and old[k] != new[k]:
            n = next((i for i, (a, b) in enumerate(zip(old[k], new[k])) if a != b), min(len(old[k]), len(new[k])))
            rep.append("differs  %s (%d -> %d lines, first at line %d of the kernel)" % (k, len(old[k]), len(new[k]), n + 1))
    return rep


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    with open(argv[1]) as f, open(argv[2]) as g:
        old_text, new_text = f.read(), g.read()
    rep = compare(old_text, new_text)
    print("\n".join(rep) if rep else "same: %d kernels" % (len(kernels(old_text)) - 1))
    return 1 if rep else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
