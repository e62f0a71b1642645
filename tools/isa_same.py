#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc -S --cuda-device-only) kernel by kernel.

usage:  python tools/isa_same.py [--allow-commuted] OLD.s NEW.s

Prints the kernels that were added, removed or whose text differs and exits 1 on any difference, 0 when the files hold the
same kernels with the same text (hence the same registers, LDS and occupancy: the resource block of a kernel follows its
code).  A refactor of a hand-scheduled unit is done when this says "same".  The only text that is normalised is the
__hip_cuid_<hash> symbol, a hash of the translation unit's source.  Everything outside a function (file header, metadata) is
compared as one more entry, "(module)".

Second verdict, "same up to commuted multiplicands": a kernel whose text differs is compared once more with the two
multiplicands (the first two source operands) of every instruction of COMMUTATIVE put in a canonical order, the bits that
op_sel, op_sel_hi, neg_lo and neg_hi hold for those two operands moved along with them.  If that makes the two texts equal --
same line count, same registers, same order, same resource block -- the kernel is reported as "commuted NAME (k lines)" and
computes the same values: a * b and b * a round alike.  Such a kernel still counts as a difference (exit 1) unless
--allow-commuted is given."""
import re
import sys

MODULE = "(module)"
# instructions whose first two source operands commute (the third, the addend of an fma, does not); e32 / e64 encodings only
COMMUTATIVE = ("v_pk_fma_f32", "v_pk_mul_f32", "v_fma_f32", "v_mul_f32")
ARRAY_MODS = {"op_sel": 0, "op_sel_hi": 1, "neg_lo": 0, "neg_hi": 0}      # per-operand bit arrays and their default bit


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


def _operands(text):
    """Split at the commas outside brackets."""
    out, depth, cur = [], 0, ""
    for ch in text:
        depth += ch in "[("
        depth -= ch in "])"
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def canonical(line):
    """The line with the multiplicands of a COMMUTATIVE instruction in sorted order; any other line unchanged."""
    m = re.match(r"\s+(v_\w+?)(_e32|_e64)?\s+(.*)$", line)
    if not m or m.group(1) not in COMMUTATIVE:
        return line
    rest, mods = m.group(3), {}
    for name, bits in re.findall(r"\s(op_sel|op_sel_hi|neg_lo|neg_hi):\[([01,]+)\]", rest):
        mods[name] = bits.split(",")
    rest = re.sub(r"\s(op_sel|op_sel_hi|neg_lo|neg_hi):\[[01,]+\]", "", rest)
    ops = _operands(rest)
    if len(ops) < 3:
        return line
    last, _, tail = ops[-1].partition(" ")          # clamp, omod and the like stay where they are
    ops[-1] = last
    nsrc = len(ops) - 1
    for name, default in ARRAY_MODS.items():        # absent array = all defaults: a swap may make an array appear or vanish
        mods[name] = (mods.get(name, []) + [str(default)] * nsrc)[:nsrc]
    pair = sorted((ops[1 + i], tuple(mods[name][i] for name in ARRAY_MODS)) for i in (0, 1))
    for i in (0, 1):
        ops[1 + i] = pair[i][0]
        for j, name in enumerate(ARRAY_MODS):
            mods[name][i] = pair[i][1][j]
    return "\t%s%s %s %s %s" % (m.group(1), m.group(2) or "", ", ".join(ops), tail.strip(),
                                " ".join("%s:[%s]" % (name, ",".join(mods[name])) for name in ARRAY_MODS))


def compare(old_text, new_text):
    """Lines of the report; empty when the two files are the same."""
    old, new = kernels(old_text), kernels(new_text)
    rep = ["removed  %s" % k for k in old if k not in new] + ["added    %s" % k for k in new if k not in old]
    for k in old:
        if k in new and old[k] != new[k]:
            if [canonical(a) for a in old[k]] == [canonical(b) for b in new[k]]:
                rep.append("commuted %s (%d lines)" % (k, sum(a != b for a, b in zip(old[k], new[k]))))
                continue
            n = next((i for i, (a, b) in enumerate(zip(old[k], new[k])) if a != b), min(len(old[k]), len(new[k])))
            rep.append("differs  %s (%d -> %d lines, first at line %d of the kernel)" % (k, len(old[k]), len(new[k]), n + 1))
    return rep


def main(argv):
    allow = "--allow-commuted" in argv
    argv = [a for a in argv if a != "--allow-commuted"]
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    with open(argv[1]) as f, open(argv[2]) as g:
        old_text, new_text = f.read(), g.read()
    rep = compare(old_text, new_text)
    print("\n".join(rep) if rep else "same: %d kernels" % (len(kernels(old_text)) - 1))
    return 1 if any(not (allow and r.startswith("commuted ")) for r in rep) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
