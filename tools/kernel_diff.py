#!/usr/bin/env python3
"""Is the device code of two source trees the same?   python tools/kernel_diff.py A B

A and B are checkouts of this repository, or exports of a commit (git archive <commit> | tar -x -C <dir>).  Every .hip unit that a
tree's Makefile lists (SRCS) is compiled to gfx950 assembly with that tree's own command for it plus --cuda-device-only -S, and the
functions are compared by mangled name, wherever in a tree they are defined: the text between a function's label and its .Lfunc_end
line with two normalisations - ';' comments removed, and the function's number dropped from its local labels (.LBB<f>_<n>), which
counts the functions of a unit - and a kernel's .amdhsa_kernel block as it is.  Nothing else in the assembly is looked at.
A function that is on one side only is then looked for on the other side under another name - a kernel whose template gained a
parameter keeps its code but not its mangled name: same body, same kernel block once the function's own name is taken out of both.
Such pairs are listed as "identical under another name"; they do not count as differences, what stays unpaired does.
Exit status 0: every function is on both sides exactly once, with the same body and the same kernel block."""
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import hip_asm


def normal(body):
    out = []
    for line in body:
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).rstrip()
        if line:
            out.append(line)
    return out


def tree_functions(tree, workdir):
    """{name: (unit, body, kernel block)} and the names defined in more than one unit."""
    units = [u for u in hip_asm.make_var(tree, "SRCS") if u.endswith(".hip")]
    with ThreadPoolExecutor(8) as pool:
        texts = list(pool.map(lambda u: hip_asm.assembly(tree, u, workdir), units))
    found, twice = {}, []
    for unit, text in zip(units, texts):
        for name, (body, block) in hip_asm.functions(text).items():
            if name in found:
                twice.append((name, found[name][0], unit))
            found[name] = (unit, normal(body), block)
    return found, twice


def nameless(name, entry):
    """A function's body and kernel block with its own name taken out."""
    _, body, block = entry
    return tuple(l.replace(name, "@") for l in body), tuple(l.replace(name, "@") for l in block)


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %s | %s" % (i + 1, x.strip(), y.strip())
    return "line %d: one side ends (%d and %d lines)" % (min(len(a), len(b)) + 1, len(a), len(b))


def main(tree_a, tree_b):
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
        (fa, twice_a), (fb, twice_b) = tree_functions(tree_a, da), tree_functions(tree_b, db)
    same, differ = [], []
    for name in sorted(set(fa) & set(fb)):
        (ua, body_a, block_a), (ub, body_b, block_b) = fa[name], fb[name]
        where = ua if ua == ub else "%s -> %s" % (ua, ub)
        if body_a != body_b:
            differ.append("%s (%s): body, %s" % (name, where, first_difference(body_a, body_b)))
        elif block_a != block_b:
            differ.append("%s (%s): .amdhsa_kernel block, %s" % (name, where, first_difference(block_a, block_b)))
        else:
            same.append((name, where))
    n_a, n_b = len(fa), len(fb)
    # renamed: a function of A that B lacks and a function of B that A lacks, with the same code (each used once)
    left = {}
    for n in sorted(set(fb) - set(fa)):
        left.setdefault(nameless(n, fb[n]), []).append(n)
    renamed = []
    for n in sorted(set(fa) - set(fb)):
        twins = left.get(nameless(n, fa[n]))
        if twins:
            renamed.append((n, twins.pop(0)))
    for na, nb in renamed:
        del fa[na], fb[nb]
    only = ["%s: only in %s (%s)" % (n, t, f[n][0]) for t, f, g in ((tree_a, fa, fb), (tree_b, fb, fa)) for n in sorted(set(f) - set(g))]
    twice = ["%s: in %s and %s of %s" % (n, u1, u2, t) for t, tw in ((tree_a, twice_a), (tree_b, twice_b)) for n, u1, u2 in tw]

    print("A = %s: %d functions;  B = %s: %d functions" % (tree_a, n_a, tree_b, n_b))
    print("identical (body and kernel block): %d" % len(same))
    for where in sorted(set(w for _, w in same)):
        print("    %-40s %d" % (where, sum(1 for _, w in same if w == where)))
    print("identical under another name: %d" % len(renamed))
    for na, nb in renamed:
        print("    %s\n        -> %s" % (na, nb))
    for title, rows in (("differ", differ), ("on one side only", only), ("defined in more than one unit", twice)):
        print("%s: %d" % (title, len(rows)))
        for row in rows:
            print("    " + row)
    return 1 if differ or only or twice else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
