"""The library's device code as text, for tools/valu_mix.py and tools/kernel_diff.py: ask a tree's Makefile what it compiles and how,
compile a unit to gfx950 assembly with exactly that command (so tool and library cannot drift), cut the assembly into functions."""
import os
import re
import shlex
import subprocess


def csrc_of(tree):
    return os.path.join(tree, "raytracing_engine_amd", "csrc")


def make_var(tree, name):
    """The words of the Makefile's variable `name`."""
    rule = "_print_var: ; @echo $(%s)" % name
    out = subprocess.run(["make", "-s", "-C", csrc_of(tree), "--eval", rule, "_print_var"], check=True, capture_output=True, text=True).stdout
    return out.split()


def compile_command(tree, unit):
    """The compile command of _obj/<unit>.o as make would run it, without its -c / -o and the unit's name."""
    out = subprocess.run(["make", "-C", csrc_of(tree), "-n", "-B", "_obj/%s.o" % unit], check=True, capture_output=True, text=True).stdout
    cmd = shlex.split(next(l for l in out.splitlines() if " -c %s" % unit in l))
    o = cmd.index("-o")
    del cmd[o:o + 2]
    cmd.remove("-c")
    cmd.remove(unit)
    return cmd


def assembly(tree, unit, workdir, src=None):
    """gfx950 assembly of the unit's device code: the library's flags plus --cuda-device-only -S.  src: another file in the unit's place."""
    csrc = csrc_of(tree)
    asm = os.path.join(workdir, unit + ".s")
    subprocess.run(compile_command(tree, unit) + ["-I", csrc, "--cuda-device-only", "-S", src or os.path.join(csrc, unit), "-o", asm], check=True,
                   stderr=subprocess.DEVNULL)
    with open(asm) as f:
        return f.read()


def functions(text):
    """{mangled name: (body lines, .amdhsa_kernel block lines)} of every function in the assembly: the body is the text between the
    function's label and its .Lfunc_end line, without the kernel descriptor block that the compiler puts in between."""
    out, cur, in_block = {}, None, False
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out[m.group(1)] = ([], [])
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            in_block = in_block or line.strip().startswith(".amdhsa_kernel ")
            cur[1 if in_block else 0].append(line)
            in_block = in_block and line.strip() != ".end_amdhsa_kernel"
    return out
