"""Developer tool: do the kernels of a translation unit keep their gfx950 code?  Compares the instruction lists of every kernel that appears
in either of two device-assembly listings (of cfd_sample.hip: the instances of begin_step_kernel, inpaint_now_kernel and cfg_step_kernel and
the small kernels next to them), labels and comments aside, each under its own demangled name; a kernel in one listing only is MISSING.
A new trailing template parameter with a default changes an instance's name, not its code: --rename OLD=NEW (repeatable) maps a part of
a name before onto its spelling after, e.g. --rename "begin_step_kernel<0, true, false>(=begin_step_kernel<0, true, false, false>(".

Make a listing (in convofusion_amd/csrc/ of each tree):
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC --cuda-device-only -S -DCFD_SOURCE_HASH='"x"' cfd_sample.hip -o X.s

Usage:  python tools/isa_same.py [--rename OLD=NEW ...] BEFORE.s AFTER.s      (exit status 1 when a kernel differs or is missing)
"""
import argparse
import re
import subprocess
import sys


def functions(path):
    """{demangled kernel name: [instructions]} of an assembly listing (directives, labels and comments dropped; branch targets renamed)."""
    out, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        t = line.split(";")[0].strip()
        if re.match(r"^s_endpgm", t):
            out[cur] = body + ["s_endpgm"]
            cur = None
        elif t and not t.startswith(".") and not t.endswith(":"):
            body.append(re.sub(r"\.LBB\d+_\d+", "LBL", t))
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d: out[k] for k, d in zip(out, names)}


def short(name):
    """A kernel's name without its 'void' and its argument list."""
    return re.sub(r"^void ", "", name).split("(")[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="a part of a kernel's name before, and after")
    ap.add_argument("before")
    ap.add_argument("after")
    a = ap.parse_args()
    before, after = functions(a.before), functions(a.after)
    for r in a.rename:
        old, new = r.split("=", 1)
        before = {k.replace(old, new): v for k, v in before.items()}
    bad = 0
    for name in sorted(set(before) | set(after)):
        if name not in before or name not in after:
            print(f"MISSING {'before' if name not in before else 'after'}: {short(name)}")
            bad += 1
            continue
        same = before[name] == after[name]
        bad += not same
        print(f"{'SAME' if same else 'DIFF'} {len(before[name])} vs {len(after[name])} instructions: {short(name)}")
    print(f"{len(set(before) | set(after))} kernels, {bad} DIFF or MISSING")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
