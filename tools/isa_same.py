"""Developer tool: do the loop's existing kernel instances keep their gfx950 code?  Compares the instruction lists of begin_step_kernel,
inpaint_now_kernel and cfg_step_kernel (default / edit / anchored / weighted / trajectory instances) in two device-assembly listings of cfd_sample.hip, labels and
comments aside.  A new trailing template parameter with a default changes an instance's name, not its code: the pairs below map the
old names onto the new ones.

Make a listing (in convofusion_amd/csrc/ of each tree):
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC --cuda-device-only -S -DCFD_SOURCE_HASH='"x"' cfd_sample.hip -o X.s

Usage:  python tools/isa_same.py BEFORE.s AFTER.s      (exit status 1 when an instance differs or is missing)
"""
import re
import subprocess
import sys

# (name before, name after): the instances as the parent commit names them and as the tied instances' commit does (begin_step_kernel and
# inpaint_now_kernel got a fourth parameter; the other kernels keep their names)
PAIRS = [("begin_step_kernel<0, false, false>(", "begin_step_kernel<0, false, false, false>("),
         ("begin_step_kernel<0, true, false>(", "begin_step_kernel<0, true, false, false>("),
         ("begin_step_kernel<0, false, true>(", "begin_step_kernel<0, false, true, false>("),
         ("inpaint_now_kernel<0, false, false>(", "inpaint_now_kernel<0, false, false, false>("),
         ("inpaint_now_kernel<0, true, false>(", "inpaint_now_kernel<0, true, false, false>("),
         ("inpaint_now_kernel<0, false, true>(", "inpaint_now_kernel<0, false, true, false>("),
         ("cfg_step_kernel<0, false, false>(", "cfg_step_kernel<0, false, false>("),
         ("cfg_step_kernel<0, true, false>(", "cfg_step_kernel<0, true, false>("),
         ("cfg_step_kernel<0, false, true>(", "cfg_step_kernel<0, false, true>("),
         ("cfg_step_kernel<0, true, true>(", "cfg_step_kernel<0, true, true>("),
         ("edit_init_kernel<0>(", "edit_init_kernel<0>("),
         ("sched_step_kernel<0>(", "sched_step_kernel<0>(")]


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


def main():
    before, after = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for old, new in PAIRS:
        a = [k for k in before if old in k]
        b = [k for k in after if new in k]
        if len(a) != 1 or len(b) != 1:
            print(f"MISSING {old[:-1]} / {new[:-1]}")
            bad += 1
            continue
        same = before[a[0]] == after[b[0]]
        bad += not same
        print(f"{'SAME' if same else 'DIFF'} {len(before[a[0]])} vs {len(after[b[0]])} instructions: {old[:-1]} -> {new[:-1]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
