"""The conditions DESIGN.md section 3.1 sets on the tracking kernels, checked on the compiler's ISA (no GPU needed):

    hipcc <the Makefile's flags for kernels_hot.hip> --cuda-device-only -S kernels_hot.hip -o hot.s
    python tools/track_isa_check.py hot.s [baseline.s]

For every kernel of the file: its loops (a backward branch to a label), innermost first, with their instruction counts and the number
of v_accvgpr_* instructions inside.  The iteration loop of a chain kernel is its largest loop without a memory instruction; a tracking
kernel must have none of the parked values' moves in it, and no scratch memory.  With a second file (the same translation unit built from
the parent commit) it also reports whether every kernel both files have is the same instruction stream, and lists the kernels only one
of the two files has: a difference of either sort fails the check."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name and line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if name is not None:
            body.append(line.rstrip("\n"))
    return out


def instructions(body):
    """[(label or None, text)] without directives and comments."""
    res = []
    for l in body:
        s = l.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", s)
            if m:
                res.append((m.group(1), None))
            continue
        res.append((None, s))
    return res


def loops(ins):
    pos, n = {}, 0
    idx = []
    for lab, text in ins:
        if lab:
            pos[lab] = n
        else:
            idx.append(text)
            n += 1
    found, n = [], 0
    for lab, text in ins:
        if lab:
            continue
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", text)
        if m:
            t = m.group(1) or m.group(2)
            if t in pos and pos[t] <= n:
                seg = idx[pos[t]:n + 1]
                found.append((pos[t], n, len(seg), sum(1 for x in seg if x.startswith("v_accvgpr")), sum(1 for x in seg if x.startswith("global_"))))
        n += 1
    return sorted(found, key=lambda f: f[2]), idx


JOBS = {"i": "track", "MultistartArgs": "multistart", "SolutionsArgs": "solutions", "LineArgs": "line", "GoalsetArgs": "goalset", "PathArgs": "path",
        "PickArgs": "pick", "PathMultistartArgs": "path_multistart"}


def job_of(name):
    """The chain job of an overload of dls_chain_job_kernel / dls_chain_hot_job_kernel, from the type of its last parameter (the job's
    tail argument, kernels.hpp IKGPU_CHAIN_JOBS): `i` for the tracking kernel's T, else ikdev::<Job>Args.  None for every other kernel."""
    m = re.search(r"job_kernelI.*(?:ChainKernelArgsIXT_EEE|HotTableE)(i|NS\d+_\d+(\w+Args)E)$", name)
    return JOBS.get(m.group(2) or m.group(1)) if m else None


def short(name):
    m = re.search(r"\d+(dls_chain\w+?kernel)ILi(\d)", name)
    tail = "never-stop" if "ELb1EEEv" in name else "stop rule" if "ELb0EEEv" in name else ""
    kernel = m.group(1).replace("job", job_of(name)) if m and job_of(name) else m.group(1) if m else None
    return "%s<NJ=%s> %s" % (kernel, m.group(2), tail) if m else name


def main():
    new = functions(sys.argv[1])
    base = functions(sys.argv[2]) if len(sys.argv) > 2 else {}
    bad = 0
    for name, body in new.items():
        if "kernel" not in name:
            continue
        ls, idx = loops(instructions(body))
        # the iteration loop touches no memory (the pass-through loops and a tracking kernel's waypoint loop do): the largest such loop;
        # a refill kernel's loop stores finished lanes, there the largest loop is reported
        inner = ls[-1:] if "refill" in name else [l for l in reversed(ls) if l[4] == 0][:1]
        total_acc = sum(1 for x in idx if x.startswith("v_accvgpr"))
        scratch = sum(1 for x in idx if x.startswith("scratch_"))
        line = "%-48s %6d instructions, v_accvgpr_* %3d, scratch_* %d" % (short(name), len(idx), total_acc, scratch)
        if inner:
            line += " | iteration loop %5d instructions, v_accvgpr_* inside %d" % (inner[0][2], inner[0][3])
            if "hot_job_kernel" in name and job_of(name) == "track" and (inner[0][3] or scratch):   # (the conditions are the hot builds': some general ones spill SGPRs)
                bad += 1
        if name in base:
            # (a label carries the kernel's position in its file, .LBB<position>_<block>: the position is not part of the stream)
            mine, theirs = ([re.sub(r"\.LBB\d+_", ".LBB_", x) for x in i] for i in (idx, loops(instructions(base[name]))[1]))
            line += " | parent: %s" % ("same instruction stream" if mine == theirs else "DIFFERENT (%d instructions)" % len(theirs))
            bad += mine != theirs
        print(line)
    if len(sys.argv) > 2:   # ... and the two files must hold the same kernels
        mine, theirs = ({n for n in fs if "kernel" in n} for fs in (new, base))
        for n in sorted(mine ^ theirs):
            print("%-48s only in %s" % (short(n), sys.argv[1] if n in mine else sys.argv[2]))
        print("kernels: %d here, %d in the parent, %d in one file only" % (len(mine), len(theirs), len(mine ^ theirs)))
        bad += len(mine ^ theirs)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
