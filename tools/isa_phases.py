"""Static instruction counts per solver phase (tool, not shipped).

Counts the instructions of each kernel's solve16 between the `; PHASE_MARK k`
comments that a -DBB_ISA_MARKS build leaves in the assembly (bb_solve.h: PH).
Static counts: a loop body counts once, so the line-search loop (phase 9) is
one evaluation and the contact loops one round.  The last column, read-wait,
counts the waits on a just-issued LDS read: an `s_waitcnt lgkmcnt(0)` within
three instructions after a `ds_read*`.  Two more columns count the exec-mask
control flow: xbr, the `s_cbranch_exec*` instructions, and short, the bodies of
at most 45 instructions that an `s_cbranch_execz` skips forward over (the code
between the branch and its target), attributed to the branch's phase.  The last two,
agpr-rd and addr-reload, count the `v_accvgpr_read_b32` and those of them whose
destination is the address operand of a `ds_*` within the next five instructions:
an LDS address that was parked in an AGPR and is brought back for one access.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -DBB_ISA_MARKS -I openballbot-rl_amd/csrc \
      --cuda-device-only -S -o /tmp/bbk.s openballbot-rl_amd/csrc/bb_kernels.hip
  python tools/isa_phases.py /tmp/bbk.s

With --pre the second mark family is counted instead: the `; PRE_MARK k` comments of bb_step.h
(BB_PRE) that cut the whole step outside the Newton loop into sections.  Per kernel (--kernel
SUBSTRING of the mangled name, default the fp64 fast multi-step kernel) and section: all
instructions, VALU, FP64 (v_*_f64), rcp + rsq, v_readlane / v_writelane (SGPR spills) and AGPR
moves (v_accvgpr_*).  A section is the text from its mark to the next mark of either family; the
code before the first mark is the kernel prologue, the solve's PHASE_MARK sections are summed
into "solve".  Where the compiler duplicated a section (both arms of the team-size test, a peeled
loop) the copies add up, so the serial fall-back of the twin forms is listed with them.
Five more columns count the LDS traffic and its waits: ds_read*, ds_write*, s_waitcnt, those of
them that wait for lgkmcnt(0), and read-wait as defined above.  The sections that hold a twin
arm and a serial arm carry sub-marks (`; PRE_MARK k twin|serial|join`, BB_PRE_ARM): under such a
section's row its parts are listed, "head" being the code before the first arm; the twin rows
are what a 16-lane team of the FUSE kernels runs.

  python tools/isa_phases.py --pre /tmp/bbk.s
"""
import re
import sys
from collections import Counter

NAMES = {0: "contact pass", 1: "ground sums", 2: "gradient", 3: "hessian row", 4: "cholesky",
         5: "sweeps", 8: "ls setup", 9: "ls loop", 6: "update", 7: "exit"}


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if "_dpp" in op or op.startswith("v_mov_b32_dpp"):
        return "dpp"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main(path):
    func, marks, counts = None, [], {}
    cur = None
    nins, labels, execz = {}, {}, {}  # per function: instructions so far, label -> index, (phase, index, target)
    since_read = None  # instructions since the last ds_read*, None when there was none in this phase
    pending, pending_phase = [], None  # (destination, age) of the recent v_accvgpr_read in this phase
    for line in open(path):
        m = re.match(r"^(_Z[^:\s]+):", line)
        if m:
            func, cur, since_read = m.group(1), None, None
            nins[func], labels[func], execz[func] = 0, {}, []
            continue
        m = re.search(r"; PHASE_MARK (\d+)", line)
        if m and func:
            cur = int(m.group(1))
            if cur == 7:  # solver exit: the rest of the kernel is not the solve
                cur = None
                continue
            counts.setdefault(func, {}).setdefault(cur, Counter())
            since_read = None
            continue
        s = line.strip()
        m = re.match(r"^(\.L[\w$.]+):", s)
        if m and func:
            labels[func][m.group(1)] = nins[func]
        if func and s and not s.startswith((";", ".")) and not s.endswith(":"):
            nins[func] += 1
        if cur is None or not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        op = s.split()[0]
        counts[func][cur][classify(op)] += 1
        # AGPR reads, and those of them that bring back an LDS address: the destination is the
        # address operand of a ds_* within five instructions
        pending = [(r, n + 1) for r, n in pending if n < 5] if pending_phase == (func, cur) else []
        pending_phase = (func, cur)
        ops = [o.strip() for o in s[len(op):].split(";")[0].split(",")]
        if op.startswith("v_accvgpr_read"):
            counts[func][cur]["agpr"] += 1
            pending.append((ops[0], 0))
        elif op.startswith("ds_") and ops:
            addr = (ops[0] if op.startswith("ds_write") else ops[1] if len(ops) > 1 else "").split()[0:1]
            hit = [p for p in pending if addr and p[0] == addr[0]]
            if hit:
                counts[func][cur]["areload"] += 1
                pending.remove(hit[0])
        if op.startswith("s_cbranch_exec"):
            counts[func][cur]["xbr"] += 1
            if op == "s_cbranch_execz":
                execz[func].append((cur, nins[func], s.split()[1]))
        # a wait for everything outstanding within three instructions of an LDS read's issue: the
        # read's whole latency is exposed (one wave per SIMD has nothing else to run)
        if op.startswith("ds_read"):
            since_read = 0
        elif since_read is not None:
            since_read += 1
            if op == "s_waitcnt" and "lgkmcnt(0)" in s and since_read <= 3:
                counts[func][cur]["rwait"] += 1
    bodies = {}
    for func, brs in execz.items():
        for ph_, idx, target in brs:
            n = labels[func].get(target, -1) - idx  # instructions between the branch and its target
            if 0 <= n <= 45:
                counts[func][ph_]["short"] += 1
                bodies.setdefault(func, {}).setdefault(ph_, []).append(n)
    for func, ph in counts.items():
        print(func[:90])
        tot = Counter()
        order = [10, 0, 1, 2, 3, 4, 5, 8, 9, 6]  # PH(k) ends phase k; code after mark k is the next phase
        for k in order:
            if k not in ph:
                continue
            c = ph[k]
            nxt = {10: "contact pass", 0: "ground sums", 1: "gradient", 2: "hessian row", 3: "cholesky", 4: "sweeps",
                   5: "ls setup", 8: "ls loop", 9: "update", 6: "conv test"}[k]
            tot.update(c)
            print("  after mark %d (%-14s) valu %5d dpp %4d lds %4d vmem %3d salu %4d wait %4d read-wait %3d xbr %3d short %3d "
                  "agpr-rd %3d addr-reload %3d %s" %
                  (k, nxt, c["valu"], c["dpp"], c["lds"], c["vmem"], c["salu"], c["wait"], c["rwait"], c["xbr"], c["short"],
                   c["agpr"], c["areload"], sorted(bodies.get(func, {}).get(k, []))))
        print("  total                        valu %5d dpp %4d lds %4d vmem %3d salu %4d wait %4d read-wait %3d xbr %3d short %3d "
              "agpr-rd %3d addr-reload %3d" %
              (tot["valu"], tot["dpp"], tot["lds"], tot["vmem"], tot["salu"], tot["wait"], tot["rwait"], tot["xbr"], tot["short"],
               tot["agpr"], tot["areload"]))


PRE_NAMES = {0: "kernel prologue", 1: "stage state", 2: "kinematics", 3: "wheel lanes", 4: "mass_finish",
             5: "bias_finish", 6: "collision", 7: "stage out, dense mass, ground setup", 8: "solve",
             9: "after the solve, RK sums", 10: "mj_advance", 11: "obs, reward, termination, stores"}


PRE_COLS = (("all", "all"), ("VALU", "valu"), ("FP64", "fp64"), ("rcp+rsq", "rcp"), ("lane", "lane"), ("AGPR", "agpr"),
            ("ds_read", "dsr"), ("ds_write", "dsw"), ("waitcnt", "wait"), ("lgkm(0)", "lgkm0"), ("read-wait", "rwait"))


def pre_main(path, want):
    func, cur, counts = None, None, {}
    since_read = None  # instructions since the last ds_read*, None when there was none in this part
    for line in open(path):
        m = re.match(r"^(_Z[^:\s]+):", line)
        if m:
            func, cur, since_read = m.group(1), (0, ""), None
            continue
        if func is None or want not in func:
            continue
        m = re.search(r"; PRE_MARK (\d+)(?: (\w+))?", line)
        if m:
            cur, since_read = (int(m.group(1)), m.group(2) or "head"), None
            continue
        m = re.search(r"; PHASE_MARK (\d+)", line)
        if m:
            cur, since_read = ((9 if int(m.group(1)) == 7 else 8), "head"), None  # PH(7): the solver's exit
            continue
        s = line.strip()
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        if s.startswith("s_endpgm"):
            func = None
            continue
        op = s.split()[0]
        c = counts.setdefault(func, {}).setdefault(cur[0], {}).setdefault(cur[1], Counter())
        c["all"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
        if op.startswith("v_") and "_f64" in op:
            c["fp64"] += 1
        if op.startswith(("v_rcp", "v_rsq")):
            c["rcp"] += 1
        if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            c["lane"] += 1
        if op.startswith("v_accvgpr"):
            c["agpr"] += 1
        if op.startswith("ds_write"):
            c["dsw"] += 1
        if op == "s_waitcnt":
            c["wait"] += 1
            if "lgkmcnt(0)" in s:
                c["lgkm0"] += 1
        # read-wait, as in the solver mode: everything outstanding is waited for within three
        # instructions of an LDS read's issue
        if op.startswith("ds_read"):
            c["dsr"] += 1
            since_read = 0
        elif since_read is not None:
            since_read += 1
            if op == "s_waitcnt" and "lgkmcnt(0)" in s and since_read <= 3:
                c["rwait"] += 1
    fmt = "  %-38s" + " %9s" * len(PRE_COLS)
    for func, secs in counts.items():
        print(func[:100])
        print(fmt % (("section",) + tuple(h for h, _ in PRE_COLS)))
        tot = Counter()
        for k in sorted(secs):
            c = Counter()
            for part in secs[k].values():
                c.update(part)
            tot.update(c)
            print(fmt % ((PRE_NAMES.get(k, str(k)),) + tuple(c[f] for _, f in PRE_COLS)))
            if len(secs[k]) > 1:
                for arm in ("head", "twin", "serial", "join"):
                    if arm in secs[k]:
                        print(fmt % (("    " + arm,) + tuple(secs[k][arm][f] for _, f in PRE_COLS)))
        print(fmt % (("total",) + tuple(tot[f] for _, f in PRE_COLS)))


if __name__ == "__main__":
    if "--pre" in sys.argv:
        args = [a for a in sys.argv[1:] if a != "--pre"]
        kern = "multi_step_kernelIdLb0E"
        if "--kernel" in args:
            i = args.index("--kernel")
            kern = args[i + 1]
            del args[i:i + 2]
        pre_main(args[0], kern)
    else:
        main(sys.argv[1])
