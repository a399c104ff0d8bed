#!/usr/bin/env python3
"""Per-trellis-step instruction budget of the headline Viterbi kernel, read from the code object the in-tree build produced.

    python scripts/viterbi_step_budget.py [--kernel "viterbi_cw_fused_kernel<6, 109u, 79u, 1, 28, false, double, 32, true>"] [--md out.md]

Disassembles commpy_amd/csrc/build/viterbi_cw.o (device part, gfx950), finds the kernel's step loop (the smallest backward branch that spans
a whole trellis step), counts the steps of one trip of it by the equality compares per step it contains (16 v_cmp_eq_u32, the row and
column hits of the 32-bit first-argmin; 64 v_cmp_eq_f64 of the first-equal scan where that is not compiled in) and sorts every instruction of the
loop body into the phases of cw_step (csrc/viterbi_cw.hip) by opcode -- the table of DESIGN.md 4.1.  The float64 minimum tree and
first-equal scan that 'soft' keeps as the fallback of the 32-bit first-argmin are compiled out of line, behind the loop (the branch
to them is marked unlikely): the loop body counted here is what a step executes when no lane of the wave ties.

Two more tables:
* the same instructions BY POSITION in the step.  The fused kernel pins the four batches of traceback LDS reads between the phases of
  cw_step (WalkHook::at, sched_barrier), and a step ends with the byte it stores into the output tile, so the read batches cut a step
  into: LLR -> branch metrics | butterflies, first half | second half | minimum tree | first-equal scan and the step's tail.  The
  traceback's own instructions (hops, LDS, waits for LDS) are listed apart wherever they sit.  An opcode table cannot tell the
  v_add_f64 of exp / log from those of the add-compare-select; this one can.  A kernel with the 32-bit first-argmin is cut at the
  compares every step has instead (position_table): where a group's walks run in one burst, five steps of six have no reads.
* the code of a 96-step chunk OUTSIDE the hot loop: the loop around it (chunk set-up, the pending walk of the last chunk) and, inside
  that, the rounds of the output flush (eight codewords each, eight rounds per flush), as static instruction counts."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
DEFAULT = "viterbi_cw_fused_kernel<6, 109u, 79u, 1, 28, false, double, 32, true>"


def disassemble(obj):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co], check=True)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    return subprocess.run(["c++filt"], input=dis, capture_output=True, text=True).stdout


def kernel_body(dis, name):
    out, on = [], False
    for line in dis.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
        if m:
            on = name in m.group(2)
            continue
        if on:
            m = re.match(r"^\s+(\S+)\s+(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line)
            if m:
                out.append((int(m.group(3), 16), re.sub(r"_(e32|e64|sdwa|dpp)$", "", m.group(1)), m.group(2) + " //" + m.group(4)))
    return out


ARGMIN32 = "first-argmin on the high dwords: v_min3_u32 row and column minima, v_cmp_eq_u32 + v_addc_co_u32 hit word, index, tie test"


def classify(op, args, prev=None):
    # (only in a kernel that has the 32-bit first-argmin compiled in, main(): elsewhere these opcodes belong to the traceback)
    if EQ[0] == "v_cmp_eq_u32" and (
            op in ("v_min3_u32", "v_min_u32", "v_cmp_eq_u32", "v_ffbl_b32", "v_bcnt_u32_b32", "v_cmp_ne_u32") or
            (prev == "v_cmp_eq_u32" and (op.startswith("v_addc_co") or op == "v_cndmask_b32")) or
            (prev == "v_ffbl_b32" and op == "v_lshrrev_b32") or (prev in ("v_cmp_ne_u32", "v_ffbl_b32") and op == "v_lshl_or_b32")):
        return ARGMIN32
    if op in ("v_add_f64",):
        return "add-compare-select: v_add_f64 (path metric + branch metric)"
    # (the first decision of a word is written outright, v_cmp_lt_f64 -> v_cndmask_b32 0, 1, vcc: acs_min_first)
    if op == "v_cmp_lt_f64" or op.startswith("v_addc_co") or (prev == "v_cmp_lt_f64" and op == "v_cndmask_b32"):
        return "add-compare-select: v_cmp_lt_f64 + v_addc_co_u32 (decision bit)"
    if op == "v_min_f64":
        return "v_min_f64 (64 survivor selects + 63 of the minimum tree)"
    if op == "v_cmp_eq_f64" or op == "v_cndmask_b32":
        return "first-equal scan: v_cmp_eq_f64 + v_cndmask_b32"
    if op.startswith(("v_exp", "v_log", "v_frexp", "v_ldexp", "v_rndne", "v_fma_f64", "v_mul_f64", "v_cvt", "v_div", "v_rcp", "v_max_f64",
                      "v_fmac_f64", "v_cmp_class", "v_cmp_u_f64", "v_cmp_gt_f64", "v_cmp_ngt", "v_cmp_nlt", "v_cmp_le_f64", "v_cmp_ge_f64",
                      "v_cmp_neq", "v_trig", "v_med3")):
        return "LLR -> branch metrics (clip, exp, log, the four sums)"
    if op.startswith("ds_"):
        return "LDS (decision ring write, traceback reads, output tile)"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "memory (LLR loads, bit stores)"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_"):
        return "scalar (loop control, NaN mask, addresses)"
    if op.startswith(("v_lshl", "v_lshr", "v_and", "v_or", "v_bfe", "v_alignbit", "v_xor", "v_add_u32", "v_sub", "v_add_co", "v_lshrrev", "v_mov",
                      "v_ashr", "v_bfi", "v_mad", "v_mul_lo", "v_mul_u32", "v_readlane", "v_readfirstlane", "v_add3", "v_lshl_add", "v_and_or",
                      "v_lshl_or", "v_perm", "v_accvgpr", "v_cmp_", "v_subrev", "v_min_u32", "v_max_u32", "v_min_i32", "v_not")):
        return "traceback hops, addresses, moves (integer VALU)"
    return "other (" + op + ")"


TRACEBACK = ("v_lshlrev_b64", "v_alignbit_b32", "ds_", "s_waitcnt")
PHASES = ["LLR -> branch metrics (clip, exp, log, sums; pad select, NaN detect, loads, the previous step's ring / tile addresses)",
          "add-compare-select, butterflies 0 .. S/4 - 1", "add-compare-select, butterflies S/4 .. S/2 - 1",
          "minimum tree (of the high dwords where the 32-bit first-argmin is compiled in)",
          "first-equal scan / hit words and index, decision word, ring slot"]


def position_table(loop, steps):
    """Instructions per step by position: a step ends at its ds_write_b8 (output tile); inside it every batch of traceback reads
    (ds_read* more than 20 instructions after the previous one) starts the next phase."""
    cnt, tb = collections.Counter(), collections.Counter()
    phase, since, nsteps = 0, 10 ** 6, 0
    # A kernel with the 32-bit first-argmin may walk a whole group's tracebacks in ONE of its steps (WalkBurst): five steps of six then
    # have no read batch and no tile store to cut at.  Its steps are cut by what every step has, in the fixed order of cw_step's asm
    # statements: the first v_cmp_lt_f64 opens the butterflies, the 33rd their second half, the 64th closes them; the 8th v_cmp_eq_u32
    # (column hits) ends the minimum part and the 16th (row hits) the step -- the few instructions behind it (index, tie test, decision
    # word, ring write) are counted with the next step's first phase, as the ring and tile addresses always were.
    landmarks = EQ[0] == "v_cmp_eq_u32"
    lt = eq = 0
    for _, op, args in loop:
        if landmarks:
            if op == "v_cmp_lt_f64":
                lt += 1
                phase = 1 if lt <= 32 else 2
        elif op.startswith("ds_read"):
            if since > 20:
                phase = min(phase + 1, len(PHASES) - 1)
            since = 0
        else:
            since += 1
        if op.startswith(TRACEBACK):
            tb["traceback + tile: " + ("LDS" if op.startswith("ds_") else "s_waitcnt" if op.startswith("s_waitcnt") else "hops")] += 1
        else:
            cnt[phase] += 1
        if landmarks:
            if op == "v_cmp_lt_f64" and lt == 64:
                phase = 3
            elif op == "v_cmp_eq_u32":
                eq += 1
                if eq == 8:
                    phase = 4
                elif eq == 16:
                    phase, nsteps, lt, eq = 0, nsteps + 1, 0, 0
        elif op == "ds_write_b8":
            phase, nsteps = 0, nsteps + 1
    out = ["", "by position in the step (%d steps found per trip, cut at %s):" %
           (nsteps, "the compares every step has" if landmarks else "the tile stores"), "",
           "| phase of cw_step, by position | instructions per trellis step |", "|---|---|"]
    for ph in range(len(PHASES)):
        out.append("| %s | %.1f |" % (PHASES[ph], cnt[ph] / steps))
    for k in sorted(tb):
        out.append("| %s | %.1f |" % (k, tb[k] / steps))
    return out


def chunk_table(body, addr, hot, general=None):
    """Static counts of the per-chunk code around the hot loop `hot` = (first, last) and of the flush rounds inside it.
    `general`: the second group loop of a kernel that splits its groups into fast and general ones (main()); the compiler may
    then lay the chunk loop out so that no backward branch spans the hot loop -- the whole kernel stands in for it."""
    def branches():
        for i, (ad, op, args) in enumerate(body):
            if op.startswith("s_cbranch") or op == "s_branch":
                m = re.search(r"\+0x([0-9a-f]+)>\s*$", args)
                j = addr.get(body[0][0] + int(m.group(1), 16)) if m else None
                if j is not None:
                    yield j, i

    def loops():
        return ((j, i) for j, i in branches() if j < i)
    outer = min(((j, i) for j, i in loops() if j < hot[0] and i > hot[1]), key=lambda ji: ji[1] - ji[0], default=None)
    out = ["", "per 96-step chunk, outside the hot loop (static counts; the hot loop runs 16 trips per chunk):", ""]
    whole = outer is None
    if whole:
        if general is None:
            return out + ["(no loop around the hot loop found)"]
        outer = (0, len(body) - 1)
        out += ["(no backward branch spans the hot loop: counted over the whole kernel, its prologue and epilogue included)", ""]
    rounds = [(j, i) for j, i in loops() if outer[0] <= j and i <= outer[1] and (i < hot[0] or j > hot[1]) and
              not (general and general[0] <= j and i <= general[1]) and not (general and j <= general[0] and i >= general[1]) and
              any(o.startswith("global_store") for _, o, _ in body[j:i + 1])]
    rnd = min(rounds, key=lambda ji: ji[1] - ji[0], default=None)
    # the float64 fallback of the 32-bit first-argmin: blocks behind the hot loop that a forward branch out of the loop enters and
    # that end with a branch back into it, each holding a first-equal scan (64 v_cmp_eq_f64).  A step runs one only when a lane of
    # its wave has a high-dword tie; they are not part of what a chunk executes besides its steps.
    cold = []
    for lp in [hot] + ([general] if general else []):
        for t, i in branches():
            if lp[0] <= i <= lp[1] and outer[1] >= t > lp[1]:
                e = next((k for j, k in branches() if k >= t and lp[0] <= j <= lp[1]), None)
                if e is not None and sum(1 for _, o, _ in body[t:e + 1] if o == "v_cmp_eq_f64") >= 64 and (t, e) not in cold:
                    cold.append((t, e))
    n_cold = sum(e - t + 1 for t, e in cold)
    n_outer = outer[1] - outer[0] + 1 - (hot[1] - hot[0] + 1) - n_cold - (general[1] - general[0] + 1 if general else 0)
    out += ["| block | instructions |", "|---|---|"]
    if cold:
        out.append("| float64 fallback of the first-argmin, %d blocks out of line behind the loop(s) (one per unrolled step; a step runs its block "
                   "only when a lane of the wave has a high-dword tie): NOT part of the rows below | %d |" % (len(cold), n_cold))
    if rnd:
        seg = body[rnd[0]:rnd[1] + 1]
        n_rnd = len(seg)
        out.append("| flush, one round of eight codewords (x 8 per chunk): %d LDS reads, %d stores, %d branches | %d |" %
                   (sum(o.startswith("ds_read") for _, o, _ in seg), sum(o.startswith("global_store") for _, o, _ in seg),
                    sum(o.startswith(("s_cbranch", "s_branch")) for _, o, _ in seg), n_rnd))
        if whole:
            out.append("| everything else outside the two group loops: kernel prologue, chunk set-up, flush set-up, the pending and the "
                       "final walk (not a per-chunk figure) | %d |" % (n_outer - n_rnd))
        else:
            out.append("| chunk set-up, flush set-up, the last chunk's pending walk | %d |" % (n_outer - n_rnd))
            out.append("| **per chunk, every flush instruction executed** | **%d** = %.1f per trellis step |" %
                       (n_outer - n_rnd + 8 * n_rnd, (n_outer - n_rnd + 8 * n_rnd) / 96.0))
    else:
        out.append("| all of it (no flush round loop found) | %d |" % n_outer)
    return out


EQ = ["v_cmp_eq_f64", 64]      # main(): "v_cmp_eq_u32", 16 per step, for a kernel that has the 32-bit first-argmin (its float64 scan is the cold fallback)


def eq_compares(seg):
    """Equality compares of the step's first-argmin in a stretch of code, in units of 64: EQ[1] of them per trellis step."""
    return sum(1 for _, o, _ in seg if o == EQ[0]) * (64 // EQ[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default=DEFAULT)
    ap.add_argument("--obj", default=os.path.join(ROOT, "commpy_amd", "csrc", "build", "viterbi_cw.o"))
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    body = kernel_body(disassemble(a.obj), a.kernel)
    if not body:
        sys.exit("kernel not found: " + a.kernel)
    addr = {ad: i for i, (ad, _, _) in enumerate(body)}
    if sum(1 for _, o, _ in body if o == "v_cmp_eq_u32") >= 16 and any(o == "v_min3_u32" for _, o, _ in body):
        EQ[:] = ["v_cmp_eq_u32", 16]
    # the step loop: of the backward branches whose span holds the most trellis steps (64 equality compares each), the SMALLEST span.
    # (The loop around it, which flushes the output tile every 96 steps, holds the same steps in a larger span; the out-of-line
    # fallback blocks of the 32-bit first-argmin sit behind the loop and branch back into it: their spans hold fewer steps.)
    cands = []
    for i, (ad, op, args) in enumerate(body):
        if op.startswith("s_cbranch") or op == "s_branch":
            m = re.search(r"\+0x([0-9a-f]+)>\s*$", args)
            if not m:
                continue
            # the operand is printed relative to the kernel symbol: resolve through the first instruction's address
            j = addr.get(body[0][0] + int(m.group(1), 16))
            if j is not None and j < i and eq_compares(body[j:i + 1]) >= 64:
                cands.append((-(eq_compares(body[j:i + 1]) // 64), i - j, j, i))
    # (where the compiler lays the chunk loop out around both group loops, that span holds twice the steps: a trip of the step loop is
    # one group of LGS steps, the kernel's first template argument)
    lgs = re.search(r"<(\d+),", a.kernel)
    group = [c for c in cands if lgs and -c[0] == int(lgs.group(1))]
    cands = group or cands
    best = min(cands)[2:] if cands else None
    if best is None:
        sys.exit("no loop found")
    loop = body[best[0]:best[1] + 1]
    steps = eq_compares(loop) // 64
    # a kernel that splits its groups into fast and general ones has a second loop of as many steps beside the hot one: the general
    # body, run by the groups that touch padding or step T (the last ones of a codeword)
    others = [c for c in cands if -c[0] == steps and (c[3] < best[0] or c[2] > best[1])]
    general = min(others)[2:] if others else None
    cnt = collections.Counter(classify(op, args, loop[k - 1][1] if k else None) for k, (_, op, args) in enumerate(loop))
    valu = sum(v for k, v in cnt.items() if not k.startswith(("LDS", "memory", "s_", "scalar")))
    lines = ["kernel: %s" % a.kernel,
             "hot loop: %d instructions per trip, %d trellis steps per trip (kernel: %d instructions)" % (len(loop), steps, len(body))] + \
            (["general group loop (behind the hot loop; groups that touch padding or step T): %d instructions per trip = %.1f per step"
              % (general[1] - general[0] + 1, (general[1] - general[0] + 1) / steps)] if general else []) + ["",
             "| phase of cw_step | instructions per trellis step |", "|---|---|"]
    for k, v in sorted(cnt.items(), key=lambda kv: -kv[1]):
        lines.append("| %s | %.1f |" % (k, v / steps))
    lines += ["| **all** | **%.1f** (vector ALU: %.1f) |" % (len(loop) / steps, valu / steps)]
    lines += position_table(loop, steps) + chunk_table(body, addr, best, general)
    text = "\n".join(lines)
    print(text)
    if a.md:
        open(a.md, "w").write(text + "\n")


if __name__ == "__main__":
    main()
