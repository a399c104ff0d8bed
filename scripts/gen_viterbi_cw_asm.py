#!/usr/bin/env python3
"""Generates commpy_amd/csrc/viterbi_cw_asm.h: the two straight-line VALU sequences of cw_step (64 states, float64) that are
written as a few LARGE asm statements instead of one small statement per instruction.

Why: hipcc (ROCm 7.2) puts `s_nop 0` between two asm statements when the second reads a VGPR the first wrote (it cannot see
whether the producer uses dst_sel, the gfx940 "dst_sel forwarding" hazard), and it serialises a chain of such statements: the
64-state minimum tree and first-equal scan of one trellis step cost 35 s_nop per step that way (212 per unrolled group of six
steps).  Inside ONE statement the order is ours: four independent chains are interleaved, no wait states are needed, and
the number of statement boundaries drops from ~80 to 6 per step.  An asm statement takes at most 30 operands, hence blocks of 24
registers; state numbers are literals in the text (they are inline constants of v_cndmask_b32).

'soft' runs a 32-bit block first (cw_step: "first-argmin on the high dwords"): the 64 high dwords as an 8 x 8 grid over the logical
state, the unsigned minimum of every column and of every row as a chain of three v_min3_u32 and one v_min_u32 (CPX_COL_BLOCK*,
CPX_ROW_BLOCK*; three chains interleaved per statement), the overall minimum from the column minima, and one hit bit per column and per row
-- v_cmp_eq_u32 against that minimum, shifted into ONE 16-bit word by v_addc_co_u32 exactly as the decision words are.  The index of the
single hit and the mask of lanes with more than one come from that word.  The float64 blocks above then run only for a wave in which some
lane has more than one hit.  Which register holds which state is the caller's business: the blocks only fix the operand order.

    python scripts/gen_viterbi_cw_asm.py > commpy_amd/csrc/viterbi_cw_asm.h
"""


def min_block(n_in):
    """4 accumulators %0..%3 (+v), n_in inputs %4..: acc[i % 4] = min(acc[i % 4], in[i]), chains interleaved."""
    return "\\n\\t".join("v_min_f64 %%%d, %%%d, %%%d" % (i % 4, i % 4, 4 + i) for i in range(n_in))


def scan_block(states):
    """%0 bst (+v), %1..%4 SGPR pairs (=&s), %5 the minimum, %6.. the metrics of `states` (descending state numbers):
    bst = state where metric == minimum, later (= lower) states overwrite earlier ones -> the FIRST equal state wins."""
    out = []
    for q in range(0, len(states), 4):
        quad = states[q:q + 4]
        for j, _ in enumerate(quad):
            out.append("v_cmp_eq_f64 %%%d, %%%d, %%5" % (1 + j, 6 + q + j))
        for j, s in enumerate(quad):
            out.append("v_cndmask_b32 %%0, %%0, %d, %%%d" % (s, 1 + j))
    return "\\n\\t".join(out)


def min8(dst, ins):
    """The four instructions that leave the unsigned minimum of the eight operands `ins` in `dst`."""
    return ["v_min3_u32 %%%d, %%%d, %%%d, %%%d" % (dst, ins[0], ins[1], ins[2]), "v_min3_u32 %%%d, %%%d, %%%d, %%%d" % (dst, dst, ins[3], ins[4]),
            "v_min3_u32 %%%d, %%%d, %%%d, %%%d" % (dst, dst, ins[5], ins[6]), "v_min_u32 %%%d, %%%d, %%%d" % (dst, dst, ins[7])]


def interleave(chains):
    return [ins for rank in zip(*chains) for ins in rank]


def hit(word, m, x, first=False):
    """word = 2 word + (x == m): the compare -> v_addc pattern of the decision words (first: the word starts as the bit itself)."""
    return ["v_cmp_eq_u32 vcc, %%%d, %%%d" % (m, x),
            "v_cndmask_b32 %%%d, 0, 1, vcc" % word if first else "v_addc_co_u32 %%%d, vcc, %%%d, %%%d, vcc" % (word, word, word)]


def col_block(n):
    """%0..%(n-1) (=&v) the minima of n columns, %n.. the eight high dwords of each column in turn; the n chains interleaved."""
    return "\\n\\t".join(interleave([min8(c, [n + 8 * c + k for k in range(8)]) for c in range(n)]))


def col_last_block():
    """%0 %1 (=&v) the minima of columns 6 and 7, %2 (=&v) m = the minimum of the eight column minima, %3 (=&v) the hit word, %4..%9 the
    minima of columns 0..5, %10.. the high dwords of columns 6 and 7.  Two of m's four instructions need columns 0..5 only and run
    between the two chains.  Then the column hits, column 7 first: column i ends at bit i of the word (at bit 8 + i once the eight
    row hits have been shifted in behind them)."""
    c6, c7 = min8(0, list(range(10, 18))), min8(1, list(range(18, 26)))
    fold = ["v_min3_u32 %2, %4, %5, %6", "v_min3_u32 %3, %7, %8, %9"]
    out = c6[:1] + c7[:1] + fold[:1] + c6[1:2] + c7[1:2] + fold[1:] + c6[2:3] + c7[2:3] + c6[3:] + c7[3:]
    out += ["v_min3_u32 %2, %2, %3, %0", "v_min_u32 %2, %2, %1"]
    for i in range(7, -1, -1):
        out += hit(3, 2, (4 + i) if i < 6 else (i - 6), first=(i == 7))
    return "\\n\\t".join(out)


def row_block(n, last=False, tie_first=True):
    """%0 the hit word (+v), %1..%n row minima (=&v, temporaries), then m and the eight high dwords of each of n rows, the highest row
    first: the n chains interleaved, each row compared with m and shifted into the word as the columns were -- row j ends at bit j.
    last: two more outputs between the temporaries and m: the index 8 j + i of the hit (=&v; j = the lowest set bit of the word, i =
    the lowest set bit above bit 7; the temporaries serve as scratch) and an SGPR pair = lanes whose word has not exactly two bits
    set -- more than one hit row or more than one hit column, i.e. more than one hit state."""
    m = n + 1 + (2 if last else 0)
    out = interleave([min8(1 + r, [m + 1 + 8 * r + k for k in range(8)]) for r in range(n)])
    for r in range(n):
        out += hit(0, m, 1 + r)
    if last:
        # tie_first: the four instructions of the index stand between the compare that writes the tie mask and the scalar test and branch
        # that read it (timed gain with no instruction removed: experiments/README.md); otherwise the compare comes next to last, as the
        # kernels that do not take the pinned form of the step keep it
        if tie_first:
            out += ["v_bcnt_u32_b32 %2, %0, 0", "v_cmp_ne_u32 %4, 2, %2", "v_ffbl_b32 %3, %0", "v_lshrrev_b32 %1, 8, %0", "v_ffbl_b32 %1, %1",
                    "v_lshl_or_b32 %3, %3, 3, %1"]
        else:
            out += ["v_ffbl_b32 %3, %0", "v_lshrrev_b32 %1, 8, %0", "v_bcnt_u32_b32 %2, %0, 0", "v_ffbl_b32 %1, %1", "v_cmp_ne_u32 %4, 2, %2",
                    "v_lshl_or_b32 %3, %3, 3, %1"]
    return "\\n\\t".join(out)


print("// GENERATED by scripts/gen_viterbi_cw_asm.py -- do not edit; see that script for the why.")
print("#pragma once")
print('#define CPX_MIN_BLOCK24 "%s"' % min_block(24))
print('#define CPX_MIN_BLOCK12 "%s"' % min_block(12))
blocks = [list(range(63, 39, -1)), list(range(39, 15, -1)), list(range(15, -1, -1))]
for i, b in enumerate(blocks):
    print('#define CPX_SCAN_BLOCK%d "%s"   // states %d .. %d' % (i, scan_block(b), b[0], b[-1]))
print('#define CPX_COL_BLOCK3 "%s"   // three column minima' % col_block(3))
print('#define CPX_COL_BLOCK_LAST "%s"   // columns 6 and 7, the minimum, the column hits' % col_last_block())
print('#define CPX_ROW_BLOCK3 "%s"   // three rows: minima and hits' % row_block(3))
print('#define CPX_ROW_BLOCK_LAST "%s"   // rows 1 and 0, the tie mask, the index' % row_block(2, last=True))
print('#define CPX_ROW_BLOCK_LAST_INDEX_FIRST "%s"   // rows 1 and 0, the index, the tie mask' % row_block(2, last=True, tie_first=False))
