#!/usr/bin/env python3
"""Development aid (no GPU): static instruction mix of one kernel in a `hipcc --cuda-device-only -S` listing.
    tools/instr_mix.py listing.s _ZN3ssg11step_kernelILi8ELi256ELb1ELb0ELb0EE [--regions] [--min-valu N]

Prints the VALU instructions of the kernel by CLASS (what an issue slot is spent on), and with --regions the same table per
REGION of the listing.  The roles of the step kernel are separate straight-line stretches of one function; what separates
them, and a role's sections from each other, are the places where a wave waits for another: `s_barrier` (barrier 0, one per
role), the `s_sleep` of a poll loop (pose hand-over, rendezvous), a call (`s_swappc_b64`: sincos) and `s_endpgm`.  A region
is the listing between two such lines; it is named by its index and its first label.  Loops are counted once (static counts).
"""
import collections, re, sys

CLASSES = [  # first match wins
    ("fp64 arith", re.compile(r"v_(mul|add|fma|fmac|min|max|div_fmas|div_fixup|div_scale|rcp|rsq|sqrt|trunc|floor|ceil|rndne|fract|ldexp|frexp_mant)_f64")),
    ("fp64 compare", re.compile(r"v_cmpx?_\w+_f64")),
    ("select (v_cndmask)", re.compile(r"v_cndmask_b32")),
    ("move (v_mov)", re.compile(r"v_mov_b(32|64)|v_accvgpr")),
    ("address / index", re.compile(r"v_(lshl_add_u64|lshl_add_u32|add_lshl_u32|lshl_or_b32|add_u32|sub_u32|subrev_u32|add_co_u32|addc_co_u32|add3_u32|"
                                   r"lshlrev_b32|lshlrev_b64|lshrrev_b32|ashrrev_i32|ashrrev_i64|mul_lo_u32|mul_hi_u32|mul_hi_i32|mul_u32_u24|mul_i32_i24|"
                                   r"mad_u64_u32|mad_i64_i32|mad_u32_u24|mad_i32_i24|and_b32|or_b32|xor_b32|and_or_b32|or3_b32|bfe_u32|bfe_i32|bfi_b32|not_b32|"
                                   r"min_i32|max_i32|min_u32|max_u32|med3_i32|sub_co_u32|subb_co_u32|bcnt_u32_b32|ffbl_b32|ffbh_u32|bitop3_b32|xad_u32|mul_lo_u16)\b")),
    ("integer compare", re.compile(r"v_cmpx?_\w+_[iu](16|32|64)|v_cmp_class")),
    ("lane traffic", re.compile(r"v_(readlane|readfirstlane|writelane|mbcnt|permlane|swap)|ds_bpermute|ds_permute|_dpp|row_shr|row_bcast")),
    ("convert", re.compile(r"v_cvt_")),
]
BOUNDARY = re.compile(r"^(s_barrier|s_sleep|s_endpgm|s_swappc_b64)\b")


def opcode(line):
    return re.sub(r"_(e32|e64|sdwa|dpp|e64_dpp)$", "", line.split()[0])


def classify(line):
    op = opcode(line)
    if not op.startswith("v_"):
        return None
    if "dpp" in line or "row_" in line:
        return "lane traffic"
    for name, rx in CLASSES:
        if rx.match(op):
            return name
    return "other VALU"


def table(lines):
    c = collections.Counter()
    ops = collections.Counter()
    for l in lines:
        k = classify(l)
        if k:
            c[k] += 1
        ops[opcode(l)] += 1
    return c, ops


def fmt(c):
    names = [n for n, _ in CLASSES] + ["other VALU"]
    return "  ".join("%s %d" % (n, c[n]) for n in names if c[n])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    regions = "--regions" in sys.argv
    min_valu = int(sys.argv[sys.argv.index("--min-valu") + 1]) if "--min-valu" in sys.argv else 20
    if "--min-valu" in sys.argv:
        args.remove(str(min_valu))
    txt = open(args[0]).read()
    name = args[1]
    i = txt.index("\n" + name)
    j = txt.index(".Lfunc_end", i)
    body = [l.strip() for l in txt[i:j].split("\n")[1:]]
    body = [l for l in body if l and not l.startswith((";", ".")) or re.match(r"^\.LBB\d+_\d+:", l)]
    insts = [l for l in body if not l.endswith(":")]
    c, ops = table(insts)
    valu = sum(c.values())
    print("static instructions %d (VALU %d): v_fma_f64 %d v_mul_f64 %d v_add_f64 %d ds_* %d s_waitcnt %d" % (
        len(insts), valu, ops["v_fma_f64"], ops["v_mul_f64"], ops["v_add_f64"], sum(v for k, v in ops.items() if k.startswith("ds_")), ops["s_waitcnt"]))
    print("VALU by class: " + fmt(c))
    print("SALU %d  LDS %d  VMEM %d  scratch %d" % (
        sum(v for k, v in ops.items() if k.startswith("s_") and not k.startswith(("s_waitcnt", "s_nop", "s_load", "s_endpgm"))),
        sum(v for k, v in ops.items() if k.startswith("ds_")), sum(v for k, v in ops.items() if k.startswith(("global_", "buffer_", "flat_"))),
        sum(v for k, v in ops.items() if k.startswith("scratch_"))))
    detail = ["v_cndmask_b32", "v_mov_b32", "v_mov_b64", "v_lshl_add_u64", "v_lshl_add_u32", "v_add_u32", "v_lshlrev_b32", "v_mul_lo_u32", "v_mad_u64_u32"]
    print("of which: " + "  ".join("%s %d" % (k, ops[k]) for k in detail))
    if not regions:
        return
    print("\nregions (between s_barrier / s_sleep / call / s_endpgm; loops counted once), VALU >= %d:" % min_valu)
    reg, label, last_label, idx, start = [], "(entry)", "(entry)", 0, 0
    n = 0
    for l in body:
        if l.endswith(":"):
            last_label = l[:-1]
            if not reg or label is None:
                label = last_label
            continue
        if label is None:
            label = "after " + last_label
        n += 1
        reg.append(l)
        if BOUNDARY.match(l):
            rc, _ = table(reg)
            if sum(rc.values()) >= min_valu:
                print("  #%-3d %-12s inst %5d..%-5d ends at %-12s VALU %4d: %s" % (idx, label, start, n, l.split()[0], sum(rc.values()), fmt(rc)))
            idx += 1
            reg, start, label = [], n, None
    if reg:
        rc, _ = table(reg)
        print("  #%-3d %-12s inst %5d..%-5d (end)              VALU %4d: %s" % (idx, label, start, n, sum(rc.values()), fmt(rc)))


if __name__ == "__main__":
    main()
