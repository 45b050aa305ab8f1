"""tools/ba1_isa_mix.py [LISTING] [--blocks]: instruction mix of the Levenberg trial of bafd2000::k_ba1_fast, per section and per
basic block.

LISTING is the assembly tools/baf_quick.sh leaves (default /tmp/baf_quick.s).  Every instruction is put into one class by the
PREFIX of its mnemonic alone: v_*_f64, v_mov*, v_permlane*, v_readlane / v_readfirstlane, v_cndmask*, other v_*, ds_*, global_*,
and everything that starts with s_ as one class.  A basic block runs from a label or the instruction behind a branch to the
next label or branch.

The sections of a trial are found by their landmarks, in listing order (= program order here):
  pass A            from the block with the last `s_setprio 2` in front of the widest lane-swap block to that block
  reduction A       the block with the most v_permlane* (the 29-value butterfly), up to its s_barrier: every wave runs it
  totals uniform    behind that barrier up to the next label: wave 0 adds the group totals and spreads the 29 sums over its lanes
  solve             from there to the next s_barrier: the 6 x 6 solve on wave 0 (seven waves wait at the barrier)
  hand-over         behind that barrier up to the first branch on the exec mask: step and status into scalar registers, every wave
  trial pose        from there up to the block with the next `s_setprio 2`: exp(dx) P on wave 0, the others branch over it
  pass B            from there to the next block with v_permlane*
  reduction B       that block up to its s_barrier (the 2-value butterfly)
  verdict           behind the barrier to the branch back to the head of the trial: block adds, computeScale, accept / reject
--blocks lists the basic blocks of every section as well.
"""
import re
import sys

CLASSES = ["v_*_f64", "v_mov*", "v_permlane*", "v_readlane/rfl", "v_cndmask*", "other v_*", "ds_*", "global_*", "s_*", "other"]
SECTIONS = ["pass A", "reduction A", "totals uniform", "solve", "hand-over", "trial pose", "pass B", "reduction B", "verdict"]


def classify(op):
    if op.startswith("v_"):
        if op.startswith("v_mov"):
            return 1
        if op.startswith("v_permlane"):
            return 2
        if op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
            return 3
        if op.startswith("v_cndmask"):
            return 4
        if "_f64" in op:
            return 0
        return 5
    if op.startswith("ds_"):
        return 6
    if op.startswith("global_"):
        return 7
    if op.startswith("s_"):
        return 8
    return 9


def kernel_items(path, want="bafd2000", kernel="k_ba1_fast"):
    """[("label", name) | ("op", mnemonic, operands)] of the kernel whose mangled name holds both strings"""
    out, inside = [], False
    for line in open(path):
        s = line.split(";")[0].strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            name = m.group(1)
            if not name.startswith(".L"):
                inside = want in name and kernel in name and not name.endswith(".kd")
            elif inside:
                out.append(("label", name))
            continue
        if not inside or not s or s.startswith("."):
            continue
        parts = s.split(None, 1)
        if re.match(r"^[a-z][a-z0-9_]*$", parts[0]):
            out.append(("op", parts[0], parts[1] if len(parts) > 1 else ""))
            if parts[0] == "s_endpgm":
                inside = False
    return out


def basic_blocks(items):
    """[(name, first item index, [item indices of its instructions])]"""
    blocks, cur, last_label, n_after = [], None, "entry", 0
    for i, it in enumerate(items):
        if it[0] == "label":
            last_label, n_after = it[1], 0
            cur = [it[1], i, []]
            blocks.append(cur)
            continue
        if cur is None:
            n_after += 1
            cur = ["%s+%d" % (last_label, n_after), i, []]
            blocks.append(cur)
        cur[2].append(i)
        if it[1].startswith(("s_cbranch", "s_branch")):
            cur = None
    return blocks


def find_sections(items, blocks):
    """{section: (first item index, one past the last)}"""
    ops = lambda b: [items[i][1] for i in b[2]]
    nperm = [sum(o.startswith("v_permlane") for o in ops(b)) for b in blocks]
    ra = max(range(len(blocks)), key=lambda k: nperm[k])

    def next_op(start, pred):
        for i in range(start, len(items)):
            if items[i][0] == "op" and pred(items[i]):
                return i
        sys.exit("landmark not found behind item %d" % start)

    def next_label(start):
        for i in range(start, len(items)):
            if items[i][0] == "label":
                return i
        sys.exit("no label behind item %d" % start)

    def block_with_prio2(before=None, after=None):
        ks = [k for k, b in enumerate(blocks) if any(items[i][1] == "s_setprio" and items[i][2].strip() == "2" for i in b[2])]
        if before is not None:
            return max(k for k in ks if blocks[k][1] < before)
        return min(k for k in ks if blocks[k][1] > after)

    a0 = blocks[block_with_prio2(before=blocks[ra][1])][1]
    head = items[a0][1] if items[a0][0] == "label" else None
    ra0 = blocks[ra][1]
    bar_a = next_op(ra0, lambda it: it[1] == "s_barrier")
    uni_end = next_label(bar_a)
    bar_s = next_op(uni_end, lambda it: it[1] == "s_barrier")
    b0 = blocks[block_with_prio2(after=bar_s)][1]
    ho_end = next_op(bar_s + 1, lambda it: it[1].startswith("s_cbranch_exec")) + 1
    rb = min(k for k in range(len(blocks)) if blocks[k][1] > b0 and nperm[k])
    rb0 = blocks[rb][1]
    bar_b = next_op(rb0, lambda it: it[1] == "s_barrier")
    heads = {items[i][1] for i in range(a0, min(a0 + 40, len(items))) if items[i][0] == "label" and i < ra0}
    if head:
        heads.add(head)
    back = next_op(bar_b, lambda it: it[1].startswith(("s_branch", "s_cbranch")) and it[2].strip() in heads)
    while items[back + 1][0] == "op" and items[back + 1][1].startswith("s_branch") and items[back + 1][2].strip() in heads:
        back += 1
    return dict(zip(SECTIONS, [(a0, ra0), (ra0, bar_a + 1), (bar_a + 1, uni_end), (uni_end, bar_s + 1), (bar_s + 1, ho_end), (ho_end, b0), (b0, rb0),
                               (rb0, bar_b + 1), (bar_b + 1, back + 1)]))


def mix(items, idx):
    c = [0] * len(CLASSES)
    for i in idx:
        if items[i][0] == "op":
            c[classify(items[i][1])] += 1
    return c


def row(name, blk, c):
    return "%-16s %-14s %5d %5d | " % (name, blk, sum(c), sum(c[:6])) + " ".join("%9d" % v for v in c)


def main(argv):
    per_block = "--blocks" in argv
    args = [a for a in argv if not a.startswith("--")]
    path = args[0] if args else "/tmp/baf_quick.s"
    items = kernel_items(path)
    if not items:
        sys.exit("no bafd2000::k_ba1_fast in %s" % path)
    blocks = basic_blocks(items)
    sec = find_sections(items, blocks)
    hdr = "%-16s %-14s %5s %5s | " % ("section", "block", "insts", "VALU") + " ".join("%9s" % c[:9] for c in CLASSES)
    print(hdr)
    print("-" * len(hdr))
    tot = {}
    for name in SECTIONS:
        lo, hi = sec[name]
        c = tot[name] = mix(items, range(lo, hi))
        print(row(name, "", c))
        if per_block:
            for b in blocks:
                idx = [i for i in b[2] if lo <= i < hi]
                if idx:
                    print(row("", b[0][:14], mix(items, idx)))
    valu = lambda n: sum(tot[n][:6])
    print()
    print("reductions, every wave and trial (reduction A + hand-over + reduction B + verdict): %d VALU"
          % (valu("reduction A") + valu("hand-over") + valu("reduction B") + valu("verdict")))
    print("  of which the butterflies up to their barriers (reduction A + reduction B):          %d VALU" % (valu("reduction A") + valu("reduction B")))
    print("wave 0 alone, the 29 totals added and made uniform (totals uniform):                  %d VALU" % valu("totals uniform"))


if __name__ == "__main__":
    main(sys.argv[1:])
