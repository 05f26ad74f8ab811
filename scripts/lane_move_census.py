#!/usr/bin/env python3
"""Static census of scalar-spill lane moves (v_readlane_b32 / v_writelane_b32) in one kernel of a device assembly listing.

Input: the `-S` output of the device compile of faster_amd/csrc/fh_capi.hip, made with the flags of faster_amd/build.py plus
`--cuda-device-only -S` (no GPU needed):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -sink-insts-to-avoid-spills -mllvm -disable-machine-licm \
        --cuda-device-only -S -o fh_capi.s faster_amd/csrc/fh_capi.hip
    python scripts/lane_move_census.py fh_capi.s > profiles/r11_lane_moves.txt

Everything here is a STATIC count: it says nothing about how often a block runs.

What is reported for the chosen kernel (default: solve_kernel<10, true, 3, false>):
  * vector instructions in total, lane reads and lane writes, by loop depth (the depth the assembly printer notes on each block);
  * lane reads per spill register, and for the spill slots that were filled straight from an s_load_dwordxN (launch arguments):
    the reads per slot and per loop; likewise for the arguments that fh::own_sreg() made single values at kernel entry (a scalar move
    inside an asm statement), in the order of fh::split_args();
  * runs of >= 4 reads of consecutive lanes of one register (a tuple reloaded to use a part of it).
"""
import argparse
import collections
import re
import sys

SREG = re.compile(r"^s(\d+)$")
SRANGE = re.compile(r"^s\[(\d+):(\d+)\]$")


def sregs(op):
    m = SREG.match(op)
    if m:
        return [int(m.group(1))]
    m = SRANGE.match(op)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    return []


def kernel_body(lines, tag):
    """Lines of the first function whose label contains `tag`, from its label to .Lfunc_end."""
    start = None
    for i, ln in enumerate(lines):
        if start is None:
            if ":" in ln and not ln.startswith((".", " ", "\t", ";")) and tag in ln.split(":")[0]:
                start = i
        elif ln.startswith(".Lfunc_end"):
            return lines[start:i], lines[start].split(":")[0]
    raise SystemExit("no kernel whose name contains %r" % tag)


def census(body):
    depth, header = 0, "-"
    pending_block = False
    valu = collections.Counter()      # depth -> vector instructions
    reads = collections.Counter()     # depth -> v_readlane_b32
    writes = collections.Counter()    # depth -> v_writelane_b32
    loop_valu = collections.Counter()  # innermost loop header -> vector instructions
    loop_moves = collections.Counter()
    loop_depth = {}
    reads_reg = collections.Counter()
    lane_reads = collections.Counter()          # (vreg, lane) -> reads
    lane_reads_loop = collections.Counter()     # (vreg, lane, header) -> reads
    lane_src = {}                               # (vreg, lane) -> (load id) if filled from an s_load result
    sdef = {}                                   # sreg -> (load id, word)
    loads = []                                  # (width, base, offset)
    runs = []                                   # (length, depth, header, vreg, first lane)
    run = None
    in_asm = False
    for ln in body:
        s = ln.strip()
        if not s:
            continue
        # block boundaries and the loop notes that follow them
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", s):
            depth, header, pending_block = 0, "-", True
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", s)
            if m:
                header, depth = m.group(1), int(m.group(2))
            lab = re.match(r"^\.L(BB\d+_\d+):", s)
            cur_label = lab.group(1) if lab else None
            run = None
            continue
        if s.startswith(";;#ASMSTART") or s.startswith(";;#ASMEND"):
            in_asm = s.startswith(";;#ASMSTART")
            continue
        if s.startswith(";"):
            if pending_block:
                m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", s)
                if m:
                    header, depth = m.group(1), int(m.group(2))
                m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", s)
                if m and cur_label:
                    header, depth = cur_label, int(m.group(1))
            continue
        pending_block = False
        if s.startswith("."):
            continue
        if header != "-":
            loop_depth[header] = depth
        code = s.split(";")[0].strip()
        parts = code.split(None, 1)
        op = parts[0]
        args = [a.strip() for a in parts[1].split(",")] if len(parts) > 1 else []
        if op.startswith("s_load_dword") and len(args) >= 3:
            lid = len(loads)
            loads.append((op[len("s_load_"):], args[1], args[2]))
            for w, r in enumerate(sregs(args[0])):
                sdef[r] = (lid, w)
        elif in_asm and op in ("s_mov_b32", "s_mov_b64") and len(args) == 2:  # own_sreg(): a launch argument made a value of its own
            lid = len(loads)
            loads.append(("own", args[1], "#%d" % sum(1 for l in loads if l[0] == "own")))
            for w, r in enumerate(sregs(args[0])):
                sdef[r] = (lid, w)
        elif op.startswith("s_") and args and not op.startswith(("s_cmp", "s_cbranch", "s_branch", "s_waitcnt", "s_bitcmp")):
            for r in sregs(args[0]):
                sdef.pop(r, None)
        if not op.startswith("v_"):
            continue  # (scalar instructions and waits between two lane reads do not end a run)
        valu[depth] += 1
        loop_valu[header] += 1
        if op == "v_readlane_b32":
            for r in sregs(args[0]):
                sdef.pop(r, None)
            reads[depth] += 1
            loop_moves[header] += 1
            if not args[2].isdigit():  # (a lane chosen at run time: the kernel's own broadcast, not a reload)
                run = None
                continue
            vreg, lane = args[1], int(args[2])
            reads_reg[vreg] += 1
            lane_reads[(vreg, lane)] += 1
            lane_reads_loop[(vreg, lane, header)] += 1
            if run and run[0] == vreg and run[2] + 1 == lane:
                run[2] = lane
            else:
                if run and run[2] - run[1] + 1 >= 4:
                    runs.append((run[2] - run[1] + 1, run[3], run[4], run[0], run[1]))
                run = [vreg, lane, lane, depth, header]
            continue
        if run and run[2] - run[1] + 1 >= 4:
            runs.append((run[2] - run[1] + 1, run[3], run[4], run[0], run[1]))
        run = None
        if op == "v_writelane_b32":
            writes[depth] += 1
            loop_moves[header] += 1
            src = sregs(args[1])
            if src and src[0] in sdef:
                lane_src[(args[0], int(args[2]))] = sdef[src[0]]
    return dict(valu=valu, reads=reads, writes=writes, loop_valu=loop_valu, loop_moves=loop_moves, loop_depth=loop_depth,
                reads_reg=reads_reg, lane_reads=lane_reads, lane_reads_loop=lane_reads_loop, lane_src=lane_src, loads=loads, runs=runs)


def per_loop_of(c, vreg, lanes):
    per_loop = collections.Counter()
    for (v2, l2, h), n in c["lane_reads_loop"].items():
        if v2 == vreg and l2 in lanes:
            per_loop[h] += n
    return per_loop


def report(name, c, out):
    p = lambda *a: print(*a, file=out)  # noqa: E731
    p("kernel: %s" % name)
    p("static counts; nothing here says how often a block runs")
    p("")
    p("vector instructions        %6d" % sum(c["valu"].values()))
    p("  v_readlane_b32           %6d" % sum(c["reads"].values()))
    p("  v_writelane_b32          %6d" % sum(c["writes"].values()))
    p("")
    p("by loop depth:   depth   vector   readlane  writelane")
    for d in sorted(c["valu"]):
        p("                 %5d   %6d   %8d  %9d" % (d, c["valu"][d], c["reads"][d], c["writes"][d]))
    p("")
    p("loops with >= 40 lane moves (innermost loop of each block):  header  depth  vector  lane moves")
    for h, n in c["loop_moves"].most_common():
        if n >= 40 and h != "-":
            p("    %-12s %5d  %6d  %10d" % (h, c["loop_depth"].get(h, 0), c["loop_valu"][h], n))
    p("")
    p("lane reads per spill register:")
    for v, n in c["reads_reg"].most_common():
        p("    %-6s %5d" % (v, n))
    p("")
    p("spill slots filled straight from a scalar load (launch arguments and what was loaded through them):")
    slots = collections.defaultdict(list)
    own = []
    for (vreg, lane), (lid, w) in c["lane_src"].items():
        slots[(lid, vreg)].append((lane, w))
    for (lid, vreg), lanes in sorted(slots.items(), key=lambda kv: -sum(c["lane_reads"][(kv[0][1], l)] for l, _ in kv[1])):
        width, base, off = c["loads"][lid]
        total = sum(c["lane_reads"][(vreg, l)] for l, _ in lanes)
        if total == 0:
            continue
        ls = sorted(l for l, _ in lanes)
        if width == "own":
            own.append((total, off, vreg, ls, per_loop_of(c, vreg, ls)))
            continue
        p("    s_load_%s %s, %s -> %s lanes %d-%d (%d words): %d reads" % (width, base, off, vreg, ls[0], ls[-1], len(ls), total))
        per_loop = collections.Counter()
        for l in ls:
            for (v2, l2, h), n in c["lane_reads_loop"].items():
                if v2 == vreg and l2 == l:
                    per_loop[h] += n
        for h, n in per_loop.most_common(6):
            p("        loop %-12s depth %d: %d" % (h, c["loop_depth"].get(h, 0), n))
        p("        per word: " + " ".join("%d:%d" % (w, c["lane_reads"][(vreg, l)]) for l, w in sorted(lanes, key=lambda t: t[1])))
    if own:
        p("")
        p("launch arguments made single values at kernel entry (own_sreg, in the order of split_args): %d spilled, %d reads in all" % (
            len(own), sum(o[0] for o in own)))
        tot = collections.Counter()
        for total, off, vreg, ls, per_loop in own:
            tot.update(per_loop)
            p("    %-4s %s lanes %s: %d reads (%s)" % (off, vreg, ",".join(str(l) for l in ls), total,
                                                   ", ".join("%s %d" % (h, n) for h, n in per_loop.most_common(4))))
        p("    by loop: " + ", ".join("%s (depth %d) %d" % (h, c["loop_depth"].get(h, 0), n) for h, n in tot.most_common(8)))
    p("")
    by_depth = collections.Counter()
    for n, d, _h, _v, _l in c["runs"]:
        by_depth[d] += n
    p("runs of >= 4 reads of consecutive lanes: %d runs, %d reads (%d of them at loop depth >= 3)" % (
        len(c["runs"]), sum(r[0] for r in c["runs"]), sum(n for d, n in by_depth.items() if d >= 3)))
    hist = collections.Counter(r[0] for r in c["runs"])
    p("    run length: count   " + "  ".join("%d: %d" % (k, hist[k]) for k in sorted(hist)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", help="device assembly listing (-S)")
    ap.add_argument("--kernel", default="solve_kernelILi10ELb1ELi3ELb0E", help="substring of the mangled kernel name")
    a = ap.parse_args()
    lines = [ln.rstrip("\n") for ln in open(a.asm)]
    body, name = kernel_body(lines, a.kernel)
    report(name, census(body), sys.stdout)


if __name__ == "__main__":
    main()
