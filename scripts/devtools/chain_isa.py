#!/usr/bin/env python3
"""The per-wave chain of the AnyMDP bucket step, counted in hipcc's assembly ("the per-wave chain").

  python scripts/devtools/chain_isa.py [anymdp.s]

Without an argument it compiles xenoverse_amd/csrc/anymdp.hip device-only to assembly with the build's flags in a temporary
directory (no GPU needed).  For every instantiation of anymdp_step_kernel<false, 1, false, true, 1, HAND, ...> — the graph-node
kernels of xv_anymdp_step_many under the bucket search at S <= 112: HAND = the overlapped path, otherwise one stream — it prints

  front   vector instructions from the exit of the poll loop (one stream: from the first wait for the link-1 loads) to the
          first line-index ds_bpermute, and which of them are transcendental or fp64
  line    ds_bpermutes in front of the first line load, and the LDS waits between the first bpermute and the last line load
  tail    vector instructions and scalar loads from the last wait for the line to the record store (one stream: to the first
          output store), along the straight path: a forward conditional branch over a region that loads from memory (the
          fence fall-back, the stuck-env observation) is taken, any other falls through
  occ     the kernel's occupancy as hipcc reports it

with the line numbers of the marks, so that a reader can check them against the file.  A tool for a person: the marks are
heuristics over one compiler's output, not an interface."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNEL = re.compile(r"^(_Z18anymdp_step_kernelILb0ELi1ELb0ELb1ELi1ELb([01])E(?:Li(n?\d+)E)?Ev\w*):")
SLOW = re.compile(r"f64|v_(log|exp|sqrt|rsq|rcp|sin|cos)_")


def compile_asm(out):
    sys.path.insert(0, ROOT)
    from xenoverse_amd import build
    cmd = [build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", os.path.join(ROOT, "xenoverse_amd", "csrc", "anymdp.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def kernel_body(lines, start):
    """[(file line number, label or None, opcode, operand string)] of the kernel, and its occupancy"""
    body, occ, i = [], None, start + 1
    while i < len(lines) and not lines[i].strip().startswith(".Lfunc_end"):
        ln = lines[i].split(";")[0].rstrip()
        m = re.match(r"^(\.L\w+):", ln)
        if m:
            body.append((i + 1, m.group(1), None, ""))
        elif ln.strip() and not ln.strip().startswith("."):
            tok = ln.split(None, 1)
            body.append((i + 1, None, tok[0], tok[1] if len(tok) > 1 else ""))
        i += 1
    for j in range(i, min(i + 80, len(lines))):
        m = re.search(r"; Occupancy: (\d+)", lines[j])
        if m:
            occ = int(m.group(1))
            break
    return body, occ


def straight_path(body, i0, stop):
    """indices of the instructions executed from i0 until stop(op, args) holds, fall-back regions skipped"""
    where = {lab: k for k, (_, lab, _, _) in enumerate(body) if lab}
    path, k = [], i0
    while k < len(body):
        _, lab, op, args = body[k]
        if op is None:
            k += 1
            continue
        path.append(k)
        if stop(op, args):
            break
        tgt = args.split()[-1] if args else ""
        if op == "s_branch" and where.get(tgt, -1) > k:
            k = where[tgt]
            continue
        if op.startswith("s_cbranch") and where.get(tgt, -1) > k and any(
                (body[q][2] or "").startswith("global_load") for q in range(k + 1, where[tgt])):
            k = where[tgt]
            continue
        k += 1
    return path


def report(lines, start, name, hand):
    body, occ = kernel_body(lines, start)
    ops = [b[2] or "" for b in body]
    where = {lab: k for k, (_, lab, _, _) in enumerate(body) if lab}
    if hand:      # the exit of the poll loop: behind the last backward branch that follows the s_sleep
        sl = ops.index("s_sleep")
        k0 = max(k for k in range(sl, len(body)) if ops[k].startswith(("s_branch", "s_cbranch")) and
                 where.get(body[k][3].split()[-1], len(body)) < sl) + 1
        mark0 = "poll-loop exit"
    else:
        first_load = next(k for k in range(len(body)) if ops[k].startswith("global_load"))
        k0 = next(k for k in range(first_load, len(body)) if ops[k] == "s_waitcnt" and "vmcnt" in body[k][3]) + 1
        mark0 = "first link-1 wait"
    bp = next(k for k in range(k0, len(body)) if ops[k] == "ds_bpermute_b32")
    front = [k for k in range(k0, bp) if ops[k].startswith("v_")]
    slow = [ops[k] for k in front if SLOW.search(ops[k])]
    print("%s\n  %s" % (name, "HAND (overlapped)" if hand else "one stream"))
    print("  front  %3d vector instructions, %s (line %d) -> first line-index bpermute (line %d); transcendental / fp64: %s"
          % (len(front), mark0, body[k0][0], body[bp][0], ", ".join(slow) if slow else "none"))
    loads = [k for k in range(bp, len(body)) if ops[k] == "global_load_dwordx4"][:8]
    waits = [k for k in range(bp, loads[-1]) if ops[k] == "s_waitcnt" and "lgkmcnt" in body[k][3]]
    ahead = sum(1 for k in range(bp, loads[0]) if ops[k] == "ds_bpermute_b32")
    print("  line   %d bpermutes in front of the first line load (line %d), %d LDS waits up to the last line load (line %d): %s"
          % (ahead, body[loads[0]][0], len(waits), body[loads[-1]][0], ", ".join(body[k][3] for k in waits)))
    if hand:
        stop, end_name = (lambda op, a: op == "global_store_dwordx2" and "sc1" in a), "record store"
    else:
        stop, end_name = (lambda op, a: op.startswith("global_store")), "first output store"
    path = straight_path(body, loads[-1] + 1, stop)
    lw = next((p for p in path if ops[p] == "s_waitcnt" and "vmcnt(0)" in body[p][3]), path[0])      # every line is there
    tail = path[path.index(lw) + 1:]
    print("  tail   %3d vector instructions, %d scalar loads, last line wait (line %d) -> %s (line %d)"
          % (sum(1 for k in tail if ops[k].startswith("v_")), sum(1 for k in tail if ops[k].startswith("s_load")),
             body[lw][0], end_name, body[path[-1]][0]))
    print("  occ    %s" % occ)


def main():
    if len(sys.argv) > 1:
        text = open(sys.argv[1]).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            compile_asm(os.path.join(d, "anymdp.s"))
            text = open(os.path.join(d, "anymdp.s")).read()
    lines = text.splitlines()
    found = 0
    for i, ln in enumerate(lines):
        m = KERNEL.match(ln)
        if m:
            mode = {None: "", "n1": ", mode: argument", "0": ", mode: DISABLED", "1": ", mode: NEXT_STEP", "2": ", mode: SAME_STEP"}[m.group(3)]
            report(lines, i, m.group(1) + mode, m.group(2) == "1")
            found += 1
    if not found:
        sys.exit("no anymdp_step_kernel<false, 1, false, true, 1, ...> in the assembly")


if __name__ == "__main__":
    main()
