"""Split a rocprofv3 kernel trace (`--kernel-trace --output-format csv`) into the calls of
dsu_mesh_decimate_parallel it holds and print, per call: the durations of claim_kernel and
collapse_kernel in launch order, one line per (round, pass), and the summed time of every other
kernel the call launches (owner flags, selects, edge cost, radix sort, CSR rebuild, quadrics).
Memsets and copies are not kernels of the trace; they show in the call's span (first kernel start
to last kernel end, which also holds the host's waits between rounds).
    python tools/remesh_rounds_trace.py <folder or *_kernel_trace.csv> [passes per round = 4]"""
import csv
import os
import sys
from collections import OrderedDict

OWN = ("flag_nondegenerate_kernel", "degree_kernel", "fill_kernel", "sort_lists_kernel", "init_quadrics_kernel",
       "owner_flags_kernel", "edge_cost_kernel", "claim_kernel", "collapse_kernel", "iota_kernel")
PRIMITIVES = ("rocprim", "hipcub")          # scans, selects and the radix sort


def short(name):
    for k in OWN:
        if k in name:
            return k
    for tag in ("radix", "scan", "partition", "select", "lookback", "histogram", "sort"):
        if tag in name.lower():
            return "primitives: " + tag
    return "primitives: other"


def find_trace(path):
    if os.path.isfile(path):
        return path
    for root, _, files in os.walk(path):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                return os.path.join(root, f)
    raise SystemExit("no *kernel_trace.csv under " + path)


def calls(rows):
    """rows sorted by start: [(name, start, end)] -> list of calls, each a list of rows"""
    is_own = lambda n: any(k in n for k in OWN)
    is_prim = lambda n: any(k in n for k in PRIMITIVES)
    starts = [i for i, r in enumerate(rows) if "flag_nondegenerate_kernel" in r[0]]
    out = []
    for a, b in zip(starts, starts[1:] + [len(rows)]):
        seg = rows[a:b]
        last = max(i for i, r in enumerate(seg) if is_own(r[0]))
        while last + 1 < len(seg) and is_prim(seg[last + 1][0]):   # the select after the last round
            last += 1
        # kernels of other streams that fall inside the call are not its own
        out.append([r for r in seg[:last + 1] if is_own(r[0]) or is_prim(r[0])])
    return out


def main():
    path = find_trace(sys.argv[1])
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[1])
    for ci, call in enumerate(calls(rows)):
        claim = [(e - s) / 1e3 for n, s, e in call if "claim_kernel" in n]
        coll = [(e - s) / 1e3 for n, s, e in call if "collapse_kernel" in n]
        other = OrderedDict()
        for n, s, e in call:
            k = short(n)
            if k in ("claim_kernel", "collapse_kernel"):
                continue
            t, c = other.get(k, (0.0, 0))
            other[k] = (t + (e - s) / 1e3, c + 1)
        span = (call[-1][2] - call[0][1]) / 1e3
        total = sum((e - s) / 1e3 for _, s, e in call)
        print("call %d: %d kernels, %.1f us of kernels in a span of %.1f us" % (ci, len(call), total, span))
        print("  claim_kernel %d launches %.1f us (max %.1f); collapse_kernel %d launches %.1f us (max %.1f); "
              "together %.1f us" % (len(claim), sum(claim), max(claim, default=0.0), len(coll), sum(coll),
                                    max(coll, default=0.0), sum(claim) + sum(coll)))
        print("  round pass   claim us  collapse us")
        for i, (a, b) in enumerate(zip(claim, coll)):
            print("  %5d %4d %10.1f %12.1f" % (i // passes, i % passes, a, b))
        print("  every other kernel of the call: %.1f us" % sum(t for t, _ in other.values()))
        for k, (t, c) in sorted(other.items(), key=lambda kv: -kv[1][0]):
            print("    %-28s %5d launches %10.1f us" % (k, c, t))


if __name__ == "__main__":
    main()
