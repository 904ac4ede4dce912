"""How far the BiLSTM branch of one forward runs ahead of the joint model of the forwards before it, from the kernel trace of a
PIPELINED fp32 three-step run (the trace and the grouping of launches into forwards are those of tools/branch_balance.py):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --gpus 1 --steps 100 --warmup 10
    python3 tools/run_ahead.py DIR [warmup forwards to drop = 10] > profiles/run_ahead_<build>.json

(kernel trace only: a counter run serialises the launches.)

The question: while a forward's dense 6032 x 6032 launch runs, is a cell launch of a LATER forward beside it? The cell launches of
the slots that share a hardware queue come one forward behind the other, so per cell queue the tool looks at consecutive forwards
(prev, next) on that queue:

  cell_gap          first cell start of next - last cell end of prev            (the queue carries no cell launch for that long)
  cells_vs_dense    first cell start of next - dense END of prev                (negative: next's cells started while prev's dense ran
                                                                                 or earlier -- they ran ahead)
  gather_vs_dense   first gather_inputs_kernel start of next - dense END of prev (where the next forward's inputs were copied)

and over the whole window: the share of time with no cell launch in flight, the share of dense-launch time with fewer than one /
fewer than two cell launches in flight, the busy share of every queue, and the join wait of branch_balance.py.

gather_inputs_kernel launches are matched to forwards in dispatch order (match_gathers); forwards whose gather fails the order
check are counted and left out of gather_vs_dense, so read that figure beside the count.

WHAT THE PAIRS CANNOT SHOW. The pairs are consecutive forwards on ONE cell queue. When the engine has as many slots as there are
hardware queues (four slots on four queues: each queue carries one slot's event stream), the two forwards of a pair are the SAME
slot's, and the slot-reuse edge makes the later one's cells wait for the earlier one's dense, head and scatter: cells_vs_dense
is then positive by construction and says nothing about run-ahead. The tool cannot see slots in a trace; it reports
forwards_between_the_forwards_of_a_pair (1: every other forward, two slots' event streams share the queue; 3: every fourth, one
slot per queue with four queues) so that the case is visible, and the run-ahead question is then answered only by
later_forwards_with_cells_running_during_a_dense and the shares of dense-launch time, which look across all queues.

The grouping is branch_balance.py's and has its limit: its dependency check would also accept the cells of forward f grouped with
the dense of a later forward f + k, since that dense starts behind those cells as well; what protects against it is only that
every class has the same number of groups and the host issues one forward at a time."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from branch_balance import consistent, forwards_of, load, pctl  # noqa: E402


def stats(v):
    if not v:
        return None
    return {"median": round(pctl(v, 50), 2), "p10": round(pctl(v, 10), 2), "p90": round(pctl(v, 90), 2), "min": round(min(v), 2),
            "max": round(max(v), 2), "share_negative": round(sum(1 for x in v if x < 0) / len(v), 4), "pairs": len(v)}


def match_gathers(rows, fws):
    """forward index -> start of its first gather launch (ns), and the launches per forward. The host issues one forward at a
    time with its gather launches first, so in dispatch order the f-th group of k gather launches is forward f's; CHECKED: no
    gather of a forward may start after that forward's first cell or its stem1 launch (such forwards are left out and counted)."""
    gathers = [r for r in rows if r["name"].startswith("gather_inputs_kernel")]
    if not gathers or not fws:
        return {}, 0, 0
    k = int(round(len(gathers) / float(len(fws))))
    start, bad = {}, 0
    for f, fw in enumerate(fws):
        g = gathers[f * k:(f + 1) * k]
        if len(g) < max(k, 1):
            break
        if max(r["t0"] for r in g) > min(fw["cell"][0]["t0"], fw["stem1"][0]["t0"]):
            bad += 1
            continue
        start[f] = min(r["t0"] for r in g)
    return start, k, bad


def covered(intervals, lo, hi):
    """{depth: ns} of [lo, hi) by how many of the intervals cover it"""
    ev = []
    for a, b in intervals:
        a, b = max(a, lo), min(b, hi)
        if a < b:
            ev.append((a, 1))
            ev.append((b, -1))
    ev.sort()
    out, depth, last = {}, 0, lo
    for t, d in ev:
        out[depth] = out.get(depth, 0) + (t - last)
        last, depth = t, depth + d
    out[depth] = out.get(depth, 0) + (hi - last)
    return out


def main():
    path, rows = load(sys.argv[1])
    drop = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    fws, seen = forwards_of(rows)
    gather_start, gathers_per_forward, gathers_bad = match_gathers(rows, fws)
    idx = [f for f in range(drop, len(fws)) if consistent(fws[f])]
    if not idx:
        raise SystemExit("no forward passes the dependency check: %s" % seen)
    good = [fws[f] for f in idx]
    w0 = min(r["t0"] for fw in good for g in fw.values() for r in g)
    w1 = max(r["t1"] for fw in good for g in fw.values() for r in g)

    per_queue = {}
    for f in idx:
        per_queue.setdefault(fws[f]["cell"][0]["queue"], []).append(f)
    queues_out, all_cd, between = {}, [], []
    for q, lst in sorted(per_queue.items()):
        gap, cd, gd, partner = [], [], [], set()
        between += [b - a - 1 for a, b in zip(lst, lst[1:])]
        for a, b in zip(lst, lst[1:]):
            prev, nxt = fws[a], fws[b]
            dense_end = prev["dense"][0]["t1"]
            partner.add(prev["dense"][0]["queue"])
            gap.append((nxt["cell"][0]["t0"] - prev["cell"][-1]["t1"]) / 1e3)
            cd.append((nxt["cell"][0]["t0"] - dense_end) / 1e3)
            if b in gather_start:
                gd.append((gather_start[b] - dense_end) / 1e3)
        all_cd += cd
        queues_out[q] = {"forwards": len(lst), "dense_queues_of_these_forwards": sorted(partner),
                         "cell_gap_us": stats(gap), "cells_vs_dense_us": stats(cd), "gather_vs_dense_us": stats(gd)}

    inwin = [r for r in rows if r["t1"] > w0 and r["t0"] < w1]
    cells = [(r["t0"], r["t1"]) for r in inwin if r["cls"] == "cell"]
    wall = covered(cells, w0, w1)
    dense_ns, dense_depth = 0, {}
    for r in inwin:
        if r["cls"] != "dense":
            continue
        lo, hi = max(r["t0"], w0), min(r["t1"], w1)
        dense_ns += hi - lo
        for k, v in covered(cells, lo, hi).items():
            dense_depth[k] = dense_depth.get(k, 0) + v
    busy = {}
    for q in sorted({r["queue"] for r in inwin}):
        c = covered([(r["t0"], r["t1"]) for r in inwin if r["queue"] == q], w0, w1)
        busy[q] = {"busy_share": round(1 - c.get(0, 0) / float(w1 - w0), 4), "carries_cells": q in per_queue,
                   "launches": sum(1 for r in inwin if r["queue"] == q)}
    waits = [(fw["cell"][-1]["t1"] - fw["avgpool7"][0]["t1"]) / 1e3 for fw in good]
    # how many LATER forwards have a cell launch running while a forward's dense runs
    later = []
    for f in idx:
        d = fws[f]["dense"][0]
        later.append(sum(1 for g in idx if g > f and fws[g]["cell"][0]["t0"] < d["t1"] and fws[g]["cell"][-1]["t1"] > d["t0"]))
    out = {
        "what": "run-ahead of the BiLSTM branch against the joint model of earlier forwards, from a rocprofv3 kernel trace (tools/run_ahead.py)",
        "trace": os.path.basename(path), "launch_groups_seen": seen, "warmup_forwards_dropped": drop,
        "forwards": len(fws) - drop, "forwards_passing_the_dependency_check": len(good),
        "gather_launches_per_forward": gathers_per_forward, "forwards_whose_gather_failed_its_order_check": gathers_bad,
        "window_us": round((w1 - w0) / 1e3, 2), "us_per_forward_in_window": round((w1 - w0) / 1e3 / len(good), 2),
        "per_cell_queue": queues_out,
        "cells_vs_dense_us_all_queues": stats(all_cd),
        "forwards_between_the_forwards_of_a_pair": {"median": pctl(between, 50), "min": min(between) if between else None, "max": max(between) if between else None,
                                                    "note": "a pair is two consecutive forwards on one cell queue. With one slot per queue (median = queues - 1) a pair is one "
                                                            "slot's two forwards, which the slot-reuse edge orders: cells_vs_dense is then positive by construction"},
        "cells_behind_the_previous_dense": "next forward's cells on the same queue start only after the previous dense ended in %.0f %% of the pairs"
                         % (100.0 * sum(1 for x in all_cd if x >= 0) / max(1, len(all_cd))),
        "share_of_wall_time_with_no_cell_launch_in_flight": round(wall.get(0, 0) / float(w1 - w0), 4),
        "share_of_dense_time_with_fewer_than_one_cell_launch_in_flight": round(dense_depth.get(0, 0) / float(max(1, dense_ns)), 4),
        "share_of_dense_time_with_fewer_than_two_cell_launches_in_flight":
            round((dense_depth.get(0, 0) + dense_depth.get(1, 0)) / float(max(1, dense_ns)), 4),
        "later_forwards_with_cells_running_during_a_dense": {"median": pctl(later, 50), "share_of_denses_with_any": round(sum(1 for x in later if x) / float(len(later)), 4)},
        "join_wait_us": {"definition": "end of the 19th cell launch - end of avgpool7_kernel; positive = the joint model waited for the BiLSTM",
                         "median": round(pctl(waits, 50), 2), "p10": round(pctl(waits, 10), 2), "p90": round(pctl(waits, 90), 2),
                         "share_positive": round(sum(1 for x in waits if x > 0) / len(waits), 4)},
        "queues": busy,
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
