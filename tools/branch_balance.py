"""Which branch of the forward the joint model waits for, and how the launches of several forwards overlap, from the kernel
trace of a PIPELINED fp32 three-step run:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --gpus 1 --steps 100 --warmup 10
    python3 tools/branch_balance.py DIR [warmup forwards to drop = 10] > profiles/branch_balance_<build>.json

(kernel trace only: a counter run serialises the launches and is not a picture of the mix.)

A forward is 19 BiLSTM cell launches (the event branch), `stem1`, `stem23`, 3 fused-chain launches and `avgpool7` (the signal
branch), then the dense 6032 x 6032 launch and `head` behind the join. The trace does not say which forward a launch belongs to;
the host submits one forward at a time, so per hardware queue and kernel class the launches come forward by forward in dispatch
order: consecutive groups of 19 / 3 / 1 launches of a class on a queue are one forward's, and the f-th group of every class in
dispatch order is forward f. The grouping is CHECKED against the graph's own dependencies (the 19 cells one behind the other, dense
behind both branches, head behind dense); forwards that fail the check are counted and left out of the statistics. The check
allows SLACK_NS: the profiler's end stamp of a launch and the start stamp of its dependent overlap by up to 0.3 us.

join_wait = end of the 19th cell launch - end of avgpool7_kernel. Positive: dense waited for the BiLSTM."""
import csv
import glob
import json
import os
import sys

PER_FORWARD = {"cell": 19, "chain": 3, "stem1": 1, "stem23": 1, "avgpool7": 1, "dense": 1, "head": 1}
DENSE = "gemm_kernel<1,3,4,1,0,2,2,1"
SLACK_NS = 1000


def short(name):
    n = name.replace("void ", "").replace("ds::", "").replace(" ", "")
    cut = n.find("(")
    return n[:cut] if cut > 0 else n


def classify(s):
    if s.startswith("lstm_cell"):
        return "cell"
    if s.startswith("inception_fused_kernel"):
        return "chain"
    if s.startswith(DENSE):
        return "dense"
    for k in ("stem1", "stem23", "avgpool7", "head"):
        if s.startswith(k + "_kernel"):
            return k
    return None


def pctl(v, q):
    v = sorted(v)
    if not v:
        return None
    x = (len(v) - 1) * q / 100.0
    lo = int(x)
    hi = min(lo + 1, len(v) - 1)
    return v[lo] + (v[hi] - v[lo]) * (x - lo)


def load(path):
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            raise SystemExit("no *kernel_trace.csv under %s" % path)
        path = found[-1]
    rows = []
    for r in csv.DictReader(open(path)):
        s = short(r["Kernel_Name"])
        rows.append({"name": s, "cls": classify(s), "queue": r["Queue_Id"], "disp": int(r["Dispatch_Id"]),
                     "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"])})
    rows.sort(key=lambda r: r["disp"])
    return path, rows


def forwards_of(rows):
    """class -> list of groups (each a list of launches in dispatch order), groups in dispatch order"""
    groups = {}
    for cls, cnt in PER_FORWARD.items():
        per_queue = {}
        for r in rows:
            if r["cls"] == cls:
                per_queue.setdefault(r["queue"], []).append(r)
        g = []
        for q, lst in per_queue.items():
            for i in range(0, len(lst) - cnt + 1, cnt):
                g.append(lst[i:i + cnt])
        g.sort(key=lambda grp: grp[0]["disp"])
        groups[cls] = g
    n = min(len(g) for g in groups.values())
    return [{cls: groups[cls][f] for cls in PER_FORWARD} for f in range(n)], {cls: len(g) for cls, g in groups.items()}


def consistent(fw):
    after = lambda later, earlier: later["t0"] + SLACK_NS >= earlier["t1"]
    c, ch = fw["cell"], fw["chain"]
    d, h, a = fw["dense"][0], fw["head"][0], fw["avgpool7"][0]
    signal = [fw["stem1"][0], fw["stem23"][0]] + ch + [a]
    return all(after(c[i + 1], c[i]) for i in range(len(c) - 1)) and all(after(signal[i + 1], signal[i]) for i in range(len(signal) - 1)) \
        and after(d, c[-1]) and after(d, a) and after(h, d)


def main():
    path, rows = load(sys.argv[1])
    drop = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    fws, seen = forwards_of(rows)
    fws = fws[drop:]
    good = [fw for fw in fws if consistent(fw)]
    if not good:
        raise SystemExit("no forward passes the dependency check: %s" % seen)
    w0 = min(r["t0"] for fw in good for g in fw.values() for r in g)
    w1 = max(r["t1"] for fw in good for g in fw.values() for r in g)
    us = lambda t: round(t / 1e3, 2)
    per_forward, waits, dense_gap = [], [], []
    for fw in good:
        a1, c1, d0 = fw["avgpool7"][0]["t1"], fw["cell"][-1]["t1"], fw["dense"][0]["t0"]
        per_forward.append({"avgpool7_end_us": us(a1 - w0), "cell19_end_us": us(c1 - w0), "dense_start_us": us(d0 - w0)})
        waits.append((c1 - a1) / 1e3)
        dense_gap.append((d0 - max(a1, c1)) / 1e3)
    # the mix: every kernel of the process inside the window of the forwards kept
    inwin = [r for r in rows if r["t1"] > w0 and r["t0"] < w1]
    durs, durs_cls = {}, {}
    for r in inwin:
        durs.setdefault(r["name"], []).append((r["t1"] - r["t0"]) / 1e3)
        if r["cls"]:
            durs_cls.setdefault(r["cls"], []).append((r["t1"] - r["t0"]) / 1e3)
    ev = []
    for r in inwin:
        ev.append((max(r["t0"], w0), 1))
        ev.append((min(r["t1"], w1), -1))
    ev.sort()
    share, depth, last = {}, 0, w0
    for t, d in ev:
        share[depth] = share.get(depth, 0) + (t - last)
        last, depth = t, depth + d
    share[depth] = share.get(depth, 0) + (w1 - last)
    in_flight = {}
    for k, v in sorted(share.items()):
        key = str(k) if k < 5 else "5+"
        in_flight[key] = round(in_flight.get(key, 0.0) + v / (w1 - w0), 4)
    queues = {}
    for q in sorted({r["queue"] for r in inwin}):
        iv = sorted((max(r["t0"], w0), min(r["t1"], w1)) for r in inwin if r["queue"] == q)
        busy, cur0, cur1 = 0, iv[0][0], iv[0][1]
        for a, b in iv[1:]:
            if a > cur1:
                busy += cur1 - cur0
                cur0, cur1 = a, b
            else:
                cur1 = max(cur1, b)
        busy += cur1 - cur0
        queues[q] = {"busy_share": round(busy / (w1 - w0), 4), "launches": len(iv)}
    cell_chain = [(fw["cell"][-1]["t1"] - fw["cell"][0]["t0"]) / 1e3 for fw in good]
    signal = [(fw["avgpool7"][0]["t1"] - fw["stem1"][0]["t0"]) / 1e3 for fw in good]
    out = {
        "what": "branch balance of the pipelined fp32 three-step forward from a rocprofv3 kernel trace (tools/branch_balance.py)",
        "trace": os.path.basename(path), "launch_groups_seen": seen, "warmup_forwards_dropped": drop,
        "forwards": len(fws), "forwards_passing_the_dependency_check": len(good),
        "window_us": us(w1 - w0), "us_per_forward_in_window": us((w1 - w0) / len(good)),
        "join_wait_us": {"definition": "end of the 19th cell launch - end of avgpool7_kernel; positive = the joint model waited for the BiLSTM",
                         "median": round(pctl(waits, 50), 2), "p90": round(pctl(waits, 90), 2), "p10": round(pctl(waits, 10), 2),
                         "share_positive": round(sum(1 for x in waits if x > 0) / len(waits), 4)},
        "dense_start_behind_the_later_branch_us": {"median": round(pctl(dense_gap, 50), 2), "p90": round(pctl(dense_gap, 90), 2)},
        "event_branch_first_cell_start_to_last_cell_end_us": {"median": round(pctl(cell_chain, 50), 1), "p90": round(pctl(cell_chain, 90), 1)},
        "signal_branch_stem1_start_to_avgpool7_end_us": {"median": round(pctl(signal, 50), 1), "p90": round(pctl(signal, 90), 1)},
        "median_in_mix_duration_us": {"by_class": {k: round(pctl(v, 50), 2) for k, v in sorted(durs_cls.items())},
                                      "by_kernel": {k: {"median": round(pctl(v, 50), 2), "launches": len(v)} for k, v in sorted(durs.items())}},
        "share_of_time_with_n_kernels_in_flight": in_flight,
        "queues": queues,
        "per_forward": per_forward,
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
