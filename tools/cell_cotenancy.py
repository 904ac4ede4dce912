"""How many BiLSTM cell workgroups share a CU at one time, from the cell kernel's own stamps (Engine(debug_stamps=True):
s_memrealtime at entry / exit, HW_ID, XCC_ID per workgroup), on the PIPELINED fp32 step (eight forwards in flight, three-step
joint model, 512 sites per forward), and what the cell prologue costs (serial engine, one mid diagonal).

A cell workgroup is four waves, one per SIMD. A CU whose SIMDs hold two fused-module waves (2 x 184 VGPRs) has 144 registers
left per SIMD: one cell workgroup at 88 VGPRs, two at 72 ("Sharing a CU"). The module kernel's stamps carry no
HW_ID, so a module's presence on a CU is not observed directly; what is observed is, per launch, the number of cell workgroups
of that launch alive on one CU at the same moment and the K-loop time of each (a cell beside a module shares the matrix pipe:
its loop runs 2 - 3 x longer than alone).

usage: python tools/cell_cotenancy.py [passes=16] > out.json"""
import json, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from deepsignal_amd import synth, weights as W
from deepsignal_amd.engine import Engine

B, NDIAG = 512, 19
passes = int(sys.argv[1]) if len(sys.argv) > 1 else 16
w = W.random_weights(seed=1)
keys = ("kmer", "means", "stds", "sanums", "signals")


def stamps(e, d):
    s = e.intermediate("lstm_rawstamps%d" % d, (1024, 8))
    s = s[s[:, 7] > 0]
    # a record another forward overwrote half-way (entry of one forward, exit of another) is dropped
    return s[(s[:, 4] > s[:, 0]) & (s[:, 4] - s[:, 0] < 1e5)]


def pct(a, q=(10, 50, 90)):
    return [int(x) for x in np.percentile(a, q)] if len(a) else []


out = {"what": __doc__.split("\n\n")[0], "batch": B}

# ---- prologue cost, GPU to itself: one mid diagonal (two light layer-0 cells with K = 256, four K = 512 cells)
e = Engine(max_batch=B, slots=1, serial=True, debug_stamps=True, fold_fc=False)
e.load_weights(w)
e.set_graph(False)
f = synth.synthetic_features(B, seed=2)
args = [f[k] for k in keys]
for _ in range(4):
    e.run(*args)
s = stamps(e, 8)
e.close()
# the two layer-0 cells are a third of a full diagonal's workgroups and have the shortest K loops (K = 256 against 512)
light = np.zeros(len(s), dtype=bool)
light[np.argsort(s[:, 2])[:len(s) // 3]] = True
per_cu = {}
for k in s[:, 5].astype(int):
    per_cu[k] = per_cu.get(k, 0) + 1
out["serial_diagonal_8"] = {
    "workgroups": int(len(s)), "cus": len(per_cu), "most_workgroups_on_one_cu": max(per_cu.values()),
    "prologue_cycles_p10_p50_p90": {"layer0_cells_K256": pct(s[light, 1]), "other_cells_K512": pct(s[~light, 1])},
    "k_loop_cycles_p10_p50_p90": {"layer0_cells_K256": pct(s[light, 2]), "other_cells_K512": pct(s[~light, 2])},
    "life_us_p10_p50_p90": [round(float(x) * 0.01, 2) for x in np.percentile(s[:, 4] - s[:, 0], (10, 50, 90))]}

# ---- pipelined step: `passes` forwards of 512 sites in one call, the library keeps eight in flight
e = Engine(max_batch=B, debug_stamps=True, fold_fc=False)
e.load_weights(w)
f = synth.synthetic_features(passes * B, seed=3)
args = [f[k] for k in keys]
e.run(*args)
e.run(*args)
hist, loops = {}, {}
most = 0
for d in range(NDIAG):
    s = stamps(e, d)
    for k in np.unique(s[:, 5]):
        g = s[s[:, 5] == k]
        mid = 0.5 * (g[:, 0] + g[:, 4])
        # workgroups of this launch alive on this CU at each workgroup's mid-life (itself included)
        alive = ((g[None, :, 0] <= mid[:, None]) & (g[None, :, 4] >= mid[:, None])).sum(axis=1)
        for a, l in zip(alive, g[:, 2]):
            hist[int(a)] = hist.get(int(a), 0) + 1
            loops.setdefault(int(a), []).append(float(l))
        most = max(most, int(alive.max()))
e.close()
tot = sum(hist.values())
out["pipelined"] = {
    "forwards_in_one_call": passes, "diagonals": NDIAG, "workgroups_seen": tot, "most_alive_on_one_cu": most,
    "share_of_workgroups_by_same_launch_cells_alive_on_their_cu": {str(k): round(v / tot, 4) for k, v in sorted(hist.items())},
    "k_loop_cycles_p10_p50_p90_by_that_count": {str(k): pct(np.array(v)) for k, v in sorted(loops.items())}}
print(json.dumps(out))
