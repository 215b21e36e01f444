"""rocprofv3 --kernel-trace CSV of `python bench.py --gpus 1 --steps 3 --warmup 1` -> the serial chain of one game group and wave as JSON:
k_wave_trunk -> k_dense1_mfma -> k_tail (two heads launches) or k_wave_trunk -> k_heads_c4 (one), per hardware queue (a game group's stream).
Per chain: begin and end of each kernel and how long each heads kernel sits between the previous kernel's end and its own end (its wait
for a slot behind the other group's trunk tiles + its run).  Only the headline's launch shape is kept: the most frequent workgroup count
of k_wave_trunk.  Also the idle slot time per wave: slots x period of a group, minus the slot time of the workgroups of all groups, ESTIMATED per
launch shape — trunk workgroups x 3 boards x 46 us per board and slot, tree blocks x 65 us, heads workgroups x the
kernel's shortest launch (an uncontended launch is one round of workgroups).
usage: python tools/heads_chain.py <kernel_trace.csv> [games_per_group] > out.json"""
import csv
import json
import statistics
import sys
from collections import Counter, defaultdict

SLOTS = 512                      # 256 CUs x 2 resident workgroups
TRUNK_WG_US = 3 * 46.0           # a 3-board trunk tile
TREE_WG_US = 65.0                # a tree block of 16 games
HEADS = ("k_dense1_mfma", "k_tail", "k_heads_c4")


def short(name):
    for k in ("k_wave_trunk",) + HEADS:
        if k in name:
            return k
    return None


def summary(v):
    v = sorted(v)
    return {"n": len(v), "mean": round(statistics.fmean(v), 2), "median": round(statistics.median(v), 2), "min": round(v[0], 2), "max": round(v[-1], 2)} if v else {"n": 0}


def main():
    games_per_group = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    queues = defaultdict(list)
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            if k:
                wg = int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"])
                grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
                queues[r["Queue_Id"] + "/" + r.get("Stream_Id", "")].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k, grid // max(wg, 1)))
    shape = Counter(e[3] for q in queues.values() for e in q if e[2] == "k_wave_trunk").most_common(1)[0][0]
    chains = []                  # (queue, [kernel events])
    for qid, ev in queues.items():
        ev.sort()
        i = 0
        while i < len(ev):
            if ev[i][2] == "k_wave_trunk" and ev[i][3] == shape:
                j = i + 1
                while j < len(ev) and ev[j][2] in HEADS:
                    j += 1
                if j > i + 1:
                    chains.append((qid, ev[i:j]))
                i = j
            else:
                i += 1
    us = lambda ns: ns / 1e3
    stat = defaultdict(list)
    heads_wg = {}
    last_start = {}
    for qid, c in sorted(chains, key=lambda qc: qc[1][0][0]):
        stat["k_wave_trunk_us"].append(us(c[0][1] - c[0][0]))
        for prev, e in zip(c, c[1:]):
            stat[e[2] + "_run_us"].append(us(e[1] - e[0]))
            stat[e[2] + "_gap_before_start_us"].append(us(e[0] - prev[1]))
            stat[e[2] + "_prev_end_to_own_end_us"].append(us(e[1] - prev[1]))
            heads_wg[e[2]] = e[3]
        stat["heads_trunk_end_to_last_end_us"].append(us(c[-1][1] - c[0][1]))
        stat["chain_us"].append(us(c[-1][1] - c[0][0]))
        if qid in last_start and c[0][0] - last_start[qid] < 5e6:      # (a pause of the host between steps is no period)
            stat["period_us"].append(us(c[0][0] - last_start[qid]))
        last_start[qid] = c[0][0]
    groups = len({q for q, _ in chains})
    period = statistics.median(stat["period_us"])
    tree_wg = games_per_group // 16
    used = groups * ((shape - tree_wg) * TRUNK_WG_US + tree_wg * TREE_WG_US + sum(heads_wg[k] * min(stat[k + "_run_us"]) for k in heads_wg))
    t0 = min(c[0][0] for _, c in chains)
    out = {
        "what": "rocprofv3 --kernel-trace of python bench.py --gpus 1 --steps 3 --warmup 1; chains of the headline launch shape, microseconds",
        "k_wave_trunk_workgroups": shape, "heads_workgroups": heads_wg, "groups": groups, "chains": len(chains),
        "stats": {k: summary(v) for k, v in sorted(stat.items())},
        "idle_slot_time": {"slots": SLOTS, "period_us": round(period, 1), "slot_us_per_wave": round(SLOTS * period), "estimated_workgroup_us_per_wave": round(used),
                           "idle_share": round(1 - used / (SLOTS * period), 4),
                           "estimate": "groups x (trunk workgroups x 138 us + tree blocks x 65 us + heads workgroups x the kernel's shortest launch)"},
        # the middle of the trace (the timed steps), both groups interleaved: [queue, [kernel, begin, end] ...], us from the first chain of the trace
        "sample_chains": [[q, [[e[2], round(us(e[0] - t0), 1), round(us(e[1] - t0), 1)] for e in c]]
                          for q, c in sorted(chains, key=lambda qc: qc[1][0][0])[len(chains) // 2:len(chains) // 2 + 12]],
    }
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
