"""Where a timed stitch step's time goes, from a rocprofv3 kernel trace of scripts/step_launches.py: the last step's launches on a time axis (kernel, workgroups,
hardware queue, start / end relative to the step's first dispatch), then per hardware queue the launches it ran and the time it was busy, and how many launches
started within 20 us of the end of the launch before them on the SAME queue (they waited for it: launches that share a queue run one after the other).
usage: python scripts/step_queue_summary.py TRACE_DIR STEP_JSON [STEPS]   (STEP_JSON: --json of step_launches.py, for the launches per step; STEPS: last steps summed, 3)"""
import csv
import glob
import json
import os
import sys


def main():
    d, step_json = sys.argv[1], sys.argv[2]
    n_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    step = json.load(open(step_json))
    per = len(step["launches"])
    f = (glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) or [None])[0]
    rows = [r for r in csv.DictReader(open(f)) if "popoa" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    tail = rows[-per * n_steps:]

    def name(r):
        return r["Kernel_Name"].split("::")[-1].split("(")[0].replace("(anonymous namespace)", "")

    def wg(r):
        return int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0) // max(1, int(r.get("Workgroup_Size", r.get("Workgroup_Size_X", 1)) or 1))

    print("step_launches.py: %.3f ms per step over its timed steps, %d launches per step" % (step["ms_per_step"], per))
    last = sorted(tail[-per:], key=lambda r: int(r["Start_Timestamp"]))
    t0 = min(int(r["Start_Timestamp"]) for r in last)
    print("\nthe last step, by start:")
    for r in last:
        print("  %-44s %6d wg  queue %-3s  start %8.1f us  end %8.1f us  (%7.1f us)" % (name(r)[:44], wg(r), r.get("Queue_Id", "?"), (int(r["Start_Timestamp"]) - t0) / 1e3,
                                                                                  (int(r["End_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    print("  span of the last step's launches: %.1f us" % ((max(int(r["End_Timestamp"]) for r in last) - t0) / 1e3))
    by_q = {}
    for r in tail:
        by_q.setdefault(r.get("Queue_Id", "?"), []).append(r)
    span = (max(int(r["End_Timestamp"]) for r in tail) - min(int(r["Start_Timestamp"]) for r in tail)) / 1e3
    print("\nthe last %d steps (%.1f us from the first start to the last end, %.1f us per step), per hardware queue:" % (n_steps, span, span / n_steps))
    total_waited = 0
    for q, rs in sorted(by_q.items()):
        rs.sort(key=lambda r: int(r["Start_Timestamp"]))
        busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rs) / 1e3
        waited = sum(1 for a, b in zip(rs, rs[1:]) if 0 <= int(b["Start_Timestamp"]) - int(a["End_Timestamp"]) <= 20000)
        overlapped = sum(1 for a, b in zip(rs, rs[1:]) if int(b["Start_Timestamp"]) < int(a["End_Timestamp"]))
        total_waited += waited
        print("  queue %-3s %4d launches  busy %8.1f us (%5.1f us per step)  started right behind the one before on the queue: %d, overlapping it: %d"
              % (q, len(rs), busy, busy / n_steps, waited, overlapped))
    kern = {}
    for r in tail:
        k = kern.setdefault(name(r), [0, 0.0])
        k[0] += 1
        k[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    print("\nper kernel over the last %d steps (launches, summed duration per step):" % n_steps)
    for k, (c, us) in sorted(kern.items(), key=lambda kv: -kv[1][1]):
        print("  %-44s %4d  %8.1f us" % (k[:44], c, us / n_steps))
    print("\nsummed launch durations per step %.1f us; launches that started right behind the one before on their queue: %d of %d"
          % (sum(v[1] for v in kern.values()) / n_steps, total_waited, len(tail)))


if __name__ == "__main__":
    main()
