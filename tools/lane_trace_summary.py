"""Concurrency of the F plan's kernels in the timed region of a plain bench.py run, from a
rocprofv3 kernel trace (--kernel-trace --output-format csv) of that run:

  python tools/lane_trace_summary.py <kernel_trace.csv> [--steps 100]

The timed region is the last --steps counting launches (k_f8_count32q) with the k_f8_tail_solve
launches between the end of the count before them and the last kernel of the trace.  Prints the
share of the region's wall time with no, one, and two or more kernels in flight, the mean kernel
durations, and the mean gap between successive count completions."""
import argparse
import csv
import json
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()

    ks = []
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            kind = ("count" if "k_f8_count32q" in name else
                    "tail_solve" if "k_f8_tail_solve" in name else None)
            if kind:
                ks.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind,
                           r.get("Queue_Id", "")))
    counts = sorted((k for k in ks if k[2] == "count"), key=lambda k: k[1])
    if len(counts) <= args.steps:
        raise SystemExit(f"{len(counts)} counting launches in the trace, need more than {args.steps}")
    t_begin = counts[-args.steps - 1][1]          # end of the last warm-up count
    region = sorted(k for k in ks if k[0] >= t_begin)
    # the flush after the warm-up launches its tails alone, then the host synchronises before the
    # first timed run: the region starts after the last such host gap (> 15 us with no kernel)
    # before the first timed count
    first_count = min(k[0] for k in region if k[2] == "count")
    lead = [k for k in region if k[2] == "tail_solve" and k[1] <= first_count]
    cut, end_so_far = 0, t_begin
    for i, k in enumerate(lead):
        if k[0] - end_so_far > 15_000:
            cut = i
        end_so_far = max(end_so_far, k[1])
    region = [k for k in region if k not in lead[:cut]]
    t0, t1 = min(k[0] for k in region), max(k[1] for k in region)

    edges = sorted([(k[0], 1) for k in region] + [(k[1], -1) for k in region])
    share = {0: 0, 1: 0, 2: 0}
    live, prev = 0, t0
    for t, d in edges:
        share[min(live, 2)] += t - prev
        prev = t
        live += d
    wall = t1 - t0

    def mean_us(kind):
        d = [k[1] - k[0] for k in region if k[2] == kind]
        return sum(d) / len(d) / 1e3

    ends = sorted(k[1] for k in region if k[2] == "count")
    gaps = [b - a for a, b in zip(ends, ends[1:])]
    out = {
        "trace": os.path.basename(args.trace),
        "steps": args.steps,
        "kernels_in_region": len(region),
        "queues": sorted({k[3] for k in region}),
        "region_us": wall / 1e3,
        "region_us_per_step": wall / 1e3 / args.steps,
        "share_no_kernel": share[0] / wall,
        "share_one_kernel": share[1] / wall,
        "share_two_or_more": share[2] / wall,
        "count32q_mean_us": mean_us("count"),
        "tail_solve_mean_us": mean_us("tail_solve"),
        "count_completion_gap_mean_us": sum(gaps) / len(gaps) / 1e3,
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
