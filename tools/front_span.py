#!/usr/bin/env python3
"""front_span.py TRACE.csv [--skip N] [--steps]

Reads the kernel trace of a bench run (`rocprofv3 --kernel-trace --output-format csv -- python bench.py ...`, the
*_kernel_trace.csv) and prints, for the front half of every scan step (matcher, NDT, proposal frame, samples, weighting):

  span      first match_kernel start to last propose_weight_kernel end
  two       the part of that span during which dispatches of two different kernels were in flight
  ndt_early whether an ndt_kernel began before the step's last match_kernel ended

and the medians over the steps (--skip N leaves the first N steps, the warm-up, out of the medians; --steps prints every
step).  Pure Python: no GPU, no package of the project."""
import argparse
import csv
import statistics

FRONT = ("match_kernel", "ndt_kernel", "propose_prep_kernel", "propose_samples_kernel", "propose_weight_kernel")


def short(name):
    """rbpf::match_kernel(rbpf::DevView, rbpf::MatchArgs) -> match_kernel"""
    return name.split("(")[0].split("::")[-1].strip()


def read_trace(path):
    """[(start ns, end ns, kernel)] of every kernel dispatch, by start"""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if r.get("Kind", "KERNEL_DISPATCH") != "KERNEL_DISPATCH":
                continue
            out.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    out.sort()
    return out


def split_steps(dispatches):
    """The front-half dispatches of each step.  A step's matcher launches all start before its first weighting ends, so a
    match_kernel that starts behind every weighting seen so far, as many weightings as matcher launches, opens the next step."""
    steps, cur = [], []
    for d in dispatches:
        if d[2] not in FRONT:
            continue
        if d[2] == "match_kernel" and cur:
            n_match = sum(1 for x in cur if x[2] == "match_kernel")
            w_ends = [x[1] for x in cur if x[2] == "propose_weight_kernel"]
            if w_ends and len(w_ends) == n_match and d[0] >= max(w_ends):
                steps.append(cur)
                cur = []
        if cur or d[2] == "match_kernel":
            cur.append(d)
    if cur and any(x[2] == "propose_weight_kernel" for x in cur):
        steps.append(cur)
    return steps


def two_kernel_time(dispatches, t0, t1):
    """ns of [t0, t1] during which dispatches of at least two different kernels were in flight"""
    ev = []
    for s, e, k in dispatches:
        s, e = max(s, t0), min(e, t1)
        if s < e:
            ev.append((s, 1, k))
            ev.append((e, 0, k))            # at equal times an end sorts before a start
    ev.sort()
    live, total, prev = {}, 0, t0
    for t, kind, k in ev:
        if sum(1 for n in live.values() if n > 0) >= 2:
            total += t - prev
        prev = t
        live[k] = live.get(k, 0) + (1 if kind else -1)
    return total


def analyse(dispatches):
    rows = []
    for step in split_steps(dispatches):
        t0 = min(x[0] for x in step if x[2] == "match_kernel")
        t1 = max(x[1] for x in step if x[2] == "propose_weight_kernel")
        last_match_end = max(x[1] for x in step if x[2] == "match_kernel")
        ndt_early = any(x[2] == "ndt_kernel" and x[0] < last_match_end for x in step)
        inside = [d for d in dispatches if d[1] > t0 and d[0] < t1]
        rows.append({"span_us": (t1 - t0) / 1e3, "two_us": two_kernel_time(inside, t0, t1) / 1e3, "ndt_early": ndt_early,
                     "launches": len(step), "match_launches": sum(1 for x in step if x[2] == "match_kernel")})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    ap.add_argument("trace")
    ap.add_argument("--skip", type=int, default=0, help="steps left out of the medians (the warm-up)")
    ap.add_argument("--steps", action="store_true", help="print every step")
    a = ap.parse_args()
    rows = analyse(read_trace(a.trace))
    if not rows:
        raise SystemExit("no scan step (match_kernel ... propose_weight_kernel) in the trace")
    if a.steps:
        for i, r in enumerate(rows):
            print(f"step {i:4d}  span {r['span_us']:9.1f} us  two kernels in flight {r['two_us']:8.1f} us  "
                  f"ndt before last match end: {'yes' if r['ndt_early'] else 'no'}  front launches {r['launches']}")
    kept = rows[a.skip:] or rows
    med = statistics.median
    print(f"steps {len(rows)} (medians over the last {len(kept)})  matcher launches per step {med(r['match_launches'] for r in kept):g}")
    print(f"front-half span, median {med(r['span_us'] for r in kept):.1f} us  mean {statistics.fmean(r['span_us'] for r in kept):.1f} us")
    print(f"two different kernels in flight, median {med(r['two_us'] for r in kept):.1f} us  "
          f"({100.0 * sum(r['two_us'] for r in kept) / sum(r['span_us'] for r in kept):.1f} % of the span)")
    print(f"steps with an ndt_kernel started before the last match_kernel ended: {sum(r['ndt_early'] for r in kept)} of {len(kept)}")


if __name__ == "__main__":
    main()
