"""Diagnostic: per-phase cycles of a map-update kernel under the bench's step (needs a stamped build:
RBPF_STAMPS=mapev|mapray|mapupdate python -m thesis_amd.build --force; RBPF_MAP_KERNEL picks the kernel).
usage: probe_stamps.py [particles] [warm steps] [measured steps]

With a RBPF_STAMPS=mapev RBPF_STAMP_DEFS=-DEV_STAMP_TURNOVER build the event walk also leaves, per particle of its last launch, the
constant-rate clock and the cycle counter at the moment a workgroup takes the particle up and at the end of the last wave that
works on it.  From those this prints the in-kernel clock and the share of the CUs' time during which a particle is being worked
on (RBPF_EV_RESIDENT=0 / 1 picks the launch shape; PROBE_LIB=<path> loads another build of the library)."""
import os, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("PROBE_LIB"):
    import thesis_amd._lib as _lib
    _lib.LIB_PATH = os.path.abspath(os.environ["PROBE_LIB"])
turn_dir = tempfile.TemporaryDirectory(prefix="ev_turnover_")   # removed when the script ends
turn_path = os.path.join(turn_dir.name, "records.txt")
os.environ["RBPF_EV_TURNOVER_OUT"] = turn_path          # read by a turnover build's launcher only: other builds leave the directory empty
from bench import Runner, PERIOD_S
from thesis_amd.datasets import synthetic
P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
W = int(sys.argv[2]) if len(sys.argv) > 2 else 3
K = int(sys.argv[3]) if len(sys.argv) > 3 else 8
log = synthetic.make_log(W + K + 4, 1081, period=PERIOD_S)
r = Runner(P, 1081, 0.05, log)
for _ in range(W):
    r.step()
r.e.set_profiling(True)
for _ in range(K):
    r.step()
c = r.e.counters()
st = np.array(list(c["stamps"]), dtype=np.float64)
print("raycast ms mean", r.e.kernel_ms("raycast").mean(), "slow cells/pu", c["slow_cells"] / (K * P), "fallbacks", c["window_fallbacks"], "reasons %x" % c["fallback_reasons"])
print("kcycles per particle-update:", np.round(st / (K * P) / 1e3, 1).tolist(), "total", round(st.sum() / (K * P) / 1e3, 1))


def turnover(path):
    """The last launch's records: header `particles n workgroups g cus c wall_clock_khz k`, then per particle
    realtime in, realtime out, cycles in, cycles out, workgroup."""
    with open(path) as f:
        head = f.readline().split()
        rec = np.loadtxt(f, dtype=np.uint64, ndmin=2)
    h = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    rec = rec[rec[:, 1] > 0]                               # particles the launch worked on
    rt0, rt1, c0, c1, wg = (rec[:, i].astype(np.int64) for i in range(5))
    mhz = (h["wall_clock_khz"] or 100000) / 1e3            # the constant-rate clock (100 MHz where the device does not say)
    clock_mhz = np.median((c1 - c0) / np.maximum(rt1 - rt0, 1)) * mhz
    span_us = (rt1 - rt0) / mhz
    kernel_us = (rt1.max() - rt0.min()) / mhz
    share = span_us.sum() / (h["cus"] * kernel_us)
    print(f"turnover: {len(rec)} particles on {h['workgroups']} workgroups, {h['cus']} CUs; in-kernel clock {clock_mhz:.0f} MHz (median of "
          f"cycles / constant-rate ticks per particle, ticks at {mhz:.0f} MHz)")
    print(f"turnover: first particle taken up to last wave's end {kernel_us:.1f} us; per particle {span_us.mean():.2f} us mean, "
          f"{np.median(span_us):.2f} median, {(c1 - c0).mean() / 1e3:.1f} k cycles mean; a particle is being worked on during "
          f"{100 * share:.1f} % of the CUs' time")
    # the time between two particles on the same workgroup (resident launch) - the loop's own turnover
    order = np.lexsort((rt0, wg))
    same = wg[order][1:] == wg[order][:-1]
    if same.any():
        gap = (rt0[order][1:] - rt1[order][:-1])[same] / mhz
        print(f"turnover: between two particles of one workgroup {gap.mean():.2f} us mean, {np.median(gap):.2f} median, {gap.max():.2f} max")


if os.path.exists(turn_path):
    turnover(turn_path)
r.e.close()                                             # (no launch after this: the records' file may go)
turn_dir.cleanup()
