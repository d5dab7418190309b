"""tools/front_span.py on hand-made kernel traces: step boundaries, the span, the two-kernel overlap, the NDT-before-match flag."""
import csv
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
M, N, W = ("rbpf::match_kernel(rbpf::DevView, rbpf::MatchArgs)", "rbpf::ndt_kernel(rbpf::DevView, rbpf::MatchArgs)",
           "rbpf::propose_weight_kernel(rbpf::DevView, rbpf::ProposeArgs)")
MAP = "rbpf::map_update_ev_kernel(rbpf::DevView)"


def tool():
    spec = importlib.util.spec_from_file_location("front_span", os.path.join(HERE, "..", "tools", "front_span.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def write(path, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Kind", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        for name, s, e in rows:
            w.writerow(["KERNEL_DISPATCH", name, s, e])


def test_one_stream_and_two_streams(tmp_path):
    fs = tool()
    one, two = [], []
    for k in range(3):
        t = 2_000_000 * k
        one += [(M, t, t + 400_000), (N, t + 400_000, t + 600_000), (W, t + 600_000, t + 750_000), (MAP, t + 750_000, t + 1_600_000)]
        # second part's matcher runs on while the first part's NDT stage and weighting go by
        two += [(M, t, t + 200_000), (M, t + 1_000, t + 340_000), (N, t + 200_000, t + 300_000), (W, t + 300_000, t + 380_000),
                (N, t + 340_000, t + 450_000), (W, t + 450_000, t + 520_000), (MAP, t + 520_000, t + 1_400_000)]
    write(tmp_path / "one.csv", one)
    write(tmp_path / "two.csv", two)
    a = fs.analyse(fs.read_trace(str(tmp_path / "one.csv")))
    b = fs.analyse(fs.read_trace(str(tmp_path / "two.csv")))
    assert len(a) == len(b) == 3
    for r in a:
        assert r["span_us"] == 750.0 and r["two_us"] == 0.0 and not r["ndt_early"] and r["match_launches"] == 1
    for r in b:
        # NDT beside the matcher 100 us, weighting beside the matcher 40 us, beside the second NDT stage 40 us
        assert r["span_us"] == 520.0 and r["two_us"] == 180.0 and r["ndt_early"] and r["match_launches"] == 2 and r["launches"] == 6
