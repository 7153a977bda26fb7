"""No GPU: the support modules of the picture tests and tools.  tests/picture_gpu.py's binding table against include/homer_gpu.h and the built library, and the pure part
of tools/picture_bench.py - the reduction of a kernel trace, spread(), bench.py's lines from a file, the rate record - on inputs written here."""
import csv
import ctypes
import os
import re
import sys

import libs
import picture_gpu
from test_abi_exports import declared_symbols

sys.path.insert(0, os.path.join(libs.ROOT, "tools"))
import picture_bench as pb  # noqa: E402


def prototypes():
    """{name: parameter count} of every hmr_gpu_* function the header declares (comments stripped as in test_abi_exports.py)"""
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for name, params in re.findall(r"\b(hmr_gpu_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        found[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return found


def test_the_binding_is_the_headers():
    from homerhevc_amd.build import build_native
    build_native()
    declared, table = prototypes(), picture_gpu.SIGNATURES
    assert set(declared) == set(declared_symbols())      # (this module's parser sees the functions test_abi_exports.py's sees)
    device = {n for n in declared if re.fullmatch(r"hmr_gpu_enc_[a-z0-9_]*_device", n)}
    assert len(device) >= 18 and device == {n for n in table if n.endswith("_device")}
    for name, (argtypes, restype) in table.items():
        assert name in declared, name
        assert argtypes is None or len(argtypes) == declared[name], (name, len(argtypes), declared[name])
    lib = ctypes.CDLL(libs.GPU_SO)      # (loads without a GPU)
    missing = [n for n in table if not hasattr(lib, n)]
    assert not missing, missing
    # declare() leaves no entry out, on any handle
    picture_gpu.declare(lib)
    for name, (argtypes, restype) in table.items():
        fn = getattr(lib, name)
        assert (argtypes is None or list(fn.argtypes) == list(argtypes)) and (restype is None or fn.restype is restype), name


# the profiler prints a kernel's name with its namespace and parameter list; k_egress is a prefix of k_egress_rgb
K_EGRESS, K_EGRESS_RGB = "(anonymous namespace)::k_egress(EgressJob const*)", "(anonymous namespace)::k_egress_rgb(RgbEgressJob const*)"


def write_trace(path, launches):
    """a kernel-trace csv of (kernel name, start ns, duration ns) launches, in the order given"""
    with open(path, "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["Kind", "Agent_Id", "Kernel_Id", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        for k, (name, start, ns) in enumerate(launches):
            out.writerow(["KERNEL_DISPATCH", 1, k, name, start, start + ns])


def test_trace_reduction(tmp_path):
    # 2 groups x 3 launches of k_egress at 1000, 2000, ... ns: warm-ups of 9 and 8 us, then 1, 3 us and 5, 2 us; k_egress_rgb's launches of 7 us in between; rows shuffled
    mine = [(K_EGRESS, 1000 * (k + 1), ns) for k, ns in enumerate((9000, 1000, 3000, 8000, 5000, 2000))]
    other = [(K_EGRESS_RGB, 1000 * (k + 1) + 500, 7000) for k in range(4)]
    rows = mine + other
    rows = [rows[k] for k in (7, 2, 9, 0, 5, 3, 8, 1, 6, 4)]
    write_trace(tmp_path / "x_kernel_trace.csv", rows)
    read = list(csv.DictReader(open(tmp_path / "x_kernel_trace.csv")))
    groups = pb.launch_groups(read, "k_egress", 2, 3)
    assert groups == [[1.0, 3.0], [5.0, 2.0]]
    assert [pb.rate(g, 1e6)["median_us"] for g in groups] == [2.0, 3.5]
    assert pb.launch_groups(read, "k_egress_rgb", 2, 2) == [[7.0], [7.0]]
    assert not pb.is_kernel(K_EGRESS_RGB, "k_egress") and pb.is_kernel(K_EGRESS, "k_egress") and pb.is_kernel("k_egress.kd", "k_egress")
    assert not pb.is_kernel("k_ingest_yuv(YuvIngestJob const*)", "k_ingest") and not pb.is_kernel("void k_ingest_rgb(RgbIngestJob const*)", "k_ingest")
    assert not pb.is_kernel("k_other(k_egress const*)", "k_egress")      # (a parameter's type is not the kernel's name)
    # one launch too few
    short = [r for r in read if not (r["Kernel_Name"] == K_EGRESS and r["Start_Timestamp"] == "6000")]
    error = pb.launch_groups(short, "k_egress", 2, 3)
    assert error == {"error": "5 launches of k_egress in the trace, 6 expected", "us": [9.0, 1.0, 3.0, 8.0, 5.0]}
    # the profiler's own failure comes through as it is
    assert pb.launch_groups({"error": "no kernel trace written", "files": []}, "k_egress", 2, 3) == {"error": "no kernel trace written", "files": []}


def test_spread():
    assert pb.spread([3.0, 1.0004, 2.0]) == {"runs": [3.0, 1.0, 2.0], "median": 2.0, "min": 1.0, "max": 3.0, "spread": 2.0}
    assert pb.spread([5.0]) == {"runs": [5.0], "median": 5.0, "min": 5.0, "max": 5.0, "spread": 0.0}


def test_bench_lines(tmp_path):
    path = tmp_path / "bench.txt"
    path.write_text("building ...\n"
                    '{"metric": "frames_per_s", "value": 100.5, "unit": "fps", "ms_per_step": 2.5, "steps": 20, "warmup": 5, "build": "abc", "n_gpus": 1}\n'
                    '{"metric": "frames_per_s", "unit": "fps"}\n'
                    '{"metric": "frames_per_s", "value": 101.5, "unit": "fps", "ms_per_step": 2.4, "steps": 20, "warmup": 5}\n')
    runs = pb.bench_lines(str(path))
    assert runs == [{"value": 100.5, "unit": "fps", "ms_per_step": 2.5, "steps": 20, "warmup": 5, "build": "abc"},
                    {"value": 101.5, "unit": "fps", "ms_per_step": 2.4, "steps": 20, "warmup": 5, "build": None}]
    assert pb.last_bench_lines([str(path), str(tmp_path / "absent.txt")]) == [runs[1]]
    assert pb.bench_lines(None) == [] and pb.bench_lines(str(tmp_path / "absent.txt")) == []


def test_rate_record():
    assert pb.COPY_PEAK_TBS == 6.29
    assert pb.rate([1.0], 1e6) == {"launch_us": [1.0], "median_us": 1.0, "tb_per_s": 1.0, "share_of_float4_copy_6.29": round(1.0 / 6.29, 3)}
    record = pb.rate([4.0, 1.0, 2.0], 6.29e6, kernel="k", bytes_per_launch=6.29e6)      # median 2 us: 3.145 TB/s, half the copy's rate
    assert list(record) == ["kernel", "bytes_per_launch", "launch_us", "median_us", "tb_per_s", "share_of_float4_copy_6.29"]
    assert record["tb_per_s"] == 3.145 and record["share_of_float4_copy_6.29"] == 0.5
