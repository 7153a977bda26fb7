"""What the picture bench tools (tools/*ingest_bench.py, *egress_bench.py, ssim_bench.py) share.  A tool is a workload description over this module: its kernel child, its
byte formula and the keys of its result file.

The first part is pure - it imports neither torch nor the library, so tests/test_picture_support_cpu.py runs it: the reduction of a kernel trace to launch times, the rate
record, spread(), bench.py's lines from a file, the result file.  The second part starts the profiler's child runs and builds encoders and descriptors over
tests/picture_gpu.py's binding; a traced child always runs BEFORE the tool's own process opens the GPU, and the counter pass is a run of its own with no tracing beside it."""
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_PEAK_TBS = 6.29          # float4 copy, measured (the microarchitecture notes' HBM figure; 8.0 TB/s is the specification)
BENCH_KEYS = ("value", "unit", "ms_per_step", "steps", "warmup", "build")


# ---- pure ----
def is_kernel(kernel_name, kernel):
    """whether a trace row's Kernel_Name is `kernel`: the whole identifier in front of the parameter list (whatever namespace or return type the profiler prints before
    it, whatever suffix after it), so k_egress is not k_egress_rgb and k_ingest is neither k_ingest_rgb nor k_ingest_yuv"""
    return re.search(r"(?<![A-Za-z0-9_])" + re.escape(kernel) + r"(?![A-Za-z0-9_])", kernel_name.split("(anonymous namespace)::")[-1].split("(")[0]) is not None


def kernel_rows(rows, kernel):
    """the rows of one kernel, in launch order"""
    return sorted((r for r in rows if is_kernel(r["Kernel_Name"], kernel)), key=lambda r: int(r["Start_Timestamp"]))


def launch_groups(rows, kernel, groups, launches):
    """The kernel's launch times in us as `groups` lists of `launches - 1`: the trace holds groups x launches launches of it, and the first of every group is the warm-up.
    Any other count is the error dict a tool returns as its kernel_rate, and so is traced_child's error dict in place of the rows."""
    if isinstance(rows, dict):
        return rows
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in kernel_rows(rows, kernel)]
    if len(us) != groups * launches:
        return {"error": f"{len(us)} launches of {kernel} in the trace, {groups * launches} expected", "us": us}
    return [us[g * launches + 1:(g + 1) * launches] for g in range(groups)]


def tb_per_s(part, nbytes):
    return nbytes / (statistics.median(part) * 1e-6) / 1e12


def rate(part, nbytes, **first):
    """the record of one group of timed launches that move nbytes each; `first` are the keys a tool puts in front"""
    tbs = tb_per_s(part, nbytes)
    return dict(first, launch_us=[round(x, 1) for x in part], median_us=round(statistics.median(part), 1), tb_per_s=round(tbs, 3),
                **{"share_of_float4_copy_6.29": round(tbs / COPY_PEAK_TBS, 3)})


def spread(xs):
    return {"runs": [round(x, 3) for x in xs], "median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "spread": round(max(xs) - min(xs), 3)}


def bench_lines(path):
    """bench.py's result lines in a file of its output (log lines and JSON lines without a value are passed over), each cut down to BENCH_KEYS; [] without the file"""
    if not path or not os.path.exists(path):
        return []
    lines = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
    return [{k: b.get(k) for k in BENCH_KEYS} for b in lines if b.get("value") is not None and "metric" in b]


def last_bench_lines(paths):
    """the last result line of each file that has one"""
    return [runs[-1] for runs in map(bench_lines, paths) if runs]


def write_result(result, out):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


# ---- the profiler's child runs ----
def _profiled_child(flags, name, dir_name, written, script, args, timeout, show_progress):
    """`rocprofv3 FLAGS --output-format csv -d DIR -o NAME -- python SCRIPT --kernel-child ARGS` as a child with a timeout: (the rows of the csv file it wrote, or an
    error dict; the command as a result file records it)"""
    head = ["rocprofv3"] + flags + ["--output-format", "csv", "-d"]
    recorded = " ".join(head + [dir_name, "-o", name, "--", "python", "tools/" + os.path.basename(script), "--kernel-child"] + args)
    with tempfile.TemporaryDirectory(prefix=f"{name}_prof_") as out:
        cmd = head + [out, "-o", name, "--", sys.executable, os.path.abspath(script), "--kernel-child"] + args
        if show_progress:      # (the child's progress lines go to this program's output as they come)
            with open(os.path.join(out, "stderr.txt"), "w") as err:
                r = subprocess.run(cmd, stderr=err, timeout=timeout)
            stderr = open(os.path.join(out, "stderr.txt")).read()
        else:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
            stderr = r.stderr
        if r.returncode != 0:
            return {"error": f"rocprofv3 run failed ({r.returncode})", "stderr_tail": stderr[-1500:]}, recorded
        files = glob.glob(os.path.join(out, "**", written[0]), recursive=True)
        if not files:
            return {"error": written[1], "files": sorted(os.listdir(out))}, recorded
        return list(csv.DictReader(open(files[0]))), recorded


def traced_child(script, args, out_prefix, timeout=900, show_progress=False):
    """the tool's kernel child under `rocprofv3 --kernel-trace --stats`, no counters: (the kernel trace's rows or an error dict, the command with TRACE_DIR for the directory)"""
    return _profiled_child(["--kernel-trace", "--stats"], out_prefix, "TRACE_DIR", ("*kernel_trace.csv", "no kernel trace written"), script, args, timeout, show_progress)


def counted_child(script, args, counters, timeout=900):
    """ONE `rocprofv3 --pmc` pass of its own over the tool's kernel child, no tracing beside it: (the counter file's rows or an error dict, the command)"""
    return _profiled_child(["--pmc"] + counters, "pmc", "DIR", ("*counter_collection.csv", "no counter file written"), script, args, timeout, False)


def resources(kernel):
    """the compiler's resource report for one kernel of csrc/picture_io.hip"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return {"skipped": "no hipcc"}
    with tempfile.TemporaryDirectory(prefix=f"{kernel}_isa_") as out:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                            "-o", os.path.join(out, "picture_io.s"), os.path.join(ROOT, "homerhevc_amd", "csrc", "picture_io.hip")], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"error": r.stderr[-800:]}
    for blk in r.stderr.split("Function Name: ")[1:]:
        if f"{len(kernel)}{kernel}" in blk.split()[0] or is_kernel(blk.split()[0], kernel):      # (the report names functions mangled: the length, then the name)
            return {k: int(v) for k, v in re.findall(r"(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]): (\d+)", blk)}
    return {"error": f"{kernel} is not in the report"}


# ---- the GPU: tests/picture_gpu.py's binding, encoders, descriptors ----
def _pg():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
    import picture_gpu as pg
    return pg


def library():
    """the library through tests/picture_gpu.py's one binding"""
    return _pg().load()


def encoders(lib, n, w, h, **keys):
    """n encoders of w x h as (context, encoder) pairs, a context - a stream - each"""
    return [_pg().new_encoder(lib, w, h, **keys) for _ in range(n)]


def close(lib, made):
    pg = _pg()
    for ctx, enc in made:
        pg.drop(lib, ctx, enc)


def stream_of():
    return _pg().current_stream()


def i420_picture(t, w, h):
    """the descriptor of a tightly packed I420 picture in the uint8 CUDA tensor t"""
    p = _pg().Picture(format=0, reserved=0)
    p.plane[0], p.plane[1], p.plane[2] = t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4
    p.pitch[0], p.pitch[1], p.pitch[2] = w, w // 2, w // 2
    return p


def nv12_picture(t, w, h):
    p = _pg().Picture(format=1, reserved=0)
    p.plane[0], p.plane[1] = t.data_ptr(), t.data_ptr() + w * h
    p.pitch[0], p.pitch[1] = w, w
    return p
