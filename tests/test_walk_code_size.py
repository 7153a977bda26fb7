"""The throughput kernel's decision walk is compiled without full RDO (enc_platform.h WaveGrpLean, enc_common.h rd_full): a tenth of the P-slice walk and a quarter of
the I-slice walk were RD_FULL code that a launch without an RD_FULL picture only walks past - and pays for: without it the kernel executes 3.5 % fewer instructions
(profiles/r07_history.md).  The cross-compile for gfx950 says how large each instantiation of the walk is; this test holds the difference (no GPU needed:
hipcc cross-compiles here, a few minutes).

The floors: with every test of rd_mode against RD_FULL folded to `false` by hand, this compiler's P-slice walk lost 22 764 bytes and its I-slice walk 48 688; the floors
leave room for the plumbing and still fail when the trait stops folding."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HIPCC, BUNDLER, READELF = "/opt/rocm/bin/hipcc", os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")


@pytest.fixture(scope="module")
def symbols(tmp_path_factory):
    """{demangled name: size in bytes} of the functions and kernels of k_encode.hip's gfx950 code object"""
    tmp = tmp_path_factory.mktemp("walk_code_size")
    obj, elf = tmp / "k_encode.o", tmp / "k_encode.elf"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(obj),
                        os.path.join(ROOT, "homerhevc_amd", "csrc", "k_encode.hip")], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    compile_log = r.stderr
    if obj.read_bytes()[:24] == b"__CLANG_OFFLOAD_BUNDLE__":
        r = subprocess.run([BUNDLER, "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950", f"--input={obj}", f"--output={elf}", "--unbundle"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    else:
        elf = obj
    r = subprocess.run([READELF, "-sW", "--demangle", str(elf)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {"resources": {}}
    for blk in compile_log.split("Function Name: ")[1:]:
        out["resources"][blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|VGPRs): (\d+)", blk)}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(.*)$", line)
        if m:
            out[m.group(2).strip()] = int(m.group(1))
    return out


def walk_size(symbols, walk, group):
    hits = [size for name, size in symbols.items() if name != "resources" and re.search(rf"\bhenc::{walk}<henc::{group}>\(", name)]
    assert len(hits) == 1, (walk, group, [n for n in symbols if walk in n])
    return hits[0]


@pytest.mark.skipif(not all(os.path.exists(p) for p in (HIPCC, BUNDLER, READELF)), reason="no hipcc / llvm tools")
def test_lean_walk_is_smaller_than_the_full_walk(symbols):
    sizes = {(walk, grp): walk_size(symbols, walk, grp) for walk in ("motion_inter_ctu", "motion_intra_ctu") for grp in ("WaveGrp", "WaveGrpLean")}
    print(sizes)
    assert sizes["motion_inter_ctu", "WaveGrp"] - sizes["motion_inter_ctu", "WaveGrpLean"] >= 15000, sizes
    assert sizes["motion_intra_ctu", "WaveGrp"] - sizes["motion_intra_ctu", "WaveGrpLean"] >= 35000, sizes


@pytest.mark.skipif(not all(os.path.exists(p) for p in (HIPCC, BUNDLER, READELF)), reason="no hipcc / llvm tools")
def test_three_pool_kernels(symbols):
    """the pool body's three instantiations; bench.py, tools/ and test_scratch_budget.py find the headline's kernel and the latency kernel by the substring k_encode_pool"""
    kernels = sorted(re.sub(r"\(.*", "", n) for n in symbols if re.match(r"k_encode_(pool|full)", n))
    assert kernels == ["k_encode_full", "k_encode_pool", "k_encode_pool_lat"], kernels
    assert len([k for k in kernels if "k_encode_pool" in k]) == 2


@pytest.mark.skipif(not all(os.path.exists(p) for p in (HIPCC, BUNDLER, READELF)), reason="no hipcc / llvm tools")
def test_generic_kernel_private_memory_budget(symbols):
    """test_scratch_budget.py holds the two kernels it finds by the substring k_encode_pool to the private-memory budget; the generic throughput kernel - what k_encode_pool
    was before the lean walk - is held to the same figures here"""
    full = [v for k, v in symbols["resources"].items() if "k_encode_full" in k]
    assert len(full) == 1, list(symbols["resources"])
    assert full[0]["ScratchSize [bytes/lane]"] <= 1024, full[0]
    assert full[0]["VGPRs Spill"] <= 8, full[0]
    assert full[0]["VGPRs"] <= 256, full[0]
