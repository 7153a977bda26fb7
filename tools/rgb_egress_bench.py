#!/usr/bin/env python3
"""GPU box tool: what the RGB egress (include/homer_gpu.h section 12i, k_egress_rgb in csrc/picture_io.hip) costs, on bench.py's flagship workload (256 sequences of
1920x1080, bench.py's configuration and clips).  Writes profiles/rgb_egress_bench.json.

    python tools/rgb_egress_bench.py [--sequences 256] [--notes FILE]

  kernel_rate   k_egress_rgb's time for one launch over all sequences' final pictures, per output form without sums and for some variants with sums, from
                `rocprofv3 --kernel-trace --stats` in a run of its own (this program starts it as a child, the traced program behind `--`, no counters): a warm-up
                launch and five timed ones per variant, medians; bytes from egress_rgb_bytes() below.
  yardstick     k_egress writing the same encoders' final pictures as I420, in the same traced run: code from before this kernel.
  gate          the outputs `rgba`, planar uint8, planar float16 and planar float32 without sums reach at least 0.8 of the yardstick's bytes per second (the allowance is
                the distance this access class already shows from a plain copy, and covers the chroma neighbour re-reads); 3-byte packed output and the variants with sums
                are recorded without a gate.
  resources     the compiler's resource report for the kernel (hipcc -Rpass-analysis=kernel-resource-usage), when hipcc is there."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import egress_bench as eb  # noqa: E402  (the kernel child's first step and the yardstick's launches)
import ingest_bench as ib  # noqa: E402  (the workload and the encoders' set-up)
import picture_bench  # noqa: E402

W, H = ib.W, ib.H

PACKED8, PLANAR8, PLANAR_F16, PLANAR_F32 = 0, 1, 2, 3
# form -> (format, pixel bytes, byte of R, G, B)
FORMS = {"rgb": (PACKED8, 3, (0, 1, 2)), "rgba": (PACKED8, 4, (0, 1, 2)), "planar8": (PLANAR8, 0, (0, 0, 0)), "f16": (PLANAR_F16, 0, (0, 0, 0)), "f32": (PLANAR_F32, 0, (0, 0, 0))}
# (name, output form or None, reference form or None)
VARIANTS = [("rgb", "rgb", None), ("rgba", "rgba", None), ("planar8", "planar8", None), ("f16", "f16", None), ("f32", "f32", None),
            ("rgba_with_sums_against_rgba", "rgba", "rgba"), ("planar8_with_sums_against_f32", "planar8", "f32"), ("f16_with_sums_against_f16", "f16", "f16"),
            ("sums_only_against_planar8", None, "planar8"), ("sums_only_against_f32", None, "f32")]
GATED = ["rgba", "planar8", "f16", "f32"]
GATE = 0.8
LAUNCHES = 6          # a warm-up launch and five timed ones


def pixel_bytes(form):
    fmt, pb, _ = FORMS[form]
    return pb if fmt == PACKED8 else {PLANAR8: 3, PLANAR_F16: 6, PLANAR_F32: 12}[fmt]


def egress_rgb_bytes(width, height, out_form, ref_form):
    """algorithmic bytes of one picture through k_egress_rgb (the comment at k_egress_rgb in csrc/picture_io.hip): the int16 planes are read (3 W H), the reference picture is read
    when sums are asked for, the RGB picture is written when one is asked for (3, 4, 3, 6 or 12 W H by form)"""
    return (3.0 + (pixel_bytes(out_form) if out_form else 0) + (pixel_bytes(ref_form) if ref_form else 0)) * width * height


def pictures(torch, RgbPicture, S, form, random):
    """a picture of its own per sequence in the form: (the tensor that holds them all, their descriptors)"""
    fmt, pb, offs = FORMS[form]
    if fmt == PACKED8:
        t = torch.randint(0, 256, (S, H, W, pb), dtype=torch.uint8, device="cuda") if random else torch.empty((S, H, W, pb), dtype=torch.uint8, device="cuda")
    else:
        dtype = {PLANAR8: torch.uint8, PLANAR_F16: torch.float16, PLANAR_F32: torch.float32}[fmt]
        if not random:
            t = torch.empty((S, 3, H, W), dtype=dtype, device="cuda")
        elif fmt == PLANAR8:
            t = torch.randint(0, 256, (S, 3, H, W), dtype=dtype, device="cuda")
        else:
            t = torch.rand((S, 3, H, W), dtype=dtype, device="cuda")
    pics = []
    for i in range(S):
        p = RgbPicture(format=fmt, matrix=1, full_range=0, reserved=0, pixel_bytes=pb)
        for c in range(3):
            p.offset[c] = offs[c]
        if fmt == PACKED8:
            p.plane[0], p.pitch[0] = t[i].data_ptr(), W * pb
        else:
            for c in range(3):
                p.plane[c], p.pitch[c] = t[i, c].data_ptr(), W * t.element_size()
        pics.append(p)
    return t, pics


def kernel_child(S):
    """the traced program: every sequence encodes one picture, then LAUNCHES launches of k_egress (I420 pictures) and LAUNCHES of k_egress_rgb per variant over the S final
    pictures"""
    from rgb_cases import RgbPicture
    torch, lib, made, encs = eb.encoded_once(S)
    outs, as_i420, as_nv12 = eb.outputs(torch, S)
    sums = torch.zeros((S, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    print("encoded one picture per sequence; k_egress", flush=True)
    for _ in range(LAUNCHES):
        eb.export_device(lib, encs, as_i420, 0, None)
        torch.cuda.synchronize()
    del outs
    e_arr, which = (C.c_void_p * S)(*encs), (C.c_int * S)(*([-1] * S))
    for name, out_form, ref_form in VARIANTS:
        out_t, out_pics = pictures(torch, RgbPicture, S, out_form, False) if out_form else (None, None)
        ref_t, ref_pics = pictures(torch, RgbPicture, S, ref_form, True) if ref_form else (None, None)
        torch.cuda.synchronize()
        print("k_egress_rgb:", name, flush=True)
        for _ in range(LAUNCHES):
            assert lib.hmr_gpu_enc_export_pictures_rgb_device(e_arr, S, which, (RgbPicture * S)(*out_pics) if out_pics else None, (RgbPicture * S)(*ref_pics) if ref_pics else None,
                                                              C.c_void_p(sums.data_ptr()) if ref_pics else None, picture_bench.stream_of()) == 0, lib.hmr_gpu_last_error()
            torch.cuda.synchronize()
        del out_t, ref_t
    picture_bench.close(lib, made)


def kernel_rate(S):
    rows, command = picture_bench.traced_child(__file__, ["--sequences", str(S)], "rgb_egress", timeout=1100, show_progress=True)
    plain = picture_bench.launch_groups(rows, "k_egress", 1, LAUNCHES)
    rgb = picture_bench.launch_groups(rows, "k_egress_rgb", len(VARIANTS), LAUNCHES)
    for groups in (plain, rgb):
        if isinstance(groups, dict):
            return groups
    res = {"command": command, "pictures_per_launch": S, "source": "the encoders' final pictures (which = -1)", "output_pictures": "one picture per sequence, BT.709 limited range",
           "bytes_formula": "3 W H read + the reference form's bytes read (sums) + the output form's bytes written: 3 / 4 / 3 / 6 / 12 W H for rgb / rgba / planar8 / f16 / f32"}
    yard = picture_bench.rate(plain[0], (3.0 + 1.5) * W * H * S, bytes_per_launch=(3.0 + 1.5) * W * H * S)
    res["yardstick_k_egress_i420_picture_same_visit"] = dict(yard, profiles_egress_bench_json_tb_per_s=5.08)
    for (name, out_form, ref_form), part in zip(VARIANTS, rgb):
        nbytes = egress_rgb_bytes(W, H, out_form, ref_form) * S
        res[name] = picture_bench.rate(part, nbytes, bytes_per_launch=nbytes)
        res[name]["ratio_to_yardstick"] = round(res[name]["tb_per_s"] / yard["tb_per_s"], 3)
    res["gate"] = {"condition": f"bytes per second of {', '.join(GATED)} (no sums) >= {GATE} x the yardstick's", "ratios": {n: res[n]["ratio_to_yardstick"] for n in GATED},
                   "holds": all(res[n]["tb_per_s"] >= GATE * yard["tb_per_s"] for n in GATED)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--notes", help="a text file whose lines become the result's notes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_egress_bench.json"))
    a = ap.parse_args()
    if a.kernel_child:
        kernel_child(a.sequences)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/rgb_egress_bench.py", "source_digest": source_digest(), "sequences": a.sequences, "width": W, "height": H,
              "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": {name: egress_rgb_bytes(W, H, o, r) for name, o, r in VARIANTS}}
    result["kernel_rate"] = kernel_rate(a.sequences)
    res = picture_bench.resources("k_egress_rgb")
    result["notes"] = [f"compiler's resource report for k_egress_rgb (hipcc -O3, gfx950): {json.dumps(res)}"]
    if a.notes and os.path.exists(a.notes):
        result["notes"] += [ln.strip() for ln in open(a.notes) if ln.strip()]
    picture_bench.write_result(result, a.out)


if __name__ == "__main__":
    main()
