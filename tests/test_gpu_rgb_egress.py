"""-m gpu: reconstructed pictures and picture slots as RGB in device memory, and their distance to the caller's RGB pictures (include/homer_gpu.h section 12i, k_egress_rgb
in csrc/picture_io.hip, homerhevc_amd/encoder.py).  The comparator of every picture is the numpy restatement of the section's arithmetic (tests/rgb_egress_cases.py),
applied to the 4:2:0 picture that went in (a slot) or that hmr_gpu_enc_export_picture_device hands out (a final picture) - never the kernel; the final pictures of the
fixtures are also pinned by tests/golden/rgb_egress.json, minted from the compiled reference's own reconstruction.  Every output lies in a larger buffer of random bytes at
an odd address and a padded pitch (or tight), and every byte outside the rows has to stay what it was."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import encoder_cases as ec
import rgb_cases as rc
import rgb_egress_cases as re_
from homerhevc_amd.encoder import BatchEncoder, Encoder, Picture, RGBFrame, psnr_rgb
from picture_gpu import (BATCH_CASES, GOLD, LAYOUTS, Output, as_tensors, config_of, current_stream, drop, export_one, gpu, make_encoder, new_encoder, new_sums,  # noqa: F401
                         rgb_frame, upload)
from picture_gpu import RgbSource as Source      # the references: rc.lay_out's buffers uploaded, rc.descriptor over them
from rgb_scale_cases import chans_of

pytestmark = pytest.mark.gpu
ERR_ARG = -3
FORMS = sorted(rc.FORMS)
RGB_GOLD = json.load(open(os.path.join(ec.GOLDEN, "rgb_egress.json")))


class Target:
    """an output picture of one form in device memory: re_.Canvas's buffers uploaded; check() downloads them"""

    def __init__(self, form, w, h, matrix, full, rng, padded=True):
        import torch
        self.canvas, self.matrix, self.full = re_.Canvas(form, w, h, rng, padded), matrix, full
        self.tensors = [torch.from_numpy(b).cuda() for b in self.canvas.buffers]
        self.pic = self.canvas.descriptor([t.data_ptr() for t in self.tensors], matrix, full)

    def check(self, rgb):
        self.canvas.check([t.cpu().numpy() for t in self.tensors], rgb)

    def untouched(self):
        return all(np.array_equal(t.cpu().numpy(), b) for t, b in zip(self.tensors, self.canvas.before))


def export_rgb(lib, encs, which, targets, refs, sums, stream=None):
    k = len(encs)
    rc_ = lib.hmr_gpu_enc_export_pictures_rgb_device((C.c_void_p * k)(*encs), k, (C.c_int * k)(*which), (rc.RgbPicture * k)(*[t.pic for t in targets]) if targets is not None else None,
                                                     (rc.RgbPicture * k)(*[r.pic for r in refs]) if refs is not None else None, C.c_void_p(sums.data_ptr()) if sums is not None else None,
                                                     stream or current_stream())
    assert rc_ == 0, lib.hmr_gpu_last_error()


def load_yuv(lib, enc, slot, yuv, w, h, layout="tight_i420", seed=0):
    pic, keep = upload(tuple(np.ascontiguousarray(p).tobytes() for p in yuv), w, h, layout, seed)
    assert lib.hmr_gpu_enc_load_source_device(enc, slot, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()


def final_yuv(lib, enc, w, h):
    """the encoder's final picture through the 4:2:0 export of section 12e, as I420 bytes"""
    out = Output(w, h, "tight_i420")
    export_one(lib, enc, out, -1, None)
    return out.picture()


# ---- slot pictures, no encode ----
@pytest.mark.parametrize("size", [(72, 8), (128, 64), (136, 40), (200, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_slot_pictures_in_every_form_and_table(gpu, size):
    """noise in slot 0, the values at which the ranges begin and end in slot 1; per layout ONE call with all 36 combinations of form and table, the slots in turn"""
    lib, (w, h) = gpu, size
    ctx, enc = new_encoder(lib, w, h)
    rng = np.random.default_rng(w + h)
    slots = [re_.noise_yuv(rng, w, h), re_.extremes_yuv(rng, w, h)]
    for s, yuv in enumerate(slots):
        load_yuv(lib, enc, s, yuv, w, h, LAYOUTS[s], seed=s)
    for padded in (True, False):
        combos = [(form, matrix, full) for form in FORMS for matrix, full in rc.MATRIX_RANGES]
        targets = [Target(form, w, h, matrix, full, rng, padded) for form, matrix, full in combos]
        which = [k & 1 for k in range(len(combos))]
        export_rgb(lib, [enc] * len(combos), which, targets, None, None)
        for t, s in zip(targets, which):
            t.check(re_.restate(*slots[s], t.matrix, t.full))
    drop(lib, ctx, enc)


def test_slot_picture_1080p(gpu):
    lib, (w, h) = gpu, (1920, 1080)
    ctx, enc = new_encoder(lib, w, h, wpp=17)
    rng = np.random.default_rng(5)
    yuv = re_.noise_yuv(rng, w, h)
    load_yuv(lib, enc, 0, yuv, w, h)
    targets = [Target("f16", w, h, "bt709", 0, rng, True), Target("bgra", w, h, "bt601", 1, rng, False)]
    export_rgb(lib, [enc, enc], [0, 0], targets, None, None)
    for t in targets:
        t.check(re_.restate(*yuv, t.matrix, t.full))
    drop(lib, ctx, enc)


@pytest.mark.parametrize("form", ["f16", "f32"])
def test_all_256_float_values_on_the_device(gpu, form):
    """full range and chroma 128 give R = G = B = Y: a luma ramp puts every 8-bit value through the device's division (and its rounding to binary16)"""
    lib, (w, h) = gpu, (256, 8)
    ctx, enc = new_encoder(lib, w, h)
    rng = np.random.default_rng(1)
    ramp = np.tile(np.arange(256, dtype=np.uint8), (h, 1))
    load_yuv(lib, enc, 0, [ramp, np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)], w, h)
    t = Target(form, w, h, "bt601", 1, rng, False)
    export_rgb(lib, [enc], [0], [t], None, None)
    chans, _ = t.canvas.channels([x.cpu().numpy() for x in t.tensors])
    want = np.arange(256).astype(np.float32) / np.float32(255)
    want = want.astype(np.float16) if form == "f16" else want
    bits = np.uint16 if form == "f16" else np.uint32
    for got in chans:
        for row in got:
            assert np.array_equal(row.view(bits), want.view(bits)), np.flatnonzero(row.view(bits) != want.view(bits))[:8].tolist()
        assert np.array_equal(rc.quantize(got[0]), np.arange(256))
    drop(lib, ctx, enc)


# ---- final pictures ----
def md5s(rgb):
    return [hashlib.md5(np.ascontiguousarray(p).tobytes()).hexdigest() for p in rgb]


@pytest.mark.parametrize("case", ["200x136", "416x240_wpp_rows"])
def test_final_pictures_and_sums_of_the_fixtures(gpu, case):
    """which = -1 after every frame: the BT.709 limited-range picture has the md5s of the restatement applied to the REFERENCE's reconstruction, every form equals the
    restatement applied to what the 4:2:0 export hands out, the sums against rgb_cases.yuv_to_rgb(the clip's frame) are the fixture's, and the stream is what it was"""
    lib, g, q = gpu, GOLD[case], RGB_GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    rng = np.random.default_rng(3)
    buf, n, stream = C.create_string_buffer(1 << 20), C.c_long(), b""
    for f, planes in enumerate(clip):
        pic, keep = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        rec = final_yuv(lib, enc, w, h)
        original = rc.yuv_to_rgb(planes, w, h)
        form, (matrix, full) = FORMS[f % len(FORMS)], rc.MATRIX_RANGES[(f + 1) % 4]
        targets = [Target("planar8", w, h, "bt709", 0, rng, bool(f & 1)), Target(form, w, h, matrix, full, rng, not f & 1)]
        refs = [Source("planar8", original, "bt601", 1, rng), Source(FORMS[(f + 4) % len(FORMS)], chans_of(FORMS[(f + 4) % len(FORMS)], rng, *original), "bt601", 0, rng)]
        sums = new_sums(2)
        export_rgb(lib, [enc, enc], [-1, -1], targets, refs, sums)
        want = re_.restate_bytes(rec, w, h, "bt709", 0)
        targets[0].check(want)
        assert md5s(want) == q["rgb_md5"][f], (case, f)
        assert sums[0].tolist() == q["ssd"][f] == re_.numpy_ssd(original, want), (case, f)
        other = re_.restate_bytes(rec, w, h, matrix, full)
        targets[1].check(other)
        assert sums[1].tolist() == re_.numpy_ssd(original, other), (case, f, form)
        assert all(r.untouched() for r in refs)
    drop(lib, ctx, enc)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


# ---- sums ----
def test_sums_against_references_in_every_form(gpu):
    """a slot picture with a row tail (136 x 40) and a final picture (200 x 136); the reference in every form, the float forms also with whatever a float can hold; the
    sums alone (the table comes from the reference's fields) and with the picture (the table comes from the output's: the reference's fields are not used)"""
    lib = gpu
    rng = np.random.default_rng(12)
    ctx, enc, w, h, image_type, clip = make_encoder(lib, "200x136")
    buf, n = C.create_string_buffer(1 << 20), C.c_long()
    pic, keep = upload(clip[0], w, h, "tight_i420")
    assert lib.hmr_gpu_enc_load_source_device(enc, 0, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_encode_source(enc, 0, image_type, buf, len(buf), C.byref(n), None) == 2, lib.hmr_gpu_last_error()
    rec = final_yuv(lib, enc, w, h)
    ctx2, enc2 = new_encoder(lib, 136, 40)
    slot = re_.noise_yuv(rng, 136, 40)
    load_yuv(lib, enc2, 0, slot, 136, 40)
    kinds = [(form, False) for form in FORMS] + [("f16", True), ("f32", True)]
    for e, which, ew, eh, rgb_of in ((enc, -1, w, h, lambda m, fr: re_.restate_bytes(rec, w, h, m, fr)), (enc2, 0, 136, 40, lambda m, fr: re_.restate(*slot, m, fr))):
        refs, eight, tables = [], [], []
        for k, (form, special) in enumerate(kinds):
            chans = rc.special_floats(rc.FLOAT_TYPES[form], rng, ew, eh) if special else chans_of(form, rng, *rc.noise(rng, ew, eh))
            tables.append(rc.MATRIX_RANGES[k % 4])
            refs.append(Source(form, chans, *tables[-1], rng, padded=bool(k % 3)))
            eight.append(rc.eight_bit(form, chans))
        k = len(kinds)
        only = new_sums(k)
        export_rgb(lib, [e] * k, [which] * k, None, refs, only)
        for i in range(k):
            assert only[i].tolist() == re_.numpy_ssd(eight[i], rgb_of(*tables[i])), (which, kinds[i], tables[i])
        targets = [Target(FORMS[(i + 2) % len(FORMS)], ew, eh, *rc.MATRIX_RANGES[(i + 1) % 4], rng, bool(i & 1)) for i in range(k)]
        both = new_sums(k)
        export_rgb(lib, [e] * k, [which] * k, targets, refs, both)
        for i, t in enumerate(targets):
            want = rgb_of(t.matrix, t.full)
            t.check(want)
            assert both[i].tolist() == re_.numpy_ssd(eight[i], want), (which, kinds[i], t.canvas.form)
        assert all(r.untouched() for r in refs)
    drop(lib, ctx, enc)
    drop(lib, ctx2, enc2)


# ---- batch ----
@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_of_different_sizes(gpu, pipelined):
    """sequences of different sizes: one load, one batch launch and ONE RGB export per step for those that still have frames - forms and tables mixed, some entries the final
    picture and some the slot, references in mixed forms.  Pipelined: the export follows its step directly, while that step's access units are still outstanding."""
    lib = gpu
    made = [make_encoder(lib, case) for case in BATCH_CASES]
    bufs = [C.create_string_buffer(1 << 20) for _ in made]
    streams = [b"" for _ in made]
    rng = np.random.default_rng(21)

    def call(live, slot):
        k = len(live)
        got = (C.c_long * k)()
        fn = lib.hmr_gpu_enc_encode_batch_pipelined if pipelined else lib.hmr_gpu_enc_encode_batch
        assert fn((C.c_void_p * k)(*[made[i][1] for i in live]), k, (C.c_int * k)(*([slot] * k)) if slot is not None else None,
                  (C.c_int * k)(*[made[i][4] for i in live]), (C.c_char_p * k)(*[C.cast(bufs[i], C.c_char_p) for i in live]), (C.c_long * k)(*[len(bufs[i]) for i in live]),
                  got) == 0, lib.hmr_gpu_last_error()
        for j, i in enumerate(live):
            streams[i] += C.string_at(bufs[i], got[j])

    prev = None
    for f in range(max(len(m[5]) for m in made)):
        live = [i for i, m in enumerate(made) if f < len(m[5])]
        k, slot = len(live), f & 1
        pics, keep = (Picture * k)(), []
        for j, i in enumerate(live):
            pics[j], t = upload(made[i][5][f], made[i][2], made[i][3], LAYOUTS[(i + f) % 3], seed=100 * i + f)
            keep.append(t)
        assert lib.hmr_gpu_enc_load_sources_device((C.c_void_p * k)(*[made[i][1] for i in live]), k, (C.c_int * k)(*([slot] * k)), pics, current_stream()) == 0, lib.hmr_gpu_last_error()
        del keep
        if pipelined and prev is not None and prev != live:
            call(prev, None)
        call(live, slot)
        prev = live
        which = [-1 if (i + f) % 3 else slot for i in live]
        targets = [Target(FORMS[(2 * i + f) % len(FORMS)], made[i][2], made[i][3], *rc.MATRIX_RANGES[(i + f) % 4], rng, bool((i + f) & 1)) for i in live]
        originals = [rc.yuv_to_rgb(made[i][5][f], made[i][2], made[i][3]) for i in live]
        ref_forms = [FORMS[(i + 3 * f + 1) % len(FORMS)] for i in live]
        refs = [Source(form, chans_of(form, rng, *o), "bt709", 0, rng, padded=bool(j & 1)) for j, (form, o) in enumerate(zip(ref_forms, originals))]
        sums = new_sums(k)
        export_rgb(lib, [made[i][1] for i in live], which, targets, refs, sums)
        finals = [Output(made[i][2], made[i][3], "tight_i420", seed=i) for i in live]
        assert lib.hmr_gpu_enc_export_pictures_device((C.c_void_p * k)(*[made[i][1] for i in live]), k, (Picture * k)(*[o.pic for o in finals]), None, None, current_stream()) == 0, lib.hmr_gpu_last_error()
        for j, i in enumerate(live):
            w, h = made[i][2], made[i][3]
            yuv = finals[j].picture() if which[j] < 0 else b"".join(made[i][5][f])
            assert which[j] >= 0 or hashlib.md5(yuv).hexdigest() == GOLD[BATCH_CASES[i]]["recon_md5"][f]
            want = re_.restate_bytes(yuv, w, h, targets[j].matrix, targets[j].full)
            targets[j].check(want)
            assert sums[j].tolist() == re_.numpy_ssd(originals[j], want), (BATCH_CASES[i], f, which[j], ref_forms[j])      # (every form quantises back to the original's 8 bits)
    if pipelined:
        call(prev, None)
    for i, case in enumerate(BATCH_CASES):
        assert len(streams[i]) == GOLD[case]["stream_bytes"] and hashlib.md5(streams[i]).hexdigest() == GOLD[case]["stream_md5"], case
    for m in made:
        drop(lib, m[0], m[1])


# ---- ordering ----
def test_rgb_egress_is_ordered_against_the_consumer_stream(gpu):
    """The mirror of the egress and ingest stream tests: the output tensor is overwritten and the reference picture is produced on a torch side stream behind so much queued
    work that neither has happened when the export call returns; that stream is the call's consumer stream.  The reference's memory is overwritten on it right after the
    call, and copies of the output and the sums are queued there - nothing is synchronised by the test."""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    g, q = GOLD[case], RGB_GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    clean = [torch.from_numpy(np.frombuffer(b"".join(planes), np.uint8).copy()).cuda() for planes in clip]
    originals = [torch.from_numpy(np.stack(rc.yuv_to_rgb(planes, w, h))).cuda() for planes in clip]
    out = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")
    staging = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")
    copies = [torch.zeros_like(out) for _ in clip]
    sums, sums_copies = new_sums(), [new_sums() for _ in clip]
    ballast = torch.ones(1 << 28, dtype=torch.float32, device="cuda")      # 1 GB
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ballast.mul_(1.0)
    torch.cuda.synchronize()      # (set-up is over: from here on nothing waits on the host but the encode calls themselves)
    planar = lambda t: rc.descriptor(rc.RGB_PLANAR8, 0, (0, 0, 0), [t[c].data_ptr() for c in range(3)], [w] * 3, "bt709", 0)
    out_pic, ref_pic = planar(out), planar(staging)
    src = Picture(format=0, reserved=0)
    buf, n, stream, pending = C.create_string_buffer(1 << 20), C.c_long(), b"", []
    for f in range(len(clip)):
        base = clean[f].data_ptr()
        src.plane[0], src.plane[1], src.plane[2] = base, base + w * h, base + w * h * 5 // 4
        src.pitch[0], src.pitch[1], src.pitch[2] = w, w // 2, w // 2
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(src), current_stream()) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        ready = torch.cuda.Event()
        with torch.cuda.stream(side):
            for _ in range(40):
                ballast.mul_(1.0)
            out.fill_(0x55)
            sums.fill_(-1)
            staging.copy_(originals[f], non_blocking=True)
            ready.record(side)
        assert lib.hmr_gpu_enc_export_picture_rgb_device(enc, -1, C.byref(out_pic), C.byref(ref_pic), C.c_void_p(sums.data_ptr()), C.c_void_p(side.cuda_stream)) == 0, lib.hmr_gpu_last_error()
        pending.append(not ready.query())
        with torch.cuda.stream(side):
            staging.fill_(0x33)
            copies[f].copy_(out, non_blocking=True)
            sums_copies[f].copy_(sums, non_blocking=True)
    torch.cuda.synchronize()
    drop(lib, ctx, enc)
    assert all(pending), f"the output had already been overwritten when the export call returned (frames {pending}): the test did not exercise the ordering"
    for f in range(len(clip)):
        assert md5s(copies[f].cpu().numpy()) == q["rgb_md5"][f], f
        assert sums_copies[f][0].tolist() == q["ssd"][f], f
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


# ---- refusals ----
def test_refusals_leave_the_encoder_working(gpu):
    """every refusal of the header's list is HMR_GPU_ERR_ARG with a text that names the field, nothing is queued, and the encoder then still produces its fixture's stream.
    (Freed tensors are deliberately not tried.)"""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    g = GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    ctx2, fresh = make_encoder(lib, case)[:2]
    st = current_stream()
    rng = np.random.default_rng(2)
    buf, n, stream = C.create_string_buffer(1 << 20), C.c_long(), b""
    src, keep = upload(clip[0], w, h, "tight_i420")
    for e in (enc, fresh):
        assert lib.hmr_gpu_enc_load_source_device(e, 0, C.byref(src), st) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_encode_source(enc, 0, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
    stream += buf.raw[:n.value]
    out, planar = Target("rgba", w, h, "bt709", 0, rng), Target("f32", w, h, "bt601", 1, rng)
    ref_rgb = rc.noise(rng, w, h)
    ref = Source("planar8", ref_rgb, "bt709", 0, rng)
    sums = new_sums(513)
    dev = C.c_void_p(sums.data_ptr())

    def many(encs, which, outs, refs, ssd, n=None):
        k = len(encs)
        rc_ = lib.hmr_gpu_enc_export_pictures_rgb_device((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*which) if which is not None else None,
                                                         (rc.RgbPicture * k)(*outs) if outs is not None else None, (rc.RgbPicture * k)(*refs) if refs is not None else None, ssd, st)
        return rc_, lib.hmr_gpu_last_error()

    def changed(pic, **kw):
        p = rc.RgbPicture.from_buffer_copy(pic)
        for k, v in kw.items():
            if k[-1].isdigit():
                getattr(p, k[:-1])[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return p

    refused = {
        "n = 0": (many([enc], [-1], [out.pic], None, None, n=0), b"n = 0"),
        "n = 513": (many([enc] * 513, [-1] * 513, [out.pic] * 513, None, None), b"n = 513"),
        "NULL encoders": ((lib.hmr_gpu_enc_export_pictures_rgb_device(None, 1, (C.c_int * 1)(-1), C.byref(out.pic), None, None, st), lib.hmr_gpu_last_error()), b"encoders"),
        "a NULL encoder": (many([enc, None], [-1, -1], [out.pic, out.pic], None, None), b"encoder is NULL"),
        "NULL encoder (single call)": ((lib.hmr_gpu_enc_export_picture_rgb_device(None, -1, C.byref(out.pic), None, None, st), lib.hmr_gpu_last_error()), b"encoder is NULL"),
        "NULL which": (many([enc], None, [out.pic], None, None), b"which"),
        "both outs and refs NULL": (many([enc], [-1], None, None, None), b"neither outs nor refs"),
        "nothing asked for (single call)": ((lib.hmr_gpu_enc_export_picture_rgb_device(enc, -1, None, None, None, st), lib.hmr_gpu_last_error()), b"neither outs nor refs"),
        "refs without dev_ssd": (many([enc], [-1], [out.pic], [ref.pic], None), b"dev_ssd"),
        "dev_ssd without refs": (many([enc], [-1], [out.pic], None, dev), b"dev_ssd"),
        "which = -2": (many([enc], [-2], [out.pic], None, None), b"which"),
        "a slot that does not exist": (many([enc, enc], [0, 1], [out.pic, out.pic], None, None), b"which"),
        "which = -1 without an encoded picture": (many([enc, fresh], [-1, -1], [out.pic, out.pic], None, None), b"which"),
        "outs: unknown format": (many([enc], [-1], [changed(out.pic, format=4)], None, None), b"format"),
        "outs: unknown matrix": (many([enc], [-1], [changed(out.pic, matrix=2)], None, None), b"matrix"),
        "outs: full_range 2": (many([enc], [-1], [changed(planar.pic, full_range=2)], None, None), b"full_range"),
        "outs: reserved": (many([enc], [-1], [changed(out.pic, reserved=1)], None, None), b"reserved"),
        "outs: pixel_bytes 5": (many([enc], [-1], [changed(out.pic, pixel_bytes=5)], None, None), b"pixel_bytes"),
        "outs: offset repeated": (many([enc], [-1], [changed(out.pic, offset2=0)], None, None), b"offset[2]"),
        "outs: missing plane": (many([enc], [0], [changed(planar.pic, plane1=None)], None, None), b"plane[1]"),
        "outs: second plane with PACKED8": (many([enc], [-1], [changed(out.pic, plane1=out.pic.plane[0])], None, None), b"plane[1]"),
        "outs: pitch below a row": (many([enc, enc], [-1, 0], [out.pic, changed(out.pic, pitch0=4 * w - 1)], None, None), b"pitch[0]"),
        "outs: float plane not element-aligned": (many([enc], [-1], [changed(planar.pic, plane2=planar.pic.plane[2] + 1)], None, None), b"plane[2]"),
        "refs: unknown matrix": (many([enc], [-1], None, [changed(ref.pic, matrix=-1)], dev), b"matrix"),
        "refs: pitch below a row": (many([enc], [-1], [out.pic], [changed(ref.pic, pitch1=w - 1)], dev), b"pitch[1]"),
        "refs: negative pitch": (many([enc], [0], None, [changed(ref.pic, pitch2=-w)], dev), b"pitch[2]"),
    }
    # memory that is not the device's: a plain host address is enough, the library only asks for the pointer's attributes and never follows it
    host, host_sums = np.zeros((h, w), np.float32), np.full(3, -7, np.int64)
    refused["an output plane in host memory"] = (many([enc], [-1], [changed(planar.pic, plane1=host.ctypes.data)], None, None), b"plane[1]")
    refused["a reference plane in host memory"] = (many([enc], [-1], None, [changed(ref.pic, plane2=host.ctypes.data)], dev), b"plane[2]")
    refused["dev_ssd in host memory"] = (many([enc], [-1], None, [ref.pic], C.c_void_p(host_sums.ctypes.data)), b"dev_ssd")
    assert not host.any() and (host_sums == -7).all()
    if torch.cuda.device_count() > 1:
        ctx4, enc4 = C.c_void_p(), C.c_void_p()
        assert lib.hmr_gpu_create(C.byref(ctx4), 1, None) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_create(ctx4, C.byref(ec.default_cfg(w, h, wpp=4)), C.byref(enc4)) == 0, lib.hmr_gpu_last_error()
        other = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda:1")
        refused["encoders on different devices"] = (many([enc, enc4], [-1, -1], [out.pic, out.pic], None, None), b"device")
        refused["an output plane on another device"] = (many([enc], [-1], [changed(planar.pic, plane1=other.data_ptr())], None, None), b"plane[1]")
        refused["a reference plane on another device"] = (many([enc], [-1], None, [changed(ref.pic, plane2=other.data_ptr())], dev), b"plane[2]")
        refused["dev_ssd on another device"] = (many([enc], [-1], None, [ref.pic], C.c_void_p(other.data_ptr())), b"dev_ssd")
        drop(lib, ctx4, enc4)
    for why, ((rc_, text), field) in refused.items():
        assert rc_ == ERR_ARG and text and field in text, (why, rc_, text)
    # nothing was written by the refused calls; the same encoder twice in one call is fine, and so is a slot of an encoder that has not encoded anything
    assert out.untouched() and planar.untouched() and sums.min().item() == -7
    rc_, text = many([enc, fresh], [-1, 0], [out.pic, planar.pic], [ref.pic, ref.pic], dev)
    assert rc_ == 0, text
    rec = final_yuv(lib, enc, w, h)
    out.check(re_.restate_bytes(rec, w, h, "bt709", 0))
    planar.check(re_.restate_bytes(clip[0], w, h, "bt601", 1))
    assert sums[0].tolist() == re_.numpy_ssd(ref_rgb, re_.restate_bytes(rec, w, h, "bt709", 0)) and sums[1].tolist() == re_.numpy_ssd(ref_rgb, re_.restate_bytes(clip[0], w, h, "bt601", 1))
    for f, planes in enumerate(clip):
        if f == 0:
            continue
        pic, t = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), st) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
    drop(lib, ctx, enc)
    drop(lib, ctx2, fresh)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


# ---- the Python classes ----
def test_encoder_class_export_rgb(gpu):
    """allocated results (planar of every dtype, packed of every order) and out= results (views and channel slices), source=True, reference= and psnr_rgb; a float16 result
    fed back as an RGBFrame to a second encoder loads the slot the uint8 result loads"""
    import torch
    case = "416x240"
    cfg, image_type, clip = config_of(case)
    w, h = cfg.width, cfg.height
    rng = np.random.default_rng(6)
    stream = b""
    with Encoder(cfg) as enc, Encoder(config_of(case)[0]) as second:
        with pytest.raises(RuntimeError):
            enc.export_rgb()
        for f, planes in enumerate(clip[:4]):
            stream += enc.encode(as_tensors(planes, w, h, f % 3, f), image_type)[0]
            rec = enc.export()[0].cpu().numpy().tobytes()
            matrix, full = rc.MATRIX_RANGES[f % 4]
            want = re_.restate_bytes(rec, w, h, matrix, full)
            original = rc.yuv_to_rgb(planes, w, h)
            reference, _ = rgb_frame("chw_f32" if f & 1 else "hwc4_bgra_view", *original, "bt601", 1, rng)
            # allocated: planar uint8 with sums, float16, float32
            got, sums = enc.export_rgb(matrix=matrix, full_range=full, reference=reference)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (3, h, w) and got.is_contiguous() and sums.dtype == torch.int64 and tuple(sums.shape) == (3,)
            assert np.array_equal(got.cpu().numpy(), np.stack(want))
            assert sums.tolist() == re_.numpy_ssd(original, want)
            assert all(abs(a - b) <= 1e-9 for a, b in zip(psnr_rgb(sums.tolist(), w, h)[:3], [10.0 * np.log10(255.0 * 255.0 * w * h / s) for s in sums.tolist()]))
            only = enc.export_rgb(out=False, matrix=matrix, full_range=full, reference=reference)
            assert only.tolist() == sums.tolist()
            halves, singles = enc.export_rgb(dtype=torch.float16, matrix=matrix, full_range=full), enc.export_rgb(dtype=torch.float32, matrix=matrix, full_range=full)
            assert halves.dtype == torch.float16 and singles.dtype == torch.float32
            assert np.array_equal(halves.cpu().numpy().view(np.uint16), re_.unit(np.stack(want), "f16").view(np.uint16))
            assert np.array_equal(singles.cpu().numpy().view(np.uint32), re_.unit(np.stack(want), "f32").view(np.uint32))
            # allocated: packed, every order over the frames
            for order in list(rc.FORMS)[f % 2:6:2]:
                packed = enc.export_rgb(order=order, matrix=matrix, full_range=full).cpu().numpy()
                pb, offs = rc.FORMS[order][1], rc.FORMS[order][2]
                assert packed.shape == (h, w, pb) and all(np.array_equal(packed[:, :, o], p) for o, p in zip(offs, want))
                assert pb == 3 or (packed[:, :, 6 - sum(offs)] == 255).all()
            # out=: a window of a larger packed tensor, channels 1 .. 3 of a four-channel float tensor
            big = torch.from_numpy(rng.integers(0, 256, (h + 2, w + 5, 4), dtype=np.uint8)).cuda()
            before = big.cpu().numpy().copy()
            frame = RGBFrame(big[1:1 + h, 3:3 + w], order="abgr", matrix=matrix, full_range=full)
            assert enc.export_rgb(out=frame) is frame.tensor
            after = big.cpu().numpy()
            assert all(np.array_equal(after[1:1 + h, 3:3 + w, 3 - c], want[c]) for c in range(3)) and (after[1:1 + h, 3:3 + w, 0] == 255).all()
            after[1:1 + h, 3:3 + w] = before[1:1 + h, 3:3 + w]
            assert np.array_equal(after, before)
            four = torch.full((4, h, w), 7.0, dtype=torch.float32, device="cuda")
            got, sums2 = enc.export_rgb(out=RGBFrame(four[1:], matrix=matrix, full_range=full), reference=reference)
            assert got.data_ptr() == four[1:].data_ptr() and sums2.tolist() == sums.tolist()
            assert (four[0] == 7.0).all().item() and np.array_equal(four[1:].cpu().numpy().view(np.uint32), re_.unit(np.stack(want), "f32").view(np.uint32))
            # the encoded source as RGB
            src = enc.export_rgb(source=True, matrix=matrix, full_range=full)
            assert np.array_equal(src.cpu().numpy(), np.stack(re_.restate_bytes(planes, w, h, matrix, full)))
            # fed back: the float16 picture loads the slot the uint8 picture loads
            second.encode(RGBFrame(halves, matrix=matrix, full_range=full))
            from_halves = second.source().cpu().numpy().tobytes()
            second.encode(RGBFrame(enc.export_rgb(matrix=matrix, full_range=full), matrix=matrix, full_range=full))
            assert second.source().cpu().numpy().tobytes() == from_halves == b"".join(p.tobytes() for p in rc.restate(*want, matrix, full))
        with pytest.raises(ValueError):
            enc.export_rgb(out=False)
        with pytest.raises(TypeError):
            enc.export_rgb(out=torch.zeros((3, h, w), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            enc.export_rgb(order="grb")
    assert stream


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_encoder_class_export_rgb(gpu, pipelined):
    made = [config_of(case) for case in BATCH_CASES]
    streams = [b"" for _ in made]
    rng = np.random.default_rng(8)
    with BatchEncoder([m[0] for m in made], pipelined=pipelined) as enc:
        with pytest.raises(RuntimeError):
            enc.export_rgb()
        for f in range(max(len(m[2]) for m in made)):
            frames = [as_tensors(m[2][f], m[0].width, m[0].height, (i + f) % 3, 100 * i + f) if f < len(m[2]) else None for i, m in enumerate(made)]
            for i, au in enumerate(enc.step(frames, [m[1] for m in made])):
                streams[i] += au
            # the pictures of the frames just given - in pipelined mode their access units are still outstanding
            matrix, full = rc.MATRIX_RANGES[f % 4]
            originals = [rc.yuv_to_rgb(m[2][f], m[0].width, m[0].height) if frames[i] is not None else None for i, m in enumerate(made)]
            references = [rgb_frame("chw_u8" if (i + f) & 1 else "hwc3", *o, "bt709", 0, rng)[0] if o is not None else None for i, o in enumerate(originals)]
            recs = enc.export()[0]
            if f % 3 == 0:
                pictures, sums = enc.export_rgb(dtype=torch_dtype(f), matrix=matrix, full_range=full, reference=references)
            elif f % 3 == 1:
                outs = [RGBFrame(new_packed(m[0].width, m[0].height), order="bgra", matrix=matrix, full_range=full) if frames[i] is not None else None for i, m in enumerate(made)]
                pictures, sums = enc.export_rgb(out=outs, reference=references)
                assert all(p is None or p is o.tensor for p, o in zip(pictures, outs))
            else:
                pictures, sums = enc.export_rgb(order="rgb", matrix=matrix, full_range=full, source=True), enc.export_rgb(out=False, matrix=matrix, full_range=full, reference=references, source=True)
            assert tuple(sums.shape) == (len(made), 3)
            for i, (m, case) in enumerate(zip(made, BATCH_CASES)):
                if frames[i] is None:
                    assert pictures[i] is None and sums[i].tolist() == [-1, -1, -1]
                    continue
                w, h = m[0].width, m[0].height
                yuv = b"".join(m[2][f]) if f % 3 == 2 else recs[i].cpu().numpy().tobytes()
                want = re_.restate_bytes(yuv, w, h, matrix, full)
                got = pictures[i].cpu().numpy()
                if f % 3 == 0:
                    form = {1: "planar8", 2: "f16", 4: "f32"}[got.dtype.itemsize]
                    expect = re_.unit(np.stack(want), form) if form != "planar8" else np.stack(want)
                    assert got.tobytes() == expect.tobytes(), (case, f)
                elif f % 3 == 1:
                    assert all(np.array_equal(got[:, :, 2 - c], want[c]) for c in range(3)) and (got[:, :, 3] == 255).all(), (case, f)
                else:
                    assert all(np.array_equal(got[:, :, c], want[c]) for c in range(3)), (case, f)
                assert sums[i].tolist() == re_.numpy_ssd(originals[i], want), (case, f)
        for i, au in enumerate(enc.flush()):
            streams[i] += au
    for i, case in enumerate(BATCH_CASES):
        assert len(streams[i]) == GOLD[case]["stream_bytes"] and hashlib.md5(streams[i]).hexdigest() == GOLD[case]["stream_md5"], case


def torch_dtype(f):
    import torch
    return [torch.uint8, torch.float16, torch.float32][(f // 3) % 3]


def new_packed(w, h):
    import torch
    return torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
