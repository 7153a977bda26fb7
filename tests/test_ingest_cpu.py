"""Pictures in device memory (include/homer_gpu.h section 12d), the parts that need no GPU: the host check of a picture descriptor, the configuration struct of
homerhevc_amd/encoder.py against the tests' own mirror, and what the package imports."""
import ctypes as C
import subprocess
import sys

import pytest

import encoder_cases as ec
import libs
from homerhevc_amd.encoder import PIC_I420, PIC_NV12, EncoderConfig, Picture

ERR_ARG = -3
W, H = 416, 240
SOME = 0x1000          # any non-NULL value: the check never follows a pointer


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    lib = C.CDLL(libs.GPU_SO)
    lib.hmr_gpu_picture_check.argtypes = [C.POINTER(Picture), C.c_int, C.c_int]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


def picture(fmt, planes, pitches, reserved=0):
    p = Picture(format=fmt, reserved=reserved)
    for c in range(3):
        p.plane[c] = planes[c]
        p.pitch[c] = pitches[c]
    return p


def i420(**kw):
    d = dict(fmt=PIC_I420, planes=[SOME, SOME + 1, SOME + 2], pitches=[W + 13, W // 2 + 7, W // 2 + 3])
    d.update(kw)
    return picture(**d)


def nv12(**kw):
    d = dict(fmt=PIC_NV12, planes=[SOME, SOME + 1, None], pitches=[W + 6, W + 6, 0])
    d.update(kw)
    return picture(**d)


def test_descriptors_that_are_accepted(lib):
    assert lib.hmr_gpu_picture_check(C.byref(i420()), W, H) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_picture_check(C.byref(nv12()), W, H) == 0, lib.hmr_gpu_last_error()
    # a pitch of exactly a row's bytes
    assert lib.hmr_gpu_picture_check(C.byref(i420(pitches=[W, W // 2, W // 2])), W, H) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_picture_check(C.byref(nv12(pitches=[W, W, 0])), W, H) == 0, lib.hmr_gpu_last_error()


REFUSED = {
    "unknown format": (i420(fmt=2), W, H, b"format"),
    "negative format": (i420(fmt=-1), W, H, b"format"),
    "reserved": (i420(reserved=1), W, H, b"reserved"),
    "no luma plane": (i420(planes=[None, SOME, SOME]), W, H, b"plane[0]"),
    "no U plane": (i420(planes=[SOME, None, SOME]), W, H, b"plane[1]"),
    "no V plane": (i420(planes=[SOME, SOME, None]), W, H, b"plane[2]"),
    "no UV plane": (nv12(planes=[SOME, None, None]), W, H, b"plane[1]"),
    "third plane with NV12": (nv12(planes=[SOME, SOME, SOME]), W, H, b"plane[2]"),
    "luma pitch below the width": (i420(pitches=[W - 1, W // 2, W // 2]), W, H, b"pitch[0]"),
    "U pitch below half the width": (i420(pitches=[W, W // 2 - 1, W // 2]), W, H, b"pitch[1]"),
    "V pitch below half the width": (i420(pitches=[W, W // 2, W // 2 - 1]), W, H, b"pitch[2]"),
    "UV pitch below the width": (nv12(pitches=[W, W - 1, 0]), W, H, b"pitch[1]"),
    "negative pitch": (i420(pitches=[-(W + 16), W // 2, W // 2]), W, H, b"pitch[0]"),
    "negative chroma pitch": (nv12(pitches=[W, -W, 0]), W, H, b"pitch[1]"),
    "odd width": (i420(), W + 1, H, b"width"),
    "odd height": (i420(), W, H - 1, b"height"),
    "zero width": (i420(), 0, H, b"width"),
    "negative height": (nv12(), W, -2, b"height"),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_descriptors_that_are_refused(lib, why):
    pic, w, h, field = REFUSED[why]
    assert lib.hmr_gpu_picture_check(C.byref(i420()), W, H) == 0      # (so that the error text below is this refusal's)
    assert lib.hmr_gpu_picture_check(C.byref(pic), w, h) == ERR_ARG
    text = lib.hmr_gpu_last_error()
    assert text and field in text, text


def test_null_descriptor_is_refused(lib):
    assert lib.hmr_gpu_picture_check(None, W, H) == ERR_ARG
    assert lib.hmr_gpu_last_error()


def test_configuration_struct_is_the_tests_mirror():
    assert [(n, t) for n, t in EncoderConfig._fields_] == [(n, t) for n, t in ec.EncCfg._fields_]
    assert C.sizeof(EncoderConfig) == C.sizeof(ec.EncCfg)
    for name, _ in ec.EncCfg._fields_:
        assert getattr(EncoderConfig, name).offset == getattr(ec.EncCfg, name).offset, name


@pytest.mark.parametrize("size", [(416, 240), (1920, 1080)])
@pytest.mark.parametrize("fields", [{}, {"qp": 22, "performance_mode": 0}, {"bitrate_mode": 1, "bitrate": 400}, {"wfpp_num_threads": 4},
                                    {"bitrate_mode": 2, "bitrate": 1500, "performance_mode": 1, "wfpp_num_threads": 8, "sample_adaptive_offset": 0},
                                    {"rd_mode": 1, "max_intra_tr_depth": 4, "num_enc_engines": 2, "chroma_qp_offset": 0, "motion_estimation_precision": 1}])
def test_configuration_defaults_are_default_cfg(size, fields):
    mine, theirs = EncoderConfig(*size, **fields), ec.default_cfg(*size, **fields)
    for name, _ in ec.EncCfg._fields_:
        assert getattr(mine, name) == getattr(theirs, name), name
    assert bytes(mine) == bytes(theirs)


def test_configuration_keywords():
    c = EncoderConfig(416, 240, bitrate=400, vbv_size=1000, vbv_init=10)
    assert (c.vbv_size, c.vbv_init) == (1000, 10)      # given: kept
    with pytest.raises(TypeError):
        EncoderConfig(416, 240, no_such_field=1)


def in_a_fresh_process(code):
    return subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {libs.ROOT!r}); " + code], capture_output=True, text=True, timeout=300)


def test_package_import_does_not_import_torch():
    r = in_a_fresh_process("import homerhevc_amd; assert 'torch' not in sys.modules, 'torch imported'; assert homerhevc_amd.Encoder and homerhevc_amd.BatchEncoder and homerhevc_amd.EncoderConfig")
    assert r.returncode == 0, r.stderr


def test_encoder_module_imports_without_a_gpu_and_construction_fails_loudly():
    r = in_a_fresh_process("import homerhevc_amd.encoder as m; assert 'torch' not in sys.modules, 'torch imported'; print(sorted(n for n in dir(m) if n[0].isupper()))")
    assert r.returncode == 0, r.stderr
    assert "BatchEncoder" in r.stdout and "EncoderConfig" in r.stdout
    import torch
    if torch.cuda.is_available():
        return
    from homerhevc_amd.encoder import BatchEncoder, Encoder
    with pytest.raises(RuntimeError, match="no HIP device|HIP"):
        Encoder(EncoderConfig(416, 240))
    with pytest.raises(RuntimeError, match="no HIP device|HIP"):
        BatchEncoder([EncoderConfig(416, 240, wfpp_num_threads=4)])
