"""-m gpu: num_enc_engines > 1 with ONE WPP thread, all engines in one object (hmr_gpu_enc_create): the picture runs CTU by CTU on the pool's raster schedule, each frame on
the persistent state of engine n mod E.  The stream, every reconstructed picture and the decoder's view of them must be what the compiled reference produced under the engine
turnstile (tests/golden/streams.json) - at a fixed QP and under rate control."""
import hashlib

import pytest

import decoder_check
from test_gpu_stream import GOLD, encode, gpu  # noqa: F401  (gpu: the fixture with the library and a context)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["416x240_eng2", "416x240_cbr300_eng2"])
def test_engines_with_one_thread_reproduce_the_reference_engine_stream(gpu, case):  # noqa: F811
    raw = []
    stream, recon = encode(gpu, case, raw_recon=raw)
    g = GOLD[case]
    assert recon == g["recon_md5"], [f for f in range(g["frames"]) if recon[f] != g["recon_md5"][f]]
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]
    decoder_check.check(stream, g, case, raw)
