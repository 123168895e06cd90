"""CPU: the carried-state LSTM kernels of the chunked decode do the one-shot kernels' arithmetic.

The stream's bit-identity with vc_codec_decode rests on lstm_persist_k<NQ, true> / lstm_wave_k<NQ, true> rounding every
sum where the one-shot instantiations do.  The source is shared, but which multiply the compiler fuses into which add
(-ffp-contract=fast) is its choice per instantiation: a first form of the carried persistent kernel, whose step-0
selects were compile-time constants, was scheduled differently and moved the waveform by 2e-5.  So the property is
checked on the ISA: the sequence of floating-point opcodes (packed / scalar multiply, add, fused multiply-add) of each
carried instantiation equals the one-shot's.  tests/test_gpu_stream.py checks the values themselves."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_store_scan as isa  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")

FP = re.compile(r"^\s*(v_(?:pk_)?(?:mul|add|sub|fma|fmac|fmaak|fmamk|mac|mad)_(?:legacy_)?f32\S*)\s+(.*?)\s*(?:;.*)?$")


@pytest.fixture(scope="module")
def codec_kernels(tmp_path_factory):
    src = os.path.join(ROOT, "voicecraft_amd", "csrc", "vc_codec.hip")
    dst = os.path.join(str(tmp_path_factory.mktemp("isa")), "vc_codec.s")
    subprocess.run([isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src, "-o", dst],
                   cwd=os.path.dirname(src), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return {isa.demangle(n): v for n, v in isa.kernels(open(dst).read()).items()}


def _fp_ops(body):
    return [(m.group(1), m.group(2)) for m in map(FP.match, body.splitlines()) if m]


def _find(kernels, base, nq, carry):
    want = f"{base}<{nq}, {'true' if carry else 'false'}>"
    hit = [v for n, v in kernels.items() if want in n]
    assert len(hit) == 1, (want, sorted(kernels))
    return hit[0]


@pytest.mark.parametrize("base,nq", [("lstm_persist_k", 2), ("lstm_persist_k", 4), ("lstm_wave_k", 1), ("lstm_wave_k", 2),
                                     ("lstm_wave_k", 3), ("lstm_wave_k", 4)])
def test_carried_lstm_forms_keep_the_one_shot_arithmetic(codec_kernels, base, nq):
    one, _, _ = _find(codec_kernels, base, nq, False)
    car, scratch, _ = _find(codec_kernels, base, nq, True)
    a, b = _fp_ops(one), _fp_ops(car)
    assert len(a) > 100, len(a)
    assert [o for o, _ in a] == [o for o, _ in b], "the carried form fuses / orders its floating-point operations differently"
    assert scratch == 0


def test_the_persistent_carried_form_keeps_its_bounded_wait(codec_kernels):
    """the hand-off of the carried form is the one-shot form's: same number of polling loads and sleeps, one error store"""
    for nq in (2, 4):
        one, _, _ = _find(codec_kernels, "lstm_persist_k", nq, False)
        car, _, _ = _find(codec_kernels, "lstm_persist_k", nq, True)
        for pat in (r"s_sleep", r"s_barrier"):
            assert len(re.findall(pat, car)) == len(re.findall(pat, one)) > 0, pat
