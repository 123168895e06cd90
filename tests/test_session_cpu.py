"""CPU: the decode-session boundary without a GPU (include/vc_engine.h vc_session_*): the symbols are exported and bound, refuse a NULL
engine, the Python surface is importable, and the session's kernels are in the compiled gfx950 code with no scratch memory."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_store_scan as isa  # noqa: E402

SESSION_SYMBOLS = ("vc_session_open", "vc_session_submit", "vc_session_advance", "vc_session_fetch", "vc_session_stats", "vc_session_close")


@pytest.fixture(scope="module")
def lib():
    from voicecraft_amd import _lib
    return _lib.load()


def test_session_symbols_are_exported_bound_and_refuse_a_null_engine(lib):
    from voicecraft_amd import _lib
    for name in SESSION_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES and _lib.PROTOTYPES[name][0] is C.c_int, name
    n, idle, t, v = C.c_int(0), C.c_int(0), C.c_int(0), (C.c_int64 * 8)()
    sc = _lib.SampleCfg()
    assert lib.vc_session_open(None, 1, C.byref(sc), None) == -1
    assert lib.vc_session_submit(None, None, 1, None, 0, 0, C.byref(t)) == -1
    assert lib.vc_session_advance(None, None, 0, C.byref(n), C.byref(idle)) == -1
    assert lib.vc_session_fetch(None, 1, None, 0, None, None) == -1
    assert lib.vc_session_stats(None, v) == -1
    assert lib.vc_session_close(None) == -1


def test_python_surface_is_importable():
    import voicecraft_amd
    from voicecraft_amd import DecodeSession, inference_tts_queue
    from voicecraft_amd.engine import VoiceCraftEngine
    assert callable(inference_tts_queue) and callable(VoiceCraftEngine.inference_tts_queue) and callable(VoiceCraftEngine.open_session)
    for m in ("submit", "poll", "drain", "stats", "fetch", "close", "__enter__", "__exit__"):
        assert callable(getattr(DecodeSession, m)), m
    assert voicecraft_amd.DecodeSession is DecodeSession


@pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
def test_session_kernels_are_compiled_for_gfx950_without_scratch(tmp_path):
    """sample_session_k<false> (a step of the session's graph), sample_session_k<true> (the first sample of the admitted rows) and
    session_turn_k (re-pack + admission): present, no scratch, at most one store that waits for an earlier one (the rule of
    tests/test_isa.py); the one-shot sampler keeps its own kernel next to them."""
    src = os.path.join(ROOT, "voicecraft_amd", "csrc", "vc_tokens.hip")
    dst = str(tmp_path / "vc_tokens.s")
    r = subprocess.run([isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src, "-o", dst],
                       cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kern = {isa.demangle(n).replace("void ", ""): v for n, v in isa.kernels(open(dst).read()).items()}
    for prefix in ("sample_session_k<false>(", "sample_session_k<true>(", "session_turn_k("):
        sel = {n: v for n, v in kern.items() if n.startswith(prefix)}
        assert len(sel) == 1, (prefix, sorted(kern))
        for name, (body, scratch, vgpr) in sel.items():
            assert scratch == 0 and "scratch_" not in body, (name, scratch)
            assert isa.store_chains(body)[0] <= 1, (name, isa.store_chains(body))
    assert any(n.startswith("sample_fused_k(") for n in kern)
    # the session's step kernel draws with the request's own key and stamps retirements: two loads through SampleDyn the one-shot form lacks
    (body_s, _, _), = [v for n, v in kern.items() if n.startswith("sample_session_k<false>(")]
    (body_f, _, _), = [v for n, v in kern.items() if n.startswith("sample_fused_k(")]
    assert body_s != body_f
