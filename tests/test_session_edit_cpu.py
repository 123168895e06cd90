"""CPU: the boundary of editing requests and per-request controls in a decode session (include/vc_engine.h vc_session_submit_ctl,
vc_session_submit_edit, vc_request_ctl), without a GPU: exported, bound, refusing a NULL engine, the struct 16 bytes on both sides."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from voicecraft_amd import _lib
    return _lib.load()


def test_new_symbols_are_exported_bound_and_refuse_a_null_engine(lib):
    from voicecraft_amd import _lib
    for name in ("vc_session_submit_ctl", "vc_session_submit_edit"):
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES and _lib.PROTOTYPES[name][0] is C.c_int, name
    t = C.c_int(0)
    ctl = _lib.RequestCtl(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=-1)
    iv, mv = (C.c_int32 * 2)(2, 4), (C.c_int32 * 2)(0, 0)
    assert lib.vc_session_submit_ctl(None, None, 1, None, 0, C.byref(ctl), 0, C.byref(t)) == -1
    assert lib.vc_session_submit_ctl(None, None, 1, None, 0, None, 0, C.byref(t)) == -1
    assert lib.vc_session_submit_edit(None, None, 1, None, 8, iv, 1, mv, C.byref(ctl), 0, C.byref(t)) == -1
    assert lib.vc_session_submit_edit(None, None, 1, None, 8, iv, 1, mv, None, 0, C.byref(t)) == -1


def test_request_ctl_is_16_bytes_on_both_sides_of_the_binding():
    from voicecraft_amd._lib import RequestCtl
    assert C.sizeof(RequestCtl) == 16
    assert [(n, getattr(RequestCtl, n).offset) for n, _ in RequestCtl._fields_] == [
        ("top_k", 0), ("top_p", 4), ("temperature", 8), ("stop_repetition", 12)]
    # the header's declaration: four 4-byte members in the same order
    src = open(os.path.join(ROOT, "include", "vc_engine.h")).read()
    m = re.search(r"typedef struct vc_request_ctl \{(.*?)\} vc_request_ctl;", src, flags=re.S)
    assert m, "vc_request_ctl is not declared in include/vc_engine.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    members = re.findall(r"\b(int32_t|float)\s+(\w+)\s*;", body)
    assert members == [("int32_t", "top_k"), ("float", "top_p"), ("float", "temperature"), ("int32_t", "stop_repetition")], members
    # ... and the device side agrees: the kernels copy one entry as a 16-byte quad (vc_tokens.hip session_turn_k)
    tok = open(os.path.join(ROOT, "voicecraft_amd", "csrc", "vc_tokens.hip")).read()
    assert "reinterpret_cast<const uint4*>(a.adm_ctl + tid)" in tok


def test_python_surface():
    import voicecraft_amd
    from voicecraft_amd import DecodeSession, inference_queue
    from voicecraft_amd.engine import VoiceCraftEngine
    assert callable(DecodeSession.submit_edit) and callable(VoiceCraftEngine.inference_queue) and callable(inference_queue)
    assert voicecraft_amd.inference_queue is inference_queue
    assert DecodeSession.CONTROLS == ("top_k", "top_p", "temperature", "stop_repetition")
